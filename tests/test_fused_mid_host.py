"""CPU check of the claim the fused sweep's between-pass kernel rests on (csrc/fused_shared.h: k_fs_gtab + k_fs_mid): scanning the offsets alone, with each
Kogge-Stone stage's matrix read from a table built by the same schedule on the chain-shared matrices, gives the exclusive prefixes of the full-element
scan (k_aff_aggs) byte for byte.  tests/hostsim_mid/mid_check.cpp is a stand-alone program on csrc/kalman_math.h (built as tests/hostsim builds its
harness: plain g++, no contraction); it covers nchunk in {1, 2, 3, 255, 256, 257, 513, 2048} at D in {1, 4}, fp64 and fp32, and compares with memcmp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_offsets_only_scan_equals_the_full_element_scan_bit_for_bit(tmp_path):
    exe = str(tmp_path / "mid_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "hostsim_mid", "mid_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("equal") == 32 and "DIFFERENT" not in res.stdout
