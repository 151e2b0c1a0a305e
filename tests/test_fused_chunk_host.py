"""CPU check of the fused sweep's chunk rule (csrc/fs_chunk.h::fs_chunk_rule, which `fs_chunk_len` and `fused_ws` share).  tests/hostsim_chunk/chunk_check.cpp is a
stand-alone program on that header (plain g++, built as tests/test_fused_mid_host.py builds its own).  The rule equals tests/fused_cases.py::chunk_len for every
C in 1 .. 1100 at T in {64, 70, 97, 130} on 256 compute units; it gives 64 at 256 x 65536, 256 x 65473, 512 x 32768 and from 1024 chains at any T >= 64; 32 at
256 x 65472, 256 x 32768, 130 x 3001 and 255 x 65536; and never more than max(T, 2).  (The row window of pass AC that the same header was to hold was measured
and not kept -- DESIGN.md section 4 -- so there is no window walk to check.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_rule_table(tmp_path):
    exe = str(tmp_path / "chunk_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "hostsim_chunk", "chunk_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "rule table ok" in res.stdout and "FAILED" not in res.stdout and "DIFFERENT" not in res.stdout
