#!/usr/bin/env python3
"""Per-kernel durations (mean / min / max / standard deviation over the launches) of the fused sweep's kernels from a rocprofv3 --kernel-trace CSV, and their
HBM traffic from two separate --pmc passes (FETCH_SIZE, WRITE_SIZE; FETCH_SIZE doubled as tools/pmc_traffic.py does).

  python tools/fs_pass_profile.py <dir with *_kernel_trace.csv> [<dir with the FETCH_SIZE pass> <dir with the WRITE_SIZE pass>] > profiles/<name>.txt"""
import collections
import csv
import glob
import math
import os
import re
import subprocess
import sys

# (k_fs_esfix and k_aff_aggs: the three launches k_fs_mid replaced -- kept so that a trace of an older library reads the same way)
KEEP = re.compile(r"^k_fs_(ac|e|mid|esfix|head|accept)<|^k_aff_aggs<|^k_filter_t0<|^k_rng|^k_fs_stats<")


def find(d, pat):
    f = sorted(glob.glob(os.path.join(d, "**", pat), recursive=True))
    if not f:
        sys.exit(f"no {pat} under {d}")
    return f[0]


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return [re.sub(r"\(.*$", "", re.sub(r"^void ax::", "", d)) for d in out]


def durations(path):
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        acc[r["Kernel_Name"]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    names = list(acc)
    return {d: acc[n] for n, d in zip(names, demangle(names))}


def counter(path):
    acc = collections.defaultdict(list)
    for r in csv.DictReader(open(path)):
        acc[r["Kernel_Name"]].append(float(r["Counter_Value"]) * 1024.0)
    names = list(acc)
    return {d: sum(acc[n]) / len(acc[n]) for n, d in zip(names, demangle(names))}


if __name__ == "__main__":
    dur = durations(find(sys.argv[1], "*kernel_trace.csv"))
    rd = wr = {}
    if len(sys.argv) >= 4:
        rd, wr = counter(find(sys.argv[2], "*counter_collection.csv")), counter(find(sys.argv[3], "*counter_collection.csv"))
    print(f"{'kernel':58s} {'calls':>6s} {'mean_us':>9s} {'min_us':>9s} {'max_us':>9s} {'sd_us':>7s} {'read_MB':>9s} {'write_MB':>9s} {'GB/s':>8s}")
    for k in sorted(dur, key=lambda k: -sum(dur[k])):
        if not KEEP.match(k):
            continue
        v = dur[k]
        mean = sum(v) / len(v)
        sd = math.sqrt(sum((x - mean) ** 2 for x in v) / max(1, len(v) - 1))
        r, w = 2.0 * rd.get(k, float("nan")), wr.get(k, float("nan"))
        print(f"{k[:58]:58s} {len(v):6d} {mean:9.1f} {min(v):9.1f} {max(v):9.1f} {sd:7.2f} {r / 1e6:9.1f} {w / 1e6:9.1f} {(r + w) / mean / 1e3:8.0f}")
