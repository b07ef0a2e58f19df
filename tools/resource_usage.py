#!/usr/bin/env python3
"""Table of the kernels' register / scratch / LDS use from hipcc's -Rpass-analysis=kernel-resource-usage remarks.

    python tools/resource_usage.py [ROLE] [--tus "22 10"]
    (ROLE 1 / 2: only that half of the pipelined kernels, like `make asm-role`; --tus: these units instead of the Makefile's TUS)

Compiles the kernel units of kernels_tu.hip for gfx950 (device only, no GPU needed) and prints one line per kernel."""
import argparse
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = f"{ROOT}/rrtplanner_amd/csrc"
ap = argparse.ArgumentParser()
ap.add_argument("role", nargs="?", choices=["1", "2"])
ap.add_argument("--tus", default=re.search(r"^TUS \?= (.*)$", open(f"{CSRC}/Makefile").read(), re.M).group(1))
args = ap.parse_args()


def remarks(tu):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
           f"-DRRT_TU={tu}", f"-I{ROOT}/include", f"-I{CSRC}", "--cuda-device-only", "-S", "-o", "/dev/null", f"{CSRC}/kernels_tu.hip",
           "-Rpass-analysis=kernel-resource-usage"]
    if args.role:
        cmd.insert(1, f"-DRRT_ONLY_ROLE={args.role}")
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stderr


with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
    out = "\n".join(pool.map(remarks, args.tus.split()))
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"remark: Function Name: (\S+)", line)
    if m:
        cur = {"name": subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()}
        rows.append(cur)
        continue
    m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
    if m and cur is not None:
        cur[m.group(1).strip()] = int(m.group(2))
print(f"{'kernel':78s} {'VGPR':>5s} {'AGPR':>5s} {'SGPR':>5s} {'vspill':>6s} {'sspill':>6s} {'scratch B/lane':>14s} {'LDS B':>7s}")
for r in rows:
    name = re.sub(r"rrtdev::|\(rrtdev::BatchView\)|void ", "", r["name"])
    print(f"{name:78s} {r.get('VGPRs', 0):5d} {r.get('AGPRs', 0):5d} {r.get('SGPRs', 0):5d} {r.get('VGPRs Spill', 0):6d} {r.get('SGPRs Spill', 0):6d} "
          f"{r.get('ScratchSize', 0):14d} {r.get('LDS Size', 0):7d}")
