#!/usr/bin/env python3
"""Wall time of one RRT* plan() on a 4096 x 4096 map: RRTStar(og, 50 000, 64, pbar=False).plan(), median of 5 after 2 warm-ups.

    python tools/large_grid_wall.py [--n 50000] [--r 64] [--grid 4096] [--runs 5] [--warmup 2]

Prints one JSON line with the route the plan took (planner.last_route where the class has it: "kernel-large" on the large-grid
kernel, "host" on the host-driven loop; a checkout from before the large-grid kernel has no such attribute and runs the host
loop).  The map is built from rectangles: two walls with a gap each, start and goal in opposite corners."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rrtplanner_amd import RRTStar  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=50000)
ap.add_argument("--r", type=float, default=64.0)
ap.add_argument("--grid", type=int, default=4096)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()

W = H = a.grid
og = np.zeros((W, H), dtype=np.int64)
og[W // 3:W // 3 + 6, :H * 3 // 4] = 1
og[2 * W // 3:2 * W // 3 + 4, H // 4:] = 1
xs, xg = np.array((3, 3)), np.array((W - 4, H - 4))
p = RRTStar(og, a.n, a.r, pbar=False, seed=0)
times, gv, nodes = [], None, None
for k in range(a.warmup + a.runs):
    t0 = time.perf_counter()
    T, gv = p.plan(xs, xg)
    dt = time.perf_counter() - t0
    nodes = p.last_stats["j"] if getattr(p, "last_stats", None) else T.number_of_nodes()
    if k >= a.warmup:
        times.append(dt)
try:
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
except Exception:
    commit = None
print(json.dumps(dict(tool="large_grid_wall", grid=[W, H], n=a.n, r_rewire=a.r, route=getattr(p, "last_route", "host (no last_route: before the large-grid kernel)"),
                      wall_s_median=statistics.median(times), wall_s_all=times, goal_vertex=int(gv), vertices=int(nodes), commit=commit)))
