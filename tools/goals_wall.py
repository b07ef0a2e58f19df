#!/usr/bin/env python3
"""Wall time of RRT.connect_goals: M goals against the tree of BASELINE config 2 (RRT*, 1024 x 1024 noise grid, n = 50 000,
r_rewire = 64), next to the same answers from a vectorised numpy restatement on the host.

    python tools/goals_wall.py [--goals 4096] [--host-goals 256] [--reps 15] [--out profiles/goals_wall.json]

device   warm-up calls, then the median of `reps` calls of planner.connect_goals(goals): upload, rrt_goals_kernel, read-back
host     per goal: the f64 cost array, a stable argsort, RRT.collisionfree (numpy) in that order until one is free -- the
         baseline, never the code under test; run on every (M / host-goals)-th goal and scaled to M
The two must agree on every goal the host looked at (vertex and cost, exactly).

The kernel goes straight to go2goal_phase.  A first stage in front of it (one pass for the cheapest vertex, one line of sight; the
answer if that line is free) was tried and lost; tools/archive/goals_first_stage.patch is that code.  When a library built with it
exists as rrtplanner_amd/librrt_hip_exp_stage1.so
    git apply tools/archive/goals_first_stage.patch && make -C rrtplanner_amd/csrc exp NAME=stage1 && git apply -R tools/archive/goals_first_stage.patch
the same device measurement runs once more on that library, in a child process of its own, and both times are written down."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

STAGE1 = os.path.join(ROOT, "rrtplanner_amd", "librrt_hip_exp_stage1.so")


def workload(m):
    from rrtplanner_amd import RRTStar
    from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pairs

    og = perlin_occupancygrid(1024, 1024, thresh=0.33, seed=1)
    xs, xg = random_connected_pairs(og, np.random.default_rng(7), 1)[0]
    free = np.argwhere(og == 0)
    goals = free[np.random.default_rng(11).integers(0, len(free), size=m)]
    p = RRTStar(og, 50000, 64, pbar=False, seed=0)
    t0 = time.perf_counter()
    T, gv = p.plan(np.asarray(xs), np.asarray(xg))
    p.plan_ms = (time.perf_counter() - t0) * 1e3  # (first call of the process: includes loading the library)
    return og, p, T, goals


def time_device(p, goals, warmup, reps):
    for _ in range(warmup):
        out = p.connect_goals(goals)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = p.connect_goals(goals)
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ts), min(ts)


def host_connect(og, points, vcosts, j, goal, collisionfree):
    d = points[:j] - goal
    cost = vcosts[:j] + np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64))
    for tried, k in enumerate(np.argsort(cost, kind="stable")):
        if collisionfree(og, points[k], goal):
            return int(k), float(cost[k]), tried + 1
    return -1, float("inf"), j


def lib_build_id(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--host-goals", type=int, default=256, help="goals the host baseline decides (spread over all of them); its time is scaled")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "goals_wall.json"))
    ap.add_argument("--device-only", action="store_true", help="print the device measurement as one JSON line and stop (the child run)")
    args = ap.parse_args()

    from rrtplanner_amd import _ffi
    from rrtplanner_amd import rrt as amd

    og, p, T, goals = workload(args.goals)
    (vertex, cost), med_ms, min_ms = time_device(p, goals, args.warmup, args.reps)
    dev = {"lib": os.path.basename(_ffi.LIB_PATH), "lib_sha256": lib_build_id(_ffi.LIB_PATH), "median_ms": med_ms, "min_ms": min_ms,
           "us_per_goal": med_ms * 1e3 / len(goals), "vertex_sum": int(vertex.astype(np.int64).sum()), "connected": int((vertex >= 0).sum())}
    if args.device_only:
        print(json.dumps(dev))
        return

    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    pick = np.arange(0, len(goals), max(1, len(goals) // args.host_goals))[:args.host_goals]
    t0 = time.perf_counter()
    host = [host_connect(og, points, vcosts, j, goals[g], amd.RRT.collisionfree) for g in pick]
    host_s = time.perf_counter() - t0
    for g, (hv, hc, _) in zip(pick, host):
        assert (vertex[g], cost[g]) == (hv, hc), (int(g), goals[g].tolist(), int(vertex[g]), float(cost[g]), hv, hc)

    out = {
        "what": "RRT.connect_goals wall time (upload + rrt_goals_kernel + read-back), median of %d calls after %d warm-up calls; tree of BASELINE "
                "config 2 (RRT*, 1024x1024 noise grid seed 1, n=50000, r_rewire=64, planner seed 0), goals drawn from the free cells with seed 11" % (args.reps, args.warmup),
        "goals": int(len(goals)), "tree_vertices": int(j), "goals_connected": dev["connected"],
        "build": {"lib_sha256": dev["lib_sha256"], "lib": dev["lib"]},
        "device": {"median_ms": med_ms, "min_ms": min_ms, "us_per_goal": dev["us_per_goal"]},
        "host_numpy": {"goals_decided": int(len(pick)), "seconds": host_s, "ms_per_goal": host_s * 1e3 / len(pick),
                       "scaled_to_all_goals_ms": host_s * 1e3 / len(pick) * len(goals), "agree": True,
                       "first_candidate_free": sum(h[2] == 1 for h in host), "lines_walked_mean": sum(h[2] for h in host) / len(host)},
        "first_plan_call_ms": p.plan_ms,
    }
    if os.path.exists(STAGE1) and os.path.abspath(_ffi.LIB_PATH) != STAGE1:
        env = dict(os.environ, RRT_HIP_LIB=STAGE1)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--device-only", "--goals", str(args.goals), "--warmup", str(args.warmup),
                            "--reps", str(args.reps)], env=env, capture_output=True, text=True, timeout=300)
        if r.returncode != 0:
            raise SystemExit("the run on %s failed:\n%s" % (STAGE1, r.stderr[-2000:]))
        alt = json.loads(r.stdout.strip().splitlines()[-1])
        assert (alt["vertex_sum"], alt["connected"]) == (dev["vertex_sum"], dev["connected"]), "the two builds disagree"
        out["first_stage"] = {"without_ms": med_ms, "with_ms": alt["median_ms"], "with_min_ms": alt["min_ms"], "with_lib_sha256": alt["lib_sha256"],
                              "note": "without: the product library (every goal goes straight to go2goal_phase); with: the same sources plus "
                                      "tools/archive/goals_first_stage.patch"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
