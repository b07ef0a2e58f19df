#!/usr/bin/env python3
"""Wall time of routes_to_poses(shortcut=True) next to the plain routes_to_poses of the same run: routes to M goal poses over ONE Dubins
tree of BASELINE config 5's shape (Dubins-RRT*, 2048 x 2048 noise grid seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings), the
tree and the goal poses of tools/pose_routes_wall.py.

    python tools/pose_shortcuts_wall.py [--goals 4096] [--reps 15] [--out profiles/pose_shortcuts_wall.json]

One child process (under `timeout -k 10`) plans the tree once and then alternates the four calls, `reps` rounds of
    routes_to_poses(poses)                routes_to_poses(poses, shortcut=True)
    routes_to_poses(poses, points=True)   routes_to_poses(poses, points=True, shortcut=True)
and reports the median, the spread, the stage times of the library (rrt_plan_pose_routes_ms, rrt_plan_pose_shortcuts_ms), the rows
and points with and without shortcuts, how many routes were shortened and the mean of length / cost over the connected poses.  The
yardstick of the shortcut call is the plain call of the same run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.poses_wall import lib_build_id, spread, workload  # noqa: E402  (the same tree and the same goal poses)

CALLS = {"routes_to_poses": dict(), "routes_to_poses_shortcut": dict(shortcut=True), "routes_to_poses_points": dict(points=True),
         "routes_to_poses_points_shortcut": dict(points=True, shortcut=True)}
PLAIN_STAGES = ["decision (rrt_pose_goals_kernel)", "depth + scan", "rows + legs + lengths (+ point scan)", "points"]
CUT_STAGES = ["decision (rrt_pose_goals_kernel)", "depth + scan", "rows + shortcuts + scan + pack", "legs + lengths (+ point scan)", "points"]


def child(args):
    from rrtplanner_amd import _ffi

    p, xs, xg, poses = workload(args.goals)
    m = len(poses)
    try:
        p.plan(np.array(xs), np.array(xg))
    except IndexError:
        pass  # (the planner's own goal is unreachable: the tree is resident all the same)
    ctx = p._device()
    for _ in range(args.warmup):
        for kw in CALLS.values():
            p.routes_to_poses(poses, **kw)
    ts = {k: [] for k in CALLS}
    ms = {k: [] for k in CALLS}
    got = {}
    for _ in range(args.reps):
        for k, kw in CALLS.items():
            t0 = time.perf_counter()
            got[k] = p.routes_to_poses(poses, **kw)
            ts[k].append((time.perf_counter() - t0) * 1e3)
            ms[k].append(ctx.pose_shortcuts_ms() if kw.get("shortcut") else ctx.pose_routes_ms())
    vertex, cost, _ = p.connect_poses(poses)
    on = vertex >= 0
    raw, cut = got["routes_to_poses_points"], got["routes_to_poses_points_shortcut"]
    assert np.array_equal(raw[1][on].view(np.int64), cost[on].view(np.int64)), "plain length != cost"
    assert np.all(cut[1][on] <= cost[on] * (1 + 1e-9)) and np.all(np.isinf(cut[1][~on])), "a shortcut route is longer than the raw one"
    nrows = lambda routes: sum(len(r) for r in routes if r is not None)
    shortened = sum(1 for a, b in zip(raw[0], cut[0]) if a is not None and len(b) < len(a))
    ratio = cut[1][on & (cost > 0)] / cost[on & (cost > 0)]
    out = {
        "lib": os.path.basename(_ffi.LIB_PATH), "lib_sha256": lib_build_id(_ffi.LIB_PATH), "tree_vertices": int(p.last_stats["j"]), "goals": m,
        "goals_connected": int(on.sum()), "rows_raw": nrows(raw[0]), "rows_kept": nrows(cut[0]), "routes_shortened": shortened,
        "longest_raw_route_rows": max(len(r) for r in raw[0] if r is not None),
        "length_over_cost": {"mean": float(ratio.mean()), "median": float(np.median(ratio)), "min": float(ratio.min()), "max": float(ratio.max())},
        "points_raw": sum(len(q) for q in raw[2] if q is not None), "points_kept": sum(len(q) for q in cut[2] if q is not None),
        "call_ms": ts,
        "stage_ms": {k: [statistics.median(x[s] for x in v) for s in range(len(v[0]))] for k, v in ms.items()},
    }
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--limit", type=int, default=420, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_shortcuts_wall.json"))
    ap.add_argument("--child", action="store_true", help="(internal) the measurement itself")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--goals", str(args.goals), "--warmup", str(args.warmup),
           "--reps", str(args.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the device after a child that failed, faulted or ran out of time
        raise SystemExit("the child ended with status %d:\n%s" % (r.returncode, r.stderr[-3000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = {
        "what": "wall time of routes_to_poses with and without shortcut=True, with and without points=True, for %d goal poses against one Dubins-RRT* tree of "
                "BASELINE config 5's shape (2048x2048 noise grid seed 3, n=100000, r_rewire=64, rho=8, 64 headings, planner seed 0; goal poses from the free "
                "cells with uniform headings, seed 11), the four calls alternated in one process, %d rounds after %d warm-up rounds; length_over_cost over "
                "the connected poses with cost > 0" % (res["goals"], args.reps, args.warmup),
    }
    out.update({k: res[k] for k in ("goals", "tree_vertices", "goals_connected", "rows_raw", "rows_kept", "routes_shortened", "longest_raw_route_rows",
                                    "length_over_cost", "points_raw", "points_kept", "lib", "lib_sha256")})
    for k, v in res["call_ms"].items():
        out[k] = spread(v)
        out[k]["stage_ms"] = dict(zip(CUT_STAGES if k.endswith("shortcut") else PLAIN_STAGES, res["stage_ms"][k]))
    for k, base in (("routes_to_poses_shortcut", "routes_to_poses"), ("routes_to_poses_points_shortcut", "routes_to_poses_points")):
        out[k]["times_the_plain_call"] = out[k]["median_ms"] / out[base]["median_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
