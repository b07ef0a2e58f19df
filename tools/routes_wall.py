#!/usr/bin/env python3
"""Wall time of RRT.routes_to next to RRT.paths_to: routes to M goals over the tree of BASELINE config 2 (RRT*, 1024 x 1024 noise
grid, n = 50 000, r_rewire = 64) -- the workload of tools/goals_wall.py, same grid, tree and goals.

    python tools/routes_wall.py [--goals 4096] [--reps 15] [--out profiles/routes_wall.json]

Four steps, timed in the same run and alternated (every repetition runs each of them once, in this order), after warm-up calls of
each; host clocks around calls that end in a device synchronise and hand back finished numpy arrays:
    connect_goals             the decision alone (upload, rrt_goals_kernel, read-back)
    paths_to                  the baseline: connect_goals, then per goal a parent walk and a point list in Python
    routes_to(shortcut=False) the same routes from the device (goals kernel, depth, scan, fill, pack, read-back, one np.split)
    routes_to(shortcut=True)  ... with the line-of-sight shortcut pass and a second scan
routes_to(shortcut=False) must equal paths_to on every goal; the shortcut routes are checked for shape only (first and last
point, never more rows, never longer) -- tests/test_routes_gpu.py compares them with the host restatement."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from goals_wall import lib_build_id, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "routes_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi

    og, p, T, goals = workload(args.goals)
    steps = {
        "connect_goals": lambda: p.connect_goals(goals),
        "paths_to": lambda: p.paths_to(T, goals),
        "routes_to": lambda: p.routes_to(goals, shortcut=False),
        "routes_to_shortcut": lambda: p.routes_to(goals, shortcut=True),
    }
    out, ts = {}, {k: [] for k in steps}
    for _ in range(args.warmup):
        for k, f in steps.items():
            out[k] = f()
    for _ in range(args.reps):
        for k, f in steps.items():
            t0 = time.perf_counter()
            out[k] = f()
            ts[k].append((time.perf_counter() - t0) * 1e3)

    vertex, cost = out["connect_goals"]
    paths = out["paths_to"]
    raw, raw_len = out["routes_to"]
    cut, cut_len = out["routes_to_shortcut"]
    ok = vertex >= 0
    pos = ok & (cost > 0)  # (a goal on the start itself has cost 0 and no ratio)
    assert len(paths) == len(raw) == len(cut) == len(goals)
    for g in range(len(goals)):
        if not ok[g]:
            assert paths[g] is None and raw[g] is None and cut[g] is None and raw_len[g] == cut_len[g] == np.inf, g
            continue
        assert np.array_equal(paths[g], raw[g]), g
        assert np.array_equal(cut[g][0], raw[g][0]) and np.array_equal(cut[g][-1], raw[g][-1]) and len(cut[g]) <= len(raw[g]), g
    assert np.all(cut_len[ok] <= raw_len[ok] * (1 + 1e-9)) and np.all(cut_len[ok] <= cost[ok] * (1 + 1e-9))
    rows_raw = int(sum(len(r) for r in raw if r is not None))
    rows_cut = int(sum(len(r) for r in cut if r is not None))

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k]), "us_per_goal": statistics.median(ts[k]) * 1e3 / len(goals)}

    res = {
        "what": "wall time of routes to many goals, median of %d calls after %d warm-up calls, the four steps alternated in one run; tree of BASELINE "
                "config 2 (RRT*, 1024x1024 noise grid seed 1, n=50000, r_rewire=64, planner seed 0), goals drawn from the free cells with seed 11"
                % (args.reps, args.warmup),
        "goals": int(len(goals)), "tree_vertices": int(p.last_stats["j"]), "goals_connected": int(ok.sum()),
        "build": {"lib_sha256": lib_build_id(_ffi.LIB_PATH), "lib": os.path.basename(_ffi.LIB_PATH)},
        "connect_goals": stat("connect_goals"),
        "paths_to": stat("paths_to"),
        "routes_to": stat("routes_to"),
        "routes_to_shortcut": stat("routes_to_shortcut"),
        "beyond_connect_goals_ms": {k: statistics.median(ts[k]) - statistics.median(ts["connect_goals"]) for k in ("paths_to", "routes_to", "routes_to_shortcut")},
        "rows": {"raw": rows_raw, "shortcut": rows_cut, "raw_per_route_mean": rows_raw / int(ok.sum()), "shortcut_per_route_mean": rows_cut / int(ok.sum()),
                 "raw_per_route_max": int(max(len(r) for r in raw if r is not None)), "routes_shortened": int(sum(len(c) < len(r) for c, r in zip(cut, raw) if r is not None))},
        "length_over_cost_mean": {"raw": float(np.mean(raw_len[pos] / cost[pos])), "shortcut": float(np.mean(cut_len[pos] / cost[pos])),
                                  "shortcut_min": float(np.min(cut_len[pos] / cost[pos]))},
        "routes_to_equals_paths_to": True,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
