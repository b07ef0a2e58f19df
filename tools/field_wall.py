#!/usr/bin/env python3
"""Wall time of field.cost_field over the whole grid next to the only other way to the same arrays: RRT.connect_goals over every free
cell in chunks of GOALS_MAX.  The tree of BASELINE config 2 (RRT*, 1024 x 1024 noise grid, n = 50 000, r_rewire = 64), as
tools/goals_wall.py builds it.

    python tools/field_wall.py [--reps 15] [--warmup 2] [--out profiles/field_wall.json]

The two are timed in turns in one run, `reps` calls each after `warmup` calls each, and their results compared for equality (vertices
and the bits of the costs; the blocked cells of the goals' side are -1 / inf by construction).  Written down: both medians, minima and
maxima, the stage times and the four counters of the last field, the mean candidates walked per free cell, the ratio of the medians,
and the one condition -- the field's slowest repetition is below connect_goals' fastest."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

GOALS_MAX = 1 << 20  # goals of one connect_goals call (rrt_kernel_abi.h)


def workload():
    from rrtplanner_amd import RRTStar
    from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pairs

    og = perlin_occupancygrid(1024, 1024, thresh=0.33, seed=1)
    xs, xg = random_connected_pairs(og, np.random.default_rng(7), 1)[0]
    p = RRTStar(og, 50000, 64, pbar=False, seed=0)
    T, gv = p.plan(np.asarray(xs), np.asarray(xg))
    return og, p


def by_goals(p, og, free):
    """the field's arrays from connect_goals: every free cell a goal, in chunks of GOALS_MAX"""
    vertex = np.full(og.shape, -1, dtype=np.int32)
    cost = np.full(og.shape, np.inf, dtype=np.float64)
    for lo in range(0, len(free), GOALS_MAX):
        part = free[lo:lo + GOALS_MAX]
        v, c = p.connect_goals(part)
        vertex[part[:, 0], part[:, 1]] = v
        cost[part[:, 0], part[:, 1]] = c
    return vertex, cost


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return out, (time.perf_counter() - t0) * 1e3


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "field_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi, field

    og, p = workload()
    free = np.argwhere(og == 0)
    ctx = p.device_context()
    for _ in range(args.warmup):
        field.cost_field(p)
        by_goals(p, og, free)
    t_field, t_goals, stages = [], [], []
    for _ in range(args.reps):
        f, ms = timed(lambda: field.cost_field(p))
        t_field.append(ms)
        stages.append(field.cost_field_ms(ctx))
        stats = field.cost_field_stats(ctx)
        g, ms = timed(lambda: by_goals(p, og, free))
        t_goals.append(ms)
        assert np.array_equal(f[0], g[0]) and np.array_equal(f[1].view(np.int64), g[1].view(np.int64)), "the field and connect_goals disagree"
    with open(_ffi.LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()[:16]
    fs, gs = spread(t_field), spread(t_goals)
    out = {
        "what": "field.cost_field of the whole grid (buckets + rrt_field_kernel + read-back) next to RRT.connect_goals over every free cell in "
                "chunks of GOALS_MAX, timed in turns, %d calls each after %d warm-up calls each; tree of BASELINE config 2 (RRT*, 1024x1024 noise "
                "grid seed 1, n=50000, r_rewire=64, planner seed 0)" % (args.reps, args.warmup),
        "build": {"lib": os.path.basename(_ffi.LIB_PATH), "lib_sha256": sha},
        "grid": list(og.shape), "free_cells": int(len(free)), "tree_vertices": int(p.last_stats["j"]), "cells_connected": int((f[0] >= 0).sum()),
        "equal": True,
        "cost_field": dict(fs, stage_ms_median=dict(zip(("buckets", "decide", "remap", "read_back"), (statistics.median(s[k] for s in stages) for k in range(4)))),
                           counters=stats, candidates_walked_per_cell=stats["los"] / max(stats["cells"], 1),
                           buckets_visited_per_cell=stats["buckets"] / max(stats["cells"], 1), vertices_priced_per_cell=stats["priced"] / max(stats["cells"], 1)),
        "connect_goals": dict(gs, chunks=(len(free) + GOALS_MAX - 1) // GOALS_MAX, us_per_goal=gs["median_ms"] * 1e3 / max(len(free), 1)),
        "ratio_of_medians": gs["median_ms"] / fs["median_ms"],
        "field_slowest_below_goals_fastest": bool(fs["max_ms"] < gs["min_ms"]),
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
