#!/usr/bin/env python3
"""Wall time of RRTStarDubins.keep_pose_tree next to planning again: the map changes under ONE Dubins tree of BASELINE config 5's
shape (Dubins-RRT*, 2048 x 2048 noise grid seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings -- the shape of
tools/poses_wall.py) and 4096 goal poses want their costs on the new map.

    python tools/pose_keep_wall.py [--goals 4096] [--reps 15] [--out profiles/pose_keep_wall.json]

Two new maps, each a case of its own: "frame", the next frame of the noise (perlin_occupancygrid(frames=2, seed=3): the tree is
planned on frame 0, the new map is frame 1), and "blocks", frame 0 with six square blocks stamped on it.  Per case two planners, timed
in the same run and alternated (every repetition runs each step once, in this order), after warm-up repetitions; host clocks around
calls that end in a device synchronise:
    keep_pose_tree        keep_pose_tree(new map): what set_og does on the host (free cells, upload) and the device call
    keep_pose_tree_call   the device call alone, again on the map that is already there (rrt_plan_keep_pose_tree: edge test, pointer
                          jumping, compaction + heading gather, two read-backs); its three stages from events on the stream
    poses_after_keep      connect_poses(goal poses) over the view
    keep_pose_tree_back   keep_pose_tree(first map): every repetition starts from the whole tree on its own map
    set_og_plan           the alternative: set_og(new map) + plan() on a second planner -- the yardstick, measured here, not a fixed number
    poses_after_plan      connect_poses(goal poses) over the new tree
The planner that replans draws a fresh sample stream every repetition, as a caller's would."""
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

from goals_wall import lib_build_id  # noqa: E402
from keep_tree_wall import stamped  # noqa: E402

CFG = dict(grid=2048, grid_seed=3, n=100000, r_rewire=64, rho=8.0, nh=64)  # bench.py CONFIGS[5], one query


def run_case(name, og, og2, xs, xg, poses, warmup, reps):
    from rrtplanner_amd.dubins import RRTStarDubins

    def planner():
        return RRTStarDubins(og, CFG["n"], CFG["r_rewire"], CFG["rho"], n_headings=CFG["nh"], pbar=False, seed=0)

    def plan(p):
        try:
            p.plan(xs, xg)
        except IndexError:  # (the plan's own goal pose unreachable: the tree is complete all the same)
            if p._tree_resident != "device":
                raise
        return p.last_stats["j"]

    keeper, replanner = planner(), planner()
    j = plan(keeper)
    plan(replanner)
    first = keeper.connect_poses(poses)
    out, stages = {}, []

    def set_og_plan():
        replanner.set_og(og2)
        return plan(replanner)

    def keep_call():
        alive = keeper.device_context().keep_pose_tree()
        stages.append(keeper.device_context().keep_tree_ms())
        return alive

    steps = {
        "keep_pose_tree": lambda: keeper.keep_pose_tree(og2),
        "keep_pose_tree_call": keep_call,
        "poses_after_keep": lambda: keeper.connect_poses(poses),
        "keep_pose_tree_back": lambda: keeper.keep_pose_tree(og),
        "set_og_plan": set_og_plan,
        "poses_after_plan": lambda: replanner.connect_poses(poses),
    }
    ts = {k: [] for k in steps}
    for r in range(warmup + reps):
        if r == warmup:
            stages.clear()
        for k, f in steps.items():
            t0 = time.perf_counter()
            out[k] = f()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
        replanner.set_og(og)  # (the next repetition's set_og(og2) uploads again; not timed)
    alive = out["keep_pose_tree"]
    assert np.array_equal(alive, out["keep_pose_tree_call"]) and out["keep_pose_tree_back"].all() and len(alive) == j
    again = keeper.connect_poses(poses)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])  # back on the first map: the first answers
    kept_v, kept_c, _ = out["poses_after_keep"]
    new_v, new_c, _ = out["poses_after_plan"]
    assert alive[kept_v[kept_v >= 0]].all()

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    return {
        "case": name, "tree_vertices": int(j), "vertices_cut": int((~alive).sum()), "cells_changed": int((og != og2).sum()),
        **{k: stat(k) for k in steps},
        "keep_pose_tree_stages_ms_median": {"edge_test": float(np.median(st[:, 0])), "pointer_jumping": float(np.median(st[:, 1])),
                                            "compaction_and_gather": float(np.median(st[:, 2]))},
        "keep_then_poses_ms": med["keep_pose_tree"] + med["poses_after_keep"],
        "plan_then_poses_ms": med["set_og_plan"] + med["poses_after_plan"],
        "keep_over_plan": med["keep_pose_tree"] / med["set_og_plan"],
        "poses_connected": {"first_map": int((first[0] >= 0).sum()), "after_keep": int((kept_v >= 0).sum()), "after_plan": int((new_v >= 0).sum())},
        "cost_mean": {"after_keep": float(np.mean(kept_c[kept_v >= 0])) if (kept_v >= 0).any() else None,
                      "after_plan": float(np.mean(new_c[new_v >= 0])) if (new_v >= 0).any() else None},
        "new_tree_vertices": int(out["set_og_plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_keep_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi
    from rrtplanner_amd.oggen import largest_free_component, perlin_occupancygrid

    frames = perlin_occupancygrid(CFG["grid"], CFG["grid"], thresh=0.33, frames=2, seed=CFG["grid_seed"])
    og = frames[0]
    # start and goal free and connected on both frames; the goal poses on cells that are free on both new maps
    both = np.argwhere(largest_free_component(frames[0] | frames[1]))
    rng = np.random.default_rng(7)
    a, b = both[rng.integers(0, len(both))], both[rng.integers(0, len(both))]
    xs, xg = np.array((a[0], a[1], 5)), np.array((b[0], b[1], 20))
    blocks = stamped(og, xs, count=6, side=48)
    free = np.argwhere((frames[0] | frames[1] | blocks) == 0)
    rng = np.random.default_rng(11)
    poses = np.column_stack([free[rng.integers(0, len(free), size=args.goals)], rng.integers(0, CFG["nh"], size=args.goals)])
    cases = [run_case("frame", og, frames[1], xs, xg, poses, args.warmup, args.reps),
             run_case("blocks", og, blocks, xs, xg, poses, args.warmup, args.reps)]
    res = {
        "what": "wall time of keeping a finished Dubins tree on a changed map against planning again, median of %d repetitions after %d "
                "warm-up repetitions, the steps alternated in one run; Dubins-RRT*, 2048x2048 noise grid (frame 0 of 2, seed 3), n=100000, "
                "r_rewire=64, rho=8, 64 headings, planner seed 0, %d goal poses on cells free on every map, drawn with seed 11; the edge test "
                "is the simple form: one edge per lane, one sweep round of 128 samples per edge" % (args.reps, args.warmup, len(poses)),
        "goals": int(len(poses)),
        "build": {"lib_sha256": lib_build_id(_ffi.LIB_PATH), "lib": os.path.basename(_ffi.LIB_PATH)},
        "cases": cases,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
