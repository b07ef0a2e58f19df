#!/usr/bin/env python3
"""Wall time of repairing a kept Dubins tree (keep_pose_tree + grow_poses) next to planning again: the map changes under ONE Dubins
tree of BASELINE config 5's shape (Dubins-RRT*, 2048 x 2048 noise grid seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings -- the
tree of tools/pose_keep_wall.py) and 4096 goal poses want their costs on the new map.

    python tools/pose_grow_wall.py [--goals 4096] [--reps 15] [--out profiles/pose_grow_wall.json]

The maps and goal poses are those of tools/pose_keep_wall.py: "frame", the next frame of the noise, and "blocks", frame 0 with six
square blocks stamped on it.  Per case two planners, timed in the same run and alternated (every repetition runs each step once, in
this order), after warm-up repetitions; host clocks around calls that end in a device synchronise:
    keep_pose_tree       keep_pose_tree(new map)
    grow_poses           grow_poses(m = the vertices keep_pose_tree cut): the draw of m cells and m headings, the seed kernels, the
                         expansion, go2goal; the seed's three stages from events on the stream (rrt_plan_grow_ms)
    poses_after_grow     connect_poses(goal poses) over the grown tree
    set_og_plan          the alternative: set_og(new map) + plan() on a second planner -- the yardstick, measured here
    poses_after_plan     connect_poses(goal poses) over the new tree
Before every repetition the first planner plans on the first map again (not timed): a grow replaces the tree it grows.
seed_over_plan is the seed's stages together over set_og_plan of the same run; repair_over_plan is keep_pose_tree + grow_poses over
set_og_plan, the claim the call stands on."""
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
from pose_keep_wall import CFG  # noqa: E402


def run_case(name, og, og2, xs, xg, poses, warmup, reps):
    from rrtplanner_amd.dubins import RRTStarDubins

    def planner():
        return RRTStarDubins(og, CFG["n"], CFG["r_rewire"], CFG["rho"], n_headings=CFG["nh"], pbar=False, seed=0)

    def plan_quietly(p):
        try:
            p.plan(xs, xg)
        except IndexError:  # (the plan's own goal pose unreachable: the tree is complete all the same)
            if p._tree_resident != "device":
                raise
        return p.last_stats["j"]

    keeper, replanner = planner(), planner()
    plan_quietly(replanner)
    out, stages, cut = {}, [], [0]

    def keep():
        alive = keeper.keep_pose_tree(og2)
        cut[0] = int((~alive).sum())
        return alive

    def grow():
        try:
            keeper.grow_poses(cut[0])
        except IndexError:
            if keeper._tree_resident != "device":
                raise
        stages.append(keeper.device_context().grow_ms())
        return keeper.last_stats["j"]

    def set_og_plan():
        replanner.set_og(og2)
        return plan_quietly(replanner)

    steps = {
        "keep_pose_tree": keep,
        "grow_poses": grow,
        "poses_after_grow": lambda: keeper.connect_poses(poses),
        "set_og_plan": set_og_plan,
        "poses_after_plan": lambda: replanner.connect_poses(poses),
    }
    ts = {k: [] for k in steps}
    for r in range(warmup + reps):
        if r == warmup:
            stages.clear()
        keeper.set_og(og)
        j = plan_quietly(keeper)  # (not timed: the tree the map changes under)
        for k, f in steps.items():
            t0 = time.perf_counter()
            out[k] = f()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
        replanner.set_og(og)
    alive = out["keep_pose_tree"]
    grown_v, grown_c, _ = out["poses_after_grow"]
    new_v, new_c, _ = out["poses_after_plan"]

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    seed_ms = float(np.median(st.sum(axis=1)))
    return {
        "case": name, "tree_vertices": int(j), "vertices_cut": int((~alive).sum()), "samples_grown": int(cut[0]),
        "vertices_after_keep": int(alive.sum()), "vertices_after_grow": int(out["grow_poses"]), "cells_changed": int((og != og2).sum()),
        **{k: stat(k) for k in steps},
        "seed_stages_ms_median": {"renumber_slots_and_headings": float(np.median(st[:, 0])), "bitmap": float(np.median(st[:, 1])),
                                  "cell_records": float(np.median(st[:, 2])), "together": seed_ms},
        "seed_over_plan": seed_ms / med["set_og_plan"],
        "repair_ms": med["keep_pose_tree"] + med["grow_poses"],
        "repair_over_plan": (med["keep_pose_tree"] + med["grow_poses"]) / med["set_og_plan"],
        "keep_grow_poses_ms": med["keep_pose_tree"] + med["grow_poses"] + med["poses_after_grow"],
        "plan_then_poses_ms": med["set_og_plan"] + med["poses_after_plan"],
        "poses_connected": {"after_grow": int((grown_v >= 0).sum()), "after_plan": int((new_v >= 0).sum())},
        "cost_mean": {"after_grow": float(np.mean(grown_c[grown_v >= 0])) if (grown_v >= 0).any() else None,
                      "after_plan": float(np.mean(new_c[new_v >= 0])) if (new_v >= 0).any() else None},
        "new_tree_vertices": int(out["set_og_plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_grow_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi
    from rrtplanner_amd.oggen import largest_free_component, perlin_occupancygrid

    # the maps, the poses and the goal poses of tools/pose_keep_wall.py
    frames = perlin_occupancygrid(CFG["grid"], CFG["grid"], thresh=0.33, frames=2, seed=CFG["grid_seed"])
    og = frames[0]
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
        "what": "wall time of keeping and growing a finished Dubins tree on a changed map against planning again, median of %d repetitions "
                "after %d warm-up repetitions, the steps alternated in one run; Dubins-RRT*, 2048x2048 noise grid (frame 0 of 2, seed 3), "
                "n=100000, r_rewire=64, rho=8, 64 headings, planner seed 0, %d goal poses on cells free on every map, drawn with seed 11"
                % (args.reps, args.warmup, len(poses)),
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
