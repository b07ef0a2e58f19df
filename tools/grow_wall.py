#!/usr/bin/env python3
"""Wall time of repairing a kept tree (RRT.keep_tree + RRT.grow) next to planning again: the map changes under the tree of BASELINE
config 2's size (RRT*, 1024 x 1024 noise grid, n = 50 000, r_rewire = 64, about 48 000 vertices) and 4096 goals want routes on the
new map.

    python tools/grow_wall.py [--goals 4096] [--reps 15] [--out profiles/grow_wall.json]

The maps and goals are those of tools/keep_tree_wall.py: "frame", the next frame of the noise, and "blocks", frame 0 with a few
square blocks stamped on it.  Per case two planners, timed in the same run and alternated (every repetition runs each step once, in
this order), after warm-up repetitions; host clocks around calls that end in a device synchronise:
    keep_tree            RRT.keep_tree(new map)
    grow                 RRT.grow(m = the vertices keep_tree cut): the draw of m samples, the seed kernels, the expansion, go2goal;
                         the seed's three stages from events on the stream (rrt_plan_grow_ms)
    routes_after_grow    routes_to(goals) over the grown tree
    set_og_plan          the alternative: set_og(new map) + plan() on a second planner -- the yardstick, measured here
    routes_after_plan    routes_to(goals) over the new tree
Before every repetition the first planner plans on the first map again (not timed): a grow replaces the tree it grows.
seed_over_plan is the seed's stages together over set_og_plan of the same run: the seed has to be a fraction of a plan for the
feature to have a point."""
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


def run_case(name, og, og2, xs, xg, goals, warmup, reps):
    from rrtplanner_amd import RRTStar

    keeper = RRTStar(og, 50000, 64, pbar=False, seed=0)
    replanner = RRTStar(og, 50000, 64, pbar=False, seed=0)
    replanner.plan(xs, xg)
    out, stages, cut = {}, [], [0]

    def plan_quietly(p):
        try:
            p.plan(xs, xg)
        except IndexError:  # (the plan's own goal walled off on the new map: the tree is complete all the same)
            if p._tree_resident != "device":
                raise
        return p.last_stats["j"]

    def keep():
        alive = keeper.keep_tree(og2)
        cut[0] = int((~alive).sum())
        return alive

    def grow():
        try:
            keeper.grow(cut[0])
        except IndexError:
            if keeper._tree_resident != "device":
                raise
        stages.append(keeper.device_context().grow_ms())
        return keeper.last_stats["j"]

    def set_og_plan():
        replanner.set_og(og2)
        return plan_quietly(replanner)

    steps = {
        "keep_tree": keep,
        "grow": grow,
        "routes_after_grow": lambda: keeper.routes_to(goals),
        "set_og_plan": set_og_plan,
        "routes_after_plan": lambda: replanner.routes_to(goals),
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
    alive = out["keep_tree"]
    grown_routes, grown_len = out["routes_after_grow"]
    new_routes, new_len = out["routes_after_plan"]

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    seed_ms = float(np.median(st.sum(axis=1)))
    return {
        "case": name, "tree_vertices": int(j), "vertices_cut": int((~alive).sum()), "samples_grown": int(cut[0]),
        "vertices_after_keep": int(alive.sum()), "vertices_after_grow": int(out["grow"]), "cells_changed": int((og != og2).sum()),
        **{k: stat(k) for k in steps},
        "seed_stages_ms_median": {"renumber_and_slots": float(np.median(st[:, 0])), "bitmap": float(np.median(st[:, 1])),
                                  "cell_records": float(np.median(st[:, 2])), "together": seed_ms},
        "seed_over_plan": seed_ms / med["set_og_plan"],
        "keep_grow_routes_ms": med["keep_tree"] + med["grow"] + med["routes_after_grow"],
        "plan_then_routes_ms": med["set_og_plan"] + med["routes_after_plan"],
        "goals_connected": {"after_grow": int(np.isfinite(grown_len).sum()), "after_plan": int(np.isfinite(new_len).sum())},
        "route_length_mean": {"after_grow": float(np.mean(grown_len[np.isfinite(grown_len)])) if np.isfinite(grown_len).any() else None,
                              "after_plan": float(np.mean(new_len[np.isfinite(new_len)])) if np.isfinite(new_len).any() else None},
        "new_tree_vertices": int(out["set_og_plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grow_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi
    from rrtplanner_amd.oggen import largest_free_component, perlin_occupancygrid

    frames = perlin_occupancygrid(1024, 1024, thresh=0.33, frames=2, seed=1)
    og = frames[0]
    both = np.argwhere(largest_free_component(frames[0] | frames[1]))
    rng = np.random.default_rng(7)
    xs, xg = both[rng.integers(0, len(both))], both[rng.integers(0, len(both))]
    blocks = stamped(og, xs)
    free = np.argwhere((frames[0] | frames[1] | blocks) == 0)
    goals = free[np.random.default_rng(11).integers(0, len(free), size=args.goals)]
    cases = [run_case("frame", og, frames[1], xs, xg, goals, args.warmup, args.reps),
             run_case("blocks", og, blocks, xs, xg, goals, args.warmup, args.reps)]
    res = {
        "what": "wall time of keeping and growing a finished tree on a changed map against planning again, median of %d repetitions after %d "
                "warm-up repetitions, the steps alternated in one run; RRT*, 1024x1024 noise grid (frame 0 of 2, seed 1), n=50000, r_rewire=64, "
                "planner seed 0, %d goals free on every map, drawn with seed 11" % (args.reps, args.warmup, len(goals)),
        "goals": int(len(goals)),
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
