#!/usr/bin/env python3
"""Wall time of RRT.keep_tree next to planning again: the map changes under the tree of BASELINE config 2's size (RRT*, 1024 x 1024
noise grid, n = 50 000, r_rewire = 64, about 48 000 vertices) and 4096 goals want routes on the new map.

    python tools/keep_tree_wall.py [--goals 4096] [--reps 15] [--out profiles/keep_tree_wall.json]

Two new maps, each a case of its own: "frame", the next frame of the noise (perlin_occupancygrid(frames=2, seed=1): the tree is
planned on frame 0, the new map is frame 1), and "blocks", frame 0 with a few square blocks stamped on it.  Per case two planners,
timed in the same run and alternated (every repetition runs each step once, in this order), after warm-up repetitions; host clocks
around calls that end in a device synchronise:
    keep_tree            RRT.keep_tree(new map): what set_og does on the host (free cells, upload) and the device call
    keep_tree_call       the device call alone, again on the map that is already there (rrt_plan_keep_tree: edge test, pointer
                         jumping, compaction, two read-backs); its three stages from events on the stream
    routes_after_keep    routes_to(goals) over the view
    keep_tree_back       keep_tree(first map): every repetition starts from the whole tree on its own map
    set_og_plan          the alternative: set_og(new map) + plan() on a second planner -- the yardstick, measured here, not a fixed number
    routes_after_plan    routes_to(goals) over the new tree
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


def stamped(og, xs, count=6, side=24, seed=21):
    """`count` square blocks of `side` cells on free ground, none on the start"""
    out = og.copy()
    rng = np.random.default_rng(seed)
    free = np.argwhere(og == 0)
    done = 0
    while done < count:
        x, y = free[rng.integers(0, len(free))]
        if abs(int(x) - int(xs[0])) <= side and abs(int(y) - int(xs[1])) <= side:
            continue
        out[x:x + side, y:y + side] = 1
        done += 1
    return out


def run_case(name, og, og2, xs, xg, goals, warmup, reps):
    from rrtplanner_amd import RRTStar

    keeper = RRTStar(og, 50000, 64, pbar=False, seed=0)
    replanner = RRTStar(og, 50000, 64, pbar=False, seed=0)
    keeper.plan(xs, xg)
    replanner.plan(xs, xg)
    j = keeper.last_stats["j"]
    first = keeper.routes_to(goals)
    out, stages = {}, []

    def set_og_plan():
        replanner.set_og(og2)
        try:
            replanner.plan(xs, xg)
        except IndexError:  # (the plan's own goal walled off on the new map: the tree is complete all the same)
            if replanner._tree_resident != "device":
                raise
        return replanner.last_stats["j"]

    def keep_call():
        alive = keeper.device_context().keep_tree()
        stages.append(keeper.device_context().keep_tree_ms())
        return alive

    steps = {
        "keep_tree": lambda: keeper.keep_tree(og2),
        "keep_tree_call": keep_call,
        "routes_after_keep": lambda: keeper.routes_to(goals),
        "keep_tree_back": lambda: keeper.keep_tree(og),
        "set_og_plan": set_og_plan,
        "routes_after_plan": lambda: replanner.routes_to(goals),
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
    alive = out["keep_tree"]
    assert np.array_equal(alive, out["keep_tree_call"]) and out["keep_tree_back"].all() and len(alive) == j
    again = keeper.routes_to(goals)
    assert np.array_equal(first[1], again[1])  # back on the first map: the first lengths
    kept_routes, kept_len = out["routes_after_keep"]
    new_routes, new_len = out["routes_after_plan"]

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    return {
        "case": name, "tree_vertices": int(j), "vertices_cut": int((~alive).sum()), "cells_changed": int((og != og2).sum()),
        **{k: stat(k) for k in steps},
        "keep_tree_stages_ms_median": {"edge_test": float(np.median(st[:, 0])), "pointer_jumping": float(np.median(st[:, 1])),
                                       "compaction": float(np.median(st[:, 2]))},
        "keep_then_routes_ms": med["keep_tree"] + med["routes_after_keep"],
        "plan_then_routes_ms": med["set_og_plan"] + med["routes_after_plan"],
        "goals_connected": {"first_map": int(np.isfinite(first[1]).sum()), "after_keep": int(np.isfinite(kept_len).sum()),
                            "after_plan": int(np.isfinite(new_len).sum())},
        "route_length_mean": {"after_keep": float(np.mean(kept_len[np.isfinite(kept_len)])) if np.isfinite(kept_len).any() else None,
                              "after_plan": float(np.mean(new_len[np.isfinite(new_len)])) if np.isfinite(new_len).any() else None},
        "new_tree_vertices": int(out["set_og_plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_tree_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi
    from rrtplanner_amd.oggen import largest_free_component, perlin_occupancygrid

    frames = perlin_occupancygrid(1024, 1024, thresh=0.33, frames=2, seed=1)
    og = frames[0]
    # start and goal free and connected on both frames; the goals of the routes free on both new maps
    both = np.argwhere(largest_free_component(frames[0] | frames[1]))
    rng = np.random.default_rng(7)
    xs, xg = both[rng.integers(0, len(both))], both[rng.integers(0, len(both))]
    blocks = stamped(og, xs)
    free = np.argwhere((frames[0] | frames[1] | blocks) == 0)
    goals = free[np.random.default_rng(11).integers(0, len(free), size=args.goals)]
    cases = [run_case("frame", og, frames[1], xs, xg, goals, args.warmup, args.reps),
             run_case("blocks", og, blocks, xs, xg, goals, args.warmup, args.reps)]
    res = {
        "what": "wall time of keeping a finished tree on a changed map against planning again, median of %d repetitions after %d warm-up "
                "repetitions, the steps alternated in one run; RRT*, 1024x1024 noise grid (frame 0 of 2, seed 1), n=50000, r_rewire=64, planner "
                "seed 0, %d goals free on every map, drawn with seed 11" % (args.reps, args.warmup, len(goals)),
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
