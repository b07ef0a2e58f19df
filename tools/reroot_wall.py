#!/usr/bin/env python3
"""Wall time of re-rooting a finished tree at a vertex the vehicle has reached (RRT.reroot) next to planning again from that point:
the tree of BASELINE config 2's size (RRT*, 1024 x 1024 noise grid, n = 50 000, r_rewire = 64, about 48 000 vertices), the map and
the goals of tools/grow_wall.py, and 4096 goals that want routes from the new start.

    python tools/reroot_wall.py [--goals 4096] [--reps 15] [--out profiles/reroot_wall.json]

Per case two planners, timed in the same run and alternated (every repetition runs each step once, in this order), after warm-up
repetitions; host clocks around calls that end in a device synchronise:
    reroot                RRT.reroot(v, m): the draw of m samples, the re-root stages, the seed, the expansion of m samples, go2goal;
                          the five re-root stages and the seed's three from events on the stream (rrt_plan_reroot_ms)
    routes_after_reroot   routes_to(goals) over the re-rooted tree
    plan                  the alternative: plan(points[v], xgoal) on a second planner -- the yardstick, measured here
    routes_after_plan     routes_to(goals) over the new tree
Before every repetition the first planner plans from the first start again with the same draws (not timed): a reroot replaces the
tree it re-roots, and the same tree gives the same v, depth and cut every time.
Cases: v three legs along the route to the goal and v at the end of that route, each with m = 0; and, where a reversed edge was
blocked and cut vertices, the same v with m = the vertices that were cut.
reroot_over_plan is the re-root stages together over `plan` of the same run."""
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

STAGES = ("path", "reversed_edges", "alive_and_depth", "order", "costs", "seed_renumber_and_slots", "seed_bitmap", "seed_cell_records")


def run_case(name, og, xs, xg, goals, legs, m_of, warmup, reps):
    """legs: how many legs along the route to xg the vehicle has driven (None: all of them); m_of(cut) -> the samples to spend"""
    from rrtplanner_amd import RRTStar

    keeper = RRTStar(og, 50000, 64, pbar=False, seed=0)
    replanner = RRTStar(og, 50000, 64, pbar=False, seed=0)
    state0 = keeper.rand_gen.bit_generator.state
    out, stages, info = {}, [], {}

    def plan_quietly(p, start):
        try:
            p.plan(start, xg)
        except IndexError:  # (the plan's own goal not reached: the tree is complete all the same)
            if p._tree_resident != "device":
                raise
        return p.last_stats["j"]

    def reroot():
        try:
            keeper.reroot(info["v"], info["m"])
        except IndexError:
            if keeper._tree_resident != "device":
                raise
        stages.append(keeper.device_context().reroot_ms())
        info["alive"] = len(keeper.last_grow_ids)
        return keeper.last_stats["j"]

    steps = {
        "reroot": reroot,
        "routes_after_reroot": lambda: keeper.routes_to(goals),
        "plan": lambda: plan_quietly(replanner, info["start"]),
        "routes_after_plan": lambda: replanner.routes_to(goals),
    }
    ts = {k: [] for k in steps}
    info["m"] = 0
    for r in range(warmup + reps):
        if r == warmup:
            stages.clear()
        keeper.rand_gen.bit_generator.state = state0
        j = plan_quietly(keeper, xs)  # (not timed: the tree the vehicle drives on)
        vertex, cost, length, offsets, xy, ids = keeper.device_context().routes(np.asarray([xg]))
        route = ids[offsets[0]:offsets[1]][:-1]  # the vertices root .. the goal's vertex (the last row is the goal)
        assert len(route) > 1, "the goal of this workload is connected"
        d = len(route) - 1 if legs is None else min(legs, len(route) - 1)
        info["v"], info["start"], info["d"] = int(route[d]), xy[offsets[0] + d].copy(), d
        for k, f in steps.items():
            t0 = time.perf_counter()
            out[k] = f()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
        if r == 0:
            info["cut"] = int(j) - info["alive"]
            info["m"] = int(m_of(info["cut"]))
            if m_of(1) and not info["cut"]:
                return None  # nothing was cut: there is no gap to repair
    re_routes, re_len = out["routes_after_reroot"]
    new_routes, new_len = out["routes_after_plan"]

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    reroot_ms = float(np.median(st[:, :5].sum(axis=1)))
    return {
        "case": name, "tree_vertices": int(j), "vertex": info["v"], "depth_d": info["d"], "samples_m": info["m"],
        "vertices_alive_after_reroot": info["alive"], "vertices_cut": info["cut"], "vertices_after_reroot_and_grow": int(out["reroot"]),
        **{k: stat(k) for k in steps},
        "stages_ms_median": {**{s: float(np.median(st[:, k])) for k, s in enumerate(STAGES)}, "reroot_together": reroot_ms,
                             "seed_together": float(np.median(st[:, 5:].sum(axis=1)))},
        "reroot_over_plan": reroot_ms / med["plan"],
        "reroot_then_routes_ms": med["reroot"] + med["routes_after_reroot"],
        "plan_then_routes_ms": med["plan"] + med["routes_after_plan"],
        "goals_connected": {"after_reroot": int(np.isfinite(re_len).sum()), "after_plan": int(np.isfinite(new_len).sum())},
        "route_length_mean": {"after_reroot": float(np.mean(re_len[np.isfinite(re_len)])) if np.isfinite(re_len).any() else None,
                              "after_plan": float(np.mean(new_len[np.isfinite(new_len)])) if np.isfinite(new_len).any() else None},
        "new_tree_vertices": int(out["plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reroot_wall.json"))
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
    cases = []
    for name, legs in (("three_legs", 3), ("end_of_route", None)):
        cases.append(run_case(name, og, xs, xg, goals, legs, lambda cut: 0, args.warmup, args.reps))
        cases.append(run_case(name + "_repaired", og, xs, xg, goals, legs, lambda cut: cut, args.warmup, args.reps))
    res = {
        "what": "wall time of re-rooting a finished tree at a vertex of its route to the goal against planning again from that vertex, median of "
                "%d repetitions after %d warm-up repetitions, the steps alternated in one run; RRT*, 1024x1024 noise grid (frame 0 of 2, seed 1), "
                "n=50000, r_rewire=64, planner seed 0, %d goals free on every map of tools/grow_wall.py, drawn with seed 11; a case whose "
                "reversed edges cut nothing has no _repaired twin" % (args.reps, args.warmup, len(goals)),
        "goals": int(len(goals)),
        "build": {"lib_sha256": lib_build_id(_ffi.LIB_PATH), "lib": os.path.basename(_ffi.LIB_PATH)},
        "cases": [c for c in cases if c is not None],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
