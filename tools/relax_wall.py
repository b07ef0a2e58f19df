#!/usr/bin/env python3
"""Wall time and route lengths of relaxing a finished tree (RRT.relax) on the workload of tools/reroot_wall.py: the tree of BASELINE
config 2's size (RRT*, 1024 x 1024 noise grid, n = 50 000, r_rewire = 64, about 48 000 vertices) and 4096 goals that want routes.

    python tools/relax_wall.py [--goals 4096] [--reps 15] [--out profiles/relax_wall.json]

Per case two planners, timed in the same run and alternated (every repetition runs each step once, in this order), after warm-up
repetitions; host clocks around calls that end in a device synchronise:
    reroot               RRT.reroot(v) on the first planner (cases with a vertex v)
    routes_after_reroot  routes_to(goals) over the re-rooted tree: what relax starts from
    relax                RRT.relax() behind it: the buckets, the rounds, the parents, the later re-root stages, the seed, go2goal; its
                         six stages and the seed's three from events on the stream (rrt_plan_relax_ms), its counters (last_relax)
    routes_after_relax   routes_to(goals) over the relaxed tree
    plan                 the alternative: plan(points[v], xgoal) on a second planner -- the yardstick, measured here
    routes_after_plan    routes_to(goals) over the new tree
Before every repetition the first planner plans from the first start again with the same draws (not timed).
Cases: v three legs along the route to the goal, v at the end of that route, and `fresh`: no reroot, relax() on the tree plan() left
(its plan is the first planner's own, and routes_after_reroot are the routes over that tree).
relax_over_plan is the six relax stages together over `plan` of the same run; route_length_relaxed_over_planned the mean route length
over the relaxed tree over that of the tree planned from v, over the goals both connect."""
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

STAGES = ("buckets", "rounds", "parents", "alive_and_depth", "order", "costs", "seed_renumber_and_slots", "seed_bitmap", "seed_cell_records")


def run_case(name, og, xs, xg, goals, legs, warmup, reps):
    """legs: how many legs along the route to xg the vehicle has driven (None: all of them; "fresh": none, and no reroot)"""
    from rrtplanner_amd import RRTStar

    keeper = RRTStar(og, 50000, 64, pbar=False, seed=0)
    replanner = RRTStar(og, 50000, 64, pbar=False, seed=0)
    state0 = keeper.rand_gen.bit_generator.state
    fresh = legs == "fresh"
    out, stages, counters, info = {}, [], [], {}

    def quietly(p, call):
        try:
            call()
        except IndexError:  # (the plan's own goal not reached: the tree is complete all the same)
            if p._tree_resident != "device":
                raise
        return p.last_stats["j"]

    def relax():
        j = quietly(keeper, keeper.relax)
        stages.append(keeper.device_context().relax_ms())
        counters.append(dict(keeper.last_relax))
        return j

    steps = {
        "reroot": (lambda: None) if fresh else (lambda: quietly(keeper, lambda: keeper.reroot(info["v"]))),
        "routes_after_reroot": lambda: keeper.routes_to(goals),
        "relax": relax,
        "routes_after_relax": lambda: keeper.routes_to(goals),
        "plan": lambda: quietly(replanner, lambda: replanner.plan(info["start"], xg)),
        "routes_after_plan": lambda: replanner.routes_to(goals),
    }
    ts = {k: [] for k in steps}
    for r in range(warmup + reps):
        if r == warmup:
            stages.clear()
            counters.clear()
        keeper.rand_gen.bit_generator.state = state0
        j = quietly(keeper, lambda: keeper.plan(xs, xg))  # (not timed: the tree the vehicle drives on)
        vertex, cost, length, offsets, xy, ids = keeper.device_context().routes(np.asarray([xg]))
        route = ids[offsets[0]:offsets[1]][:-1]  # the vertices root .. the goal's vertex (the last row is the goal)
        assert len(route) > 1, "the goal of this workload is connected"
        d = 0 if fresh else len(route) - 1 if legs is None else min(legs, len(route) - 1)
        info["v"], info["start"], info["d"] = int(route[d]), xy[offsets[0] + d].copy(), d
        for k, f in steps.items():
            t0 = time.perf_counter()
            out[k] = f()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    relax_ms = float(np.median(st[:, :6].sum(axis=1)))
    lens = {k: out["routes_after_" + k][1] for k in ("reroot", "relax", "plan")}
    both = np.isfinite(lens["relax"]) & np.isfinite(lens["plan"]) & np.isfinite(lens["reroot"])

    def mean(a, mask=None):
        a = a[np.isfinite(a) if mask is None else mask]
        return float(np.mean(a)) if len(a) else None

    return {
        "case": name, "tree_vertices": int(j), "vertex": info["v"], "depth_d": info["d"], "vertices_relaxed": int(out["relax"]),
        **{k: stat(k) for k in steps if not (fresh and k == "reroot")},
        "stages_ms_median": {**{s: float(np.median(st[:, k])) for k, s in enumerate(STAGES)}, "relax_together": relax_ms,
                             "seed_together": float(np.median(st[:, 6:].sum(axis=1)))},
        "counters_median": {k: float(np.median([c[k] for c in counters])) for k in counters[0]},
        "counters_min_max": {k: [int(min(c[k] for c in counters)), int(max(c[k] for c in counters))] for k in counters[0]},
        "relax_over_plan": relax_ms / med["plan"],
        "reroot_relax_then_routes_ms": med["reroot"] * (not fresh) + med["relax"] + med["routes_after_relax"],
        "plan_then_routes_ms": med["plan"] + med["routes_after_plan"],
        "goals_connected": {k: int(np.isfinite(v).sum()) for k, v in lens.items()},
        "route_length_mean": {k: mean(v) for k, v in lens.items()},
        "route_length_mean_over_goals_all_connect": {k: mean(v, both) for k, v in lens.items()},
        "route_length_relaxed_over_planned": mean(lens["relax"], both) / mean(lens["plan"], both),
        "route_length_relaxed_over_before": mean(lens["relax"], both) / mean(lens["reroot"], both),
        "new_tree_vertices": int(out["plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="three_legs,end_of_route,fresh")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_wall.json"))
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
    legs = {"three_legs": 3, "end_of_route": None, "fresh": "fresh"}
    cases = [run_case(name, og, xs, xg, goals, legs[name], args.warmup, args.reps) for name in args.cases.split(",")]
    res = {
        "what": "wall time and route lengths of relaxing a finished tree (behind a re-root at a vertex of its route to the goal, or as plan() "
                "left it) against planning again from that vertex, median of %d repetitions after %d warm-up repetitions, the steps alternated "
                "in one run; RRT*, 1024x1024 noise grid (frame 0 of 2, seed 1), n=50000, r_rewire=64 (also relax's radius), planner seed 0, %d "
                "goals free on every map of tools/grow_wall.py, drawn with seed 11" % (args.reps, args.warmup, len(goals)),
        "goals": int(len(goals)),
        "build": {"lib_sha256": lib_build_id(_ffi.LIB_PATH), "lib": os.path.basename(_ffi.LIB_PATH)},
        "cases": cases,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
