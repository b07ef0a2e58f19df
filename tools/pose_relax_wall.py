#!/usr/bin/env python3
"""Wall time and connected costs of relaxing a finished Dubins tree (RRTDubins / RRTStarDubins .relax_poses) on the workload of
tools/poses_wall.py: ONE tree of BASELINE config 5's shape (2048 x 2048 noise grid seed 3, n = 100 000, r_rewire = 64, rho = 8,
64 headings) and its 4096 goal poses.

    python tools/pose_relax_wall.py [--goals 4096] [--reps 15] [--passes star,dubins,kept_grown] [--out profiles/pose_relax_wall.json]

Per pass two planners, timed in the same run and alternated (every repetition runs each step once, in this order), after warm-up
repetitions; host clocks around calls that end in a device synchronise:
    poses_before         connect_poses(goal poses) over the tree as it stands: the unrelaxed tree of the same run
    relax_poses          relax_poses(r = 64): the buckets, the rounds, the parents, the order, the costs, the seed, the goal decision; its
                         six stages and the seed's three from events on the stream (rrt_plan_relax_poses_ms), its counters (last_relax)
    poses_after_relax    connect_poses(goal poses) over the relaxed tree
    set_og_plan          the alternative: set_og + plan() on a second planner -- the yardstick, measured here
    poses_after_plan     connect_poses(goal poses) over the new tree
Before every repetition the first planner builds its tree again with the same draws (not timed).
Passes: `star`, the tree RRTStarDubins.plan() left; `dubins`, the tree of RRTDubins (nearest-vertex parents; r = 64 passed); `kept_grown`,
the RRTStarDubins tree kept on the map with six blocks stamped on it (tools/pose_keep_wall.py) and grown by as many samples as were cut.
relax_over_plan is the six relax stages together over set_og_plan of the same run; cost_relaxed_over_before the mean connected cost over
the relaxed tree over that of the unrelaxed tree, over the goal poses both connect (the same ones: the vertices do not move)."""
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

from keep_tree_wall import stamped  # noqa: E402
from poses_wall import CFG, lib_build_id, workload  # noqa: E402

STAGES = ("buckets", "rounds", "parents", "alive_and_depth", "order", "costs", "seed_renumber_slots_and_headings", "seed_bitmap", "seed_cell_records")


def run_pass(name, og, xs, xg, poses, warmup, reps):
    from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

    def planner():
        if name == "dubins":
            return RRTDubins(og, CFG["n"], CFG["rho"], n_headings=CFG["nh"], pbar=False, seed=0)
        return RRTStarDubins(og, CFG["n"], CFG["r_rewire"], CFG["rho"], n_headings=CFG["nh"], pbar=False, seed=0)

    def quietly(p, call):
        try:
            call()
        except IndexError:  # (the plan's own goal pose unreachable: the tree is complete all the same)
            if p._tree_resident != "device":
                raise
        return int(p._grow_j0)  # the vertices of the tree the call left

    keeper, replanner = planner(), planner()
    state0 = keeper.rand_gen.bit_generator.state
    og2 = stamped(og, xs[:2], count=6, side=48) if name == "kept_grown" else og
    out, stages, counters, info = {}, [], [], {}

    def relax():
        j = quietly(keeper, lambda: keeper.relax_poses(CFG["r_rewire"]))
        stages.append(keeper.device_context().relax_poses_ms())
        counters.append(dict(keeper.last_relax))
        return j

    def set_og_plan():
        replanner.set_og(og2)
        return quietly(replanner, lambda: replanner.plan(xs, xg))

    steps = {
        "poses_before": lambda: keeper.connect_poses(poses),
        "relax_poses": relax,
        "poses_after_relax": lambda: keeper.connect_poses(poses),
        "set_og_plan": set_og_plan,
        "poses_after_plan": lambda: replanner.connect_poses(poses),
    }
    ts = {k: [] for k in steps}
    for r in range(warmup + reps):
        if r == warmup:
            stages.clear()
            counters.clear()
        keeper.set_og(og)
        keeper.rand_gen.bit_generator.state = state0
        j = quietly(keeper, lambda: keeper.plan(xs, xg))  # (not timed: the tree the call relaxes)
        if name == "kept_grown":
            alive = keeper.keep_pose_tree(og2)
            info["cut"] = int((~alive).sum())
            j = quietly(keeper, lambda: keeper.grow_poses(info["cut"]))
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
    v = {k: out["poses_" + k][0] for k in ("before", "after_relax", "after_plan")}
    c = {k: out["poses_" + k][1] for k in ("before", "after_relax", "after_plan")}
    both = (v["before"] >= 0) & (v["after_relax"] >= 0)
    all3 = both & (v["after_plan"] >= 0)
    return {
        "pass": name, "planner": type(keeper).__name__, "tree_vertices": int(j), "vertices_relaxed": int(out["relax_poses"]),
        **({"vertices_cut_and_samples_grown": info["cut"]} if name == "kept_grown" else {}),
        **{k: stat(k) for k in steps},
        "stages_ms_median": {**{s: float(np.median(st[:, k])) for k, s in enumerate(STAGES)}, "relax_together": relax_ms,
                             "seed_together": float(np.median(st[:, 6:].sum(axis=1)))},
        "counters_median": {k: float(np.median([x[k] for x in counters])) for k in counters[0]},
        "counters_min_max": {k: [int(min(x[k] for x in counters)), int(max(x[k] for x in counters))] for k in counters[0]},
        "vertices_cheaper": int(np.median([x["fell"] for x in counters])),
        "relax_over_plan": relax_ms / med["set_og_plan"],
        "relax_call_over_plan": med["relax_poses"] / med["set_og_plan"],
        "poses_connected": {k: int((x >= 0).sum()) for k, x in v.items()},
        "cost_mean_over_poses_both_connect": {"before": float(np.mean(c["before"][both])), "after_relax": float(np.mean(c["after_relax"][both]))},
        "cost_relaxed_over_before": float(np.mean(c["after_relax"][both]) / np.mean(c["before"][both])),
        "cost_mean_over_poses_all_three_connect": {k: float(np.mean(x[all3])) for k, x in c.items()},
        "new_tree_vertices": int(out["set_og_plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--passes", default="star,dubins,kept_grown")
    ap.add_argument("--variants-that-lost", default=None, help="a JSON file of variants tried against this build, copied into the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_relax_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi

    p, xs, xg, poses = workload(args.goals)
    og = p.og
    xs, xg = np.array(xs), np.array(xg)
    passes = []
    for name in args.passes.split(","):
        passes.append(run_pass(name, og, xs, xg, poses, args.warmup, args.reps))
        print(json.dumps(passes[-1]), flush=True)
    res = {
        "what": "wall time and connected costs of relaxing a finished Dubins tree over its own poses against planning again, median of %d "
                "repetitions after %d warm-up repetitions, the steps alternated in one run; 2048x2048 noise grid seed 3, n=100000, r_rewire=64 "
                "(also relax_poses' radius), rho=8, 64 headings, planner seed 0, the %d goal poses of tools/poses_wall.py"
                % (args.reps, args.warmup, len(poses)),
        "goals": int(len(poses)),
        "build": {"lib_sha256": lib_build_id(_ffi.LIB_PATH), "lib": os.path.basename(_ffi.LIB_PATH)},
        "passes": passes,
        "variants_that_lost": json.load(open(args.variants_that_lost)) if args.variants_that_lost else [],
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
