#!/usr/bin/env python3
"""Wall time and connected costs of re-rooting a finished Dubins tree at a pose the vehicle has reached (moving.reroot_poses) next to
planning again from that pose, on the workload of tools/poses_wall.py: ONE tree of BASELINE config 5's shape (2048 x 2048 noise grid
seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings, about 92 000 vertices) and its 4096 goal poses.

    python tools/pose_reroot_wall.py [--goals 4096] [--reps 15] [--out profiles/pose_reroot_wall.json]

Per case two planners, timed in the same run and alternated (every repetition runs each step once, in this order), after warm-up
repetitions; host clocks around calls that end in a device synchronise:
    reroot_poses          moving.reroot_poses(v, 64): the root-first input, the buckets, the start costs, the rounds, the parents, the
                          order, the costs, the seed, the goal decision; its seven stages and the seed's three from events on the stream
                          (rrt_plan_reroot_poses_ms), its counters (last_relax)
    poses_after_reroot    connect_poses(goal poses) over the re-rooted tree
    set_og_plan           the alternative: set_og + plan() from v's pose on a second planner -- the yardstick, measured here
    poses_after_plan      connect_poses(goal poses) over the new tree
Before every repetition the first planner plans from the first start again with the same draws (not timed): a re-root replaces the tree
it re-roots, and the same tree gives the same v every time.
Cases: v three legs along the route to the goal pose, and v at the end of that route; and `three_legs_kept`, after a map change: the
map gets six blocks of 48 cells (tools/pose_keep_wall.py), the tree is kept on it (keep_pose_tree, not timed), v is the deepest alive
vertex of the first three legs, and reroot_poses(v, 64, m) spends as many samples as the keep cut; the yardstick plans on the new map.
reroot_over_plan is the seven re-root stages together over set_og_plan of the same run.
--variants name=library[,...]: the same cases again in a child process each on an experiment build of the library (make exp), recorded
under `variants` next to the baseline."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402

from keep_tree_wall import stamped  # noqa: E402
from poses_wall import CFG, lib_build_id, workload  # noqa: E402

STAGES = ("front_and_buckets", "start_costs", "rounds", "parents", "alive_and_depth", "order", "costs", "seed_renumber_slots_and_headings", "seed_bitmap",
          "seed_cell_records")


def run_case(name, og, xs, xg, poses, legs, kept, warmup, reps):
    """legs: how many legs along the route to xg the vehicle has driven (None: all of them); kept: the map changes first"""
    from rrtplanner_amd import moving
    from rrtplanner_amd.dubins import RRTStarDubins

    def planner():
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
    og2 = stamped(og, xs[:2], count=6, side=48) if kept else og
    out, stages, counters, info = {}, [], [], {"m": 0}

    def reroot():
        j = quietly(keeper, lambda: moving.reroot_poses(keeper, info["v"], CFG["r_rewire"], info["m"]))
        stages.append(moving.reroot_poses_ms(keeper.device_context()))
        counters.append(dict(keeper.last_relax))
        return j

    def set_og_plan():
        replanner.set_og(og2)
        return quietly(replanner, lambda: replanner.plan(info["start"], xg))

    steps = {
        "reroot_poses": reroot,
        "poses_after_reroot": lambda: keeper.connect_poses(poses),
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
        j = quietly(keeper, lambda: keeper.plan(xs, xg))  # (not timed: the tree the vehicle drives on)
        vertex, cost, length, offsets, xyh, ids = keeper.device_context().pose_routes(np.asarray([xg]))
        route = ids[offsets[0]:offsets[1]][:-1]  # the vertices root .. the goal's vertex (the last row is the goal pose)
        assert len(route) > 1, "the goal pose of this workload is connected"
        d = len(route) - 1 if legs is None else min(legs, len(route) - 1)
        if kept:
            alive = keeper.keep_pose_tree(og2)  # (not timed: the map change itself, tools/pose_keep_wall.py measures it)
            info["m"] = int((~alive).sum())
            while not alive[route[d]]:
                d -= 1  # (the root is alive: no block is stamped on the start)
        info["v"], info["start"], info["d"] = int(route[d]), np.array(xyh[offsets[0] + d]), d
        for k, f in steps.items():
            t0 = time.perf_counter()
            out[k] = f()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)

    def stat(k):
        return {"median_ms": statistics.median(ts[k]), "min_ms": min(ts[k]), "max_ms": max(ts[k])}

    med = {k: statistics.median(ts[k]) for k in ts}
    st = np.array(stages, dtype=np.float64)
    reroot_ms = float(np.median(st[:, :7].sum(axis=1)))
    v = {k: out["poses_after_" + k][0] for k in ("reroot", "plan")}
    c = {k: out["poses_after_" + k][1] for k in ("reroot", "plan")}
    both = (v["reroot"] >= 0) & (v["plan"] >= 0)
    reached = int(np.median([x["reached"] for x in counters]))
    return {
        "case": name, "tree_vertices": int(j), "vertex": info["v"], "depth_d": info["d"], "start_pose": [int(x) for x in info["start"]],
        "vertices_reached": reached, "vertices_cut": int(j) - reached, "vertices_cut_by_the_keep_and_samples_m": info["m"],
        "vertices_after_reroot_and_grow": int(out["reroot_poses"]),
        **{k: stat(k) for k in steps},
        "stages_ms_median": {**{s: float(np.median(st[:, k])) for k, s in enumerate(STAGES)}, "reroot_together": reroot_ms,
                             "seed_together": float(np.median(st[:, 7:].sum(axis=1)))},
        "counters_median": {k: float(np.median([x[k] for x in counters])) for k in counters[0]},
        "counters_min_max": {k: [int(min(x[k] for x in counters)), int(max(x[k] for x in counters))] for k in counters[0]},
        "reroot_over_plan": reroot_ms / med["set_og_plan"],
        "reroot_call_over_plan": med["reroot_poses"] / med["set_og_plan"],
        "reroot_then_poses_ms": med["reroot_poses"] + med["poses_after_reroot"],
        "plan_then_poses_ms": med["set_og_plan"] + med["poses_after_plan"],
        "poses_connected": {k: int((x >= 0).sum()) for k, x in v.items()},
        "cost_mean_over_poses_both_connect": {k: float(np.mean(x[both])) for k, x in c.items()},
        "cost_rerooted_over_new_plan": float(np.mean(c["reroot"][both]) / np.mean(c["plan"][both])),
        "new_tree_vertices": int(out["set_og_plan"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--cases", default="three_legs,end_of_route,three_legs_kept")
    ap.add_argument("--variants", default="", help="name=library[,name=library...]: experiment builds measured in child processes")
    ap.add_argument("--child", action="store_true", help="print the cases as one JSON line and write no file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_reroot_wall.json"))
    args = ap.parse_args()

    from rrtplanner_amd import _ffi

    p, xs, xg, poses = workload(args.goals)
    og = p.og
    xs, xg = np.array(xs), np.array(xg)
    cases = []
    for name in args.cases.split(","):
        cases.append(run_case(name, og, xs, xg, poses, None if name == "end_of_route" else 3, name.endswith("_kept"), args.warmup, args.reps))
        print(json.dumps(cases[-1]), file=sys.stderr, flush=True)
    build = {"lib_sha256": lib_build_id(_ffi.LIB_PATH), "lib": os.path.basename(_ffi.LIB_PATH)}
    if args.child:
        print(json.dumps({"build": build, "cases": cases}))
        return
    variants = []
    for spec in filter(None, args.variants.split(",")):
        vname, lib = spec.split("=")
        cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "--goals", str(args.goals), "--warmup", str(args.warmup),
               "--reps", str(args.reps), "--cases", args.cases]
        r = subprocess.run(cmd, env=dict(os.environ, RRT_HIP_LIB=os.path.abspath(lib)), capture_output=True, text=True)
        if r.returncode != 0:  # nothing more is started on the device after a child that failed, faulted or ran out of time
            raise SystemExit("variant %s ended with status %d:\n%s" % (vname, r.returncode, r.stderr[-3000:]))
        got = json.loads(r.stdout.strip().splitlines()[-1])
        keep = ("case", "reroot_poses", "set_og_plan", "stages_ms_median", "counters_median", "counters_min_max", "reroot_over_plan", "reroot_call_over_plan")
        variants.append({"variant": vname, "build": got["build"], "cases": [{k: c[k] for k in keep} for c in got["cases"]]})
    res = {
        "what": "wall time and connected costs of re-rooting a finished Dubins tree at a pose of its route to the goal pose against planning again "
                "from that pose, median of %d repetitions after %d warm-up repetitions, the steps alternated in one run; 2048x2048 noise grid seed "
                "3, n=100000, r_rewire=64 (also reroot_poses' radius), rho=8, 64 headings, planner seed 0, the %d goal poses of tools/poses_wall.py"
                % (args.reps, args.warmup, len(poses)),
        "goals": int(len(poses)),
        "build": build,
        "cases": cases,
        "variants": variants,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
