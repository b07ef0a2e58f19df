#!/usr/bin/env python3
"""Wall time of connect_poses: M goal poses against ONE Dubins tree of BASELINE config 5's shape (Dubins-RRT*, 2048 x 2048 noise
grid seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings), in the kernel's two forms, next to what a user did before the call
existed: one fresh plan() per goal pose.

    python tools/poses_wall.py [--goals 4096] [--reps 15] [--blocks 3] [--plans 4] [--out profiles/poses_wall.json]

bounded      the product library: the vertices sorted by the chord bound, one word per vertex that survives it (rrt_pose_goals.h)
exhaustive   the same sources built with -DRRT_POSES_EXHAUSTIVE, where tools/archive/poses_exhaustive.patch is applied:
                 git apply tools/archive/poses_exhaustive.patch && make -C rrtplanner_amd/csrc exp EXP=-DRRT_POSES_EXHAUSTIVE NAME=poses_a \\
                     && git apply -R tools/archive/poses_exhaustive.patch
             goals_body with go2goal_phase<true>: three words per vertex before any sweep.  Left out when that library is absent.
fresh plan   `plans` plan() calls of the same planner towards different goal poses, scaled to M.

The two forms alternate: `blocks` child processes each, bounded / exhaustive / bounded / ..., every child a fresh process that plans
the tree, warms up and times reps / blocks calls; the medians and the spread (min, max, inter-quartile range) are over all timed
calls of a form.  Every child runs under `timeout -k 10` of its own and the run stops at the first one that fails.  The two forms
must give the same answers.  The decision that profiles/poses_wall.json records: the bounded form ships if its median beats the
exhaustive one's by more than the larger of the two spreads (max - min)."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

EXHAUSTIVE = os.path.join(ROOT, "rrtplanner_amd", "librrt_hip_exp_poses_a.so")
CFG = dict(grid=2048, grid_seed=3, n=100000, r_rewire=64, rho=8.0, nh=64)  # bench.py CONFIGS[5], one query


def workload(m):
    from rrtplanner_amd.dubins import RRTStarDubins
    from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pairs

    og = perlin_occupancygrid(CFG["grid"], CFG["grid"], thresh=0.33, seed=CFG["grid_seed"])
    xs, xg = random_connected_pairs(og, np.random.default_rng(7), 1)[0]
    free = np.argwhere(og == 0)
    rng = np.random.default_rng(11)
    poses = np.column_stack([free[rng.integers(0, len(free), size=m)], rng.integers(0, CFG["nh"], size=m)])
    p = RRTStarDubins(og, CFG["n"], CFG["r_rewire"], CFG["rho"], n_headings=CFG["nh"], pbar=False, seed=0)
    return p, (int(xs[0]), int(xs[1]), 5), (int(xg[0]), int(xg[1]), 20), poses


def lib_build_id(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def child(args):
    """one fresh process; one JSON line.  calls: the tree on a batch of this tool's own (its counters are a batch call), then
    connect_poses timed.  plans: fresh plan() calls of the planner towards other goal poses."""
    from rrtplanner_amd import _ffi, hostprep

    p, xs, xg, poses = workload(args.goals)
    out = {"lib": os.path.basename(_ffi.LIB_PATH), "lib_sha256": lib_build_id(_ffi.LIB_PATH)}
    if args.child == "plans":
        ts = []
        for k in range(args.plans + 1):  # (the first one loads the library and allocates: not counted)
            p.rand_gen = np.random.default_rng(0)  # the same sample stream: the same tree, another goal pose
            t0 = time.perf_counter()
            try:
                p.plan(np.array(xs), poses[k])
            except IndexError:
                pass  # (that goal pose is unreachable: the answer a user gets for it, at the same price)
            ts.append((time.perf_counter() - t0) * 1e3)
        out.update(plan_ms=ts[1:], first_plan_call_ms=ts[0], tree_vertices=int(p.last_stats["j"]))
        print(json.dumps(out))
        return
    n, nh = CFG["n"], CFG["nh"]
    rng = np.random.default_rng(0)  # the planner's stream: n free cells, then n headings
    samples = hostprep.draw_free_samples(rng, p.free, n)
    heads = rng.integers(0, nh, size=n)
    ctx = _ffi.Context(0)
    ctx.set_grid(hostprep.og_nonzero(p.og))
    b = _ffi.Batch(ctx, 1, n, dubins=True)
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR, n, xs, xg, samples, r2_rewire=hostprep.radius_threshold(CFG["r_rewire"]), headings=heads,
                              rho=CFG["rho"], nh=nh)
    b.set_query(0, q)
    b.launch()
    b.sync()
    res = b.get_result(0, arrays=False)
    for _ in range(args.warmup):
        vertex, cost = b.connect_poses(0, poses)
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        vertex, cost = b.connect_poses(0, poses)
        ts.append((time.perf_counter() - t0) * 1e3)
    words, sweeps = b.connect_poses_counts()
    out.update(call_ms=ts, words=words, sweeps=sweeps, connected=int((vertex >= 0).sum()), tree_vertices=int(res.j), plan_kernel_ms=b.elapsed_ms(),
               vertex_sum=int(vertex.astype(np.int64).sum()), cost_sha256=hashlib.sha256(cost.tobytes()).hexdigest()[:16])
    b.close()
    ctx.close()
    print(json.dumps(out))


def compiled(extra=()):
    """registers, LDS, scratch and occupancy of rrt_pose_goals_kernel from hipcc's kernel-resource-usage remarks (device code only)"""
    import re

    csrc = os.path.join(ROOT, "rrtplanner_amd", "csrc")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
           *extra, "-DRRT_TU=9", "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "--cuda-device-only", "-S", "-o", "/dev/null",
           os.path.join(csrc, "kernels_tu.hip"), "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    return {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", err)}


def spread(ts):
    qs = statistics.quantiles(ts, n=4) if len(ts) >= 4 else [min(ts), statistics.median(ts), max(ts)]
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "iqr_ms": qs[2] - qs[0], "calls": len(ts)}


def run_child(mode, lib, args, limit):
    env = dict(os.environ)
    if lib:
        env["RRT_HIP_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--goals", str(args.goals), "--warmup",
           str(args.warmup), "--reps", str(max(1, args.reps // args.blocks)), "--plans", str(args.plans)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the device after a child that failed, faulted or ran out of time
        raise SystemExit("child %s on %s ended with status %d:\n%s" % (mode, lib or "the product library", r.returncode, r.stderr[-3000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print("# %s on %s: %s" % (mode, res["lib"], ["%.1f" % t for t in res.get("call_ms", res.get("plan_ms"))]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--blocks", type=int, default=3, help="child processes per form; the forms alternate")
    ap.add_argument("--plans", type=int, default=4, help="fresh plan() calls that are timed and scaled to --goals")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poses_wall.json"))
    ap.add_argument("--child", choices=["calls", "plans"], help="(internal) the measurement of one child process")
    args = ap.parse_args()
    if args.child:
        return child(args)

    forms = [("bounded", None)] + ([("exhaustive", EXHAUSTIVE)] if os.path.exists(EXHAUSTIVE) else [])
    runs = {name: [] for name, _ in forms}
    for _ in range(args.blocks):
        for name, lib in forms:
            runs[name].append(run_child("calls", lib, args, args.limit))
    plans = run_child("plans", None, args, args.limit)

    out = {
        "what": "connect_poses wall time (upload + rrt_pose_goals_kernel + read-back) of %d goal poses against one Dubins-RRT* tree of BASELINE "
                "config 5's shape (2048x2048 noise grid seed 3, n=100000, r_rewire=64, rho=8, 64 headings, planner seed 0); goal poses drawn "
                "from the free cells with uniform headings, seed 11; %d child processes per form, alternating, %d warm-up calls each"
                % (args.goals, args.blocks, args.warmup),
        "goals": args.goals,
    }
    for name, _ in forms:
        rs = runs[name]
        same = {(r["vertex_sum"], r["connected"], r["cost_sha256"], r["tree_vertices"]) for r in rs}
        assert len(same) == 1, "the children of the %s form disagree" % name
        ts = [t for r in rs for t in r["call_ms"]]
        out[name] = dict(spread(ts), us_per_goal=statistics.median(ts) * 1e3 / args.goals, lib=rs[0]["lib"], lib_sha256=rs[0]["lib_sha256"],
                         words_per_goal=rs[0]["words"] / args.goals, sweeps_per_goal=rs[0]["sweeps"] / args.goals,
                         per_child_median_ms=[statistics.median(r["call_ms"]) for r in rs])
    if "exhaustive" in out:
        out["exhaustive"]["counts_note"] = "that build counts the three passes' words (3 per vertex) and no sweeps: go2goal_phase is not instrumented"
    out["bounded"]["compiled"] = compiled()
    if "exhaustive" in out and "RRT_POSES_EXHAUSTIVE" in open(os.path.join(ROOT, "rrtplanner_amd", "csrc", "rrt_pose_goals.h")).read():
        out["exhaustive"]["compiled"] = compiled(["-DRRT_POSES_EXHAUSTIVE"])
    b = runs["bounded"][0]
    out.update(tree_vertices=b["tree_vertices"], goals_connected=b["connected"])
    pm = statistics.median(plans["plan_ms"])
    out["fresh_plan_per_goal"] = {"plans_timed": len(plans["plan_ms"]), "plan_ms": plans["plan_ms"], "median_ms": pm, "scaled_to_all_goals_ms": pm * args.goals}
    if "exhaustive" in out:
        a, bb = out["exhaustive"], out["bounded"]
        e = runs["exhaustive"][0]
        assert (e["vertex_sum"], e["connected"], e["cost_sha256"]) == (b["vertex_sum"], b["connected"], b["cost_sha256"]), "the two forms disagree"
        sp = max(a["max_ms"] - a["min_ms"], bb["max_ms"] - bb["min_ms"])
        ships = "bounded" if a["median_ms"] - bb["median_ms"] > sp else "exhaustive"
        out["decision"] = {"rule": "the bounded form ships if its median beats the exhaustive one's by more than the spread of the repetitions "
                                   "(the larger max - min of the two forms); otherwise the exhaustive one, which is less code",
                           "spread_ms": sp, "median_gain_ms": a["median_ms"] - bb["median_ms"], "ships": ships, "answers_agree": True}
    else:
        out["decision"] = {"ships": "not decided here: %s is absent, only the product library was timed" % os.path.basename(EXHAUSTIVE)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
