#!/usr/bin/env python3
"""Wall time of routes_to_poses: routes to M goal poses, and the vehicle's path along them, over ONE Dubins tree of BASELINE config 5's
shape (Dubins-RRT*, 2048 x 2048 noise grid seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings), next to the connect_poses call
they ride on and to what a user did before the call existed: paths_to_poses and poses_polyline on the host.

    python tools/pose_routes_wall.py [--goals 4096] [--reps 15] [--host 256] [--out profiles/pose_routes_wall.json]

One child process (under `timeout -k 10`) plans the tree once and then alternates the three device calls, `reps` rounds of
    connect_poses(poses)   routes_to_poses(poses)   routes_to_poses(poses, points=True)
and reports the median, the spread and the stage times of the library (rrt_plan_pose_routes_ms).  The host route -- paths_to_poses,
then poses_polyline per route -- is timed once on the first `host` poses and scaled to M, as tools/goals_wall.py did.

The host polyline (numpy, libm) is compared with the device points of the same legs: point k of a leg against the libm point at arc
length 0.5 k, within 1e-8.  A leg on which two Dubins words have one length (mirror images) may be driven along the other word by
either arithmetic; such legs show up as `legs_beyond_tol` and are listed, they are no error (tests/test_pose_routes_cpu.py checks
the points against the oracle's cells leg by leg)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tools.poses_wall import CFG, lib_build_id, spread, workload  # noqa: E402  (the same tree and the same goal poses)

TOL = 1e-8


def child(args):
    from rrtplanner_amd import _ffi
    from rrtplanner_amd.dubins import dubins_polyline, dubins_shortest

    p, xs, xg, poses = workload(args.goals)
    m = len(poses)
    try:
        T, gv = p.plan(np.array(xs), np.array(xg))
    except IndexError:
        raise SystemExit("the planner's own goal is unreachable: paths_to_poses needs the tree plan() returns")
    ctx = p._device()
    for _ in range(args.warmup):
        p.connect_poses(poses)
        p.routes_to_poses(poses, points=True)
    ts = {"connect_poses": [], "routes_to_poses": [], "routes_to_poses_points": []}
    ms = {"routes_to_poses": [], "routes_to_poses_points": []}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        vertex, cost, _ = p.connect_poses(poses)
        ts["connect_poses"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        routes, length = p.routes_to_poses(poses)
        ts["routes_to_poses"].append((time.perf_counter() - t0) * 1e3)
        ms["routes_to_poses"].append(ctx.pose_routes_ms())
        t0 = time.perf_counter()
        routes, length, paths = p.routes_to_poses(poses, points=True)
        ts["routes_to_poses_points"].append((time.perf_counter() - t0) * 1e3)
        ms["routes_to_poses_points"].append(ctx.pose_routes_ms())
    on = vertex >= 0
    rows = sum(len(r) for r in routes if r is not None)
    points = sum(len(q) for q in paths if q is not None)
    assert np.array_equal(length[on].view(np.int64), cost[on].view(np.int64)) and np.all(np.isinf(length[~on])), "length != cost"
    # the host route of the first `host` poses
    h = min(args.host, m)
    t0 = time.perf_counter()
    host_routes = p.paths_to_poses(T, poses[:h])
    t1 = time.perf_counter()
    host_lines = [p.poses_polyline(r) if r is not None else None for r in host_routes]
    t2 = time.perf_counter()
    legs = beyond = 0
    worst, listed = 0.0, []
    for g in range(h):
        if host_routes[g] is None:
            assert routes[g] is None
            continue
        assert np.array_equal(host_routes[g], routes[g]), "the device rows differ from paths_to_poses"
        at = 0
        for a, b in zip(routes[g][:-1], routes[g][1:]):
            th0, th1 = 2.0 * np.pi * a[2] / CFG["nh"], 2.0 * np.pi * b[2] / CFG["nh"]
            n = int(np.floor(float(dubins_shortest(a[0], a[1], th0, b[0], b[1], th1, CFG["rho"])[3]) / 0.5)) + 1
            line = dubins_polyline(a, b, CFG["rho"], CFG["nh"], 0.5)
            n = min(n, len(paths[g]) - 1 - at, len(line))
            dev = float(np.max(np.abs(line[:n] - paths[g][at:at + n]))) if n else 0.0
            at += n
            legs += 1
            if dev >= TOL:
                beyond += 1
                listed.append([int(x) for x in a] + [int(x) for x in b] + [dev])
            else:
                worst = max(worst, dev)
        if at != len(paths[g]) - 1:  # (a length within an ulp of a multiple of 0.5: the two arithmetics count one sample apart)
            listed.append(["route", g, "points", len(paths[g]) - 1, "libm counts", at])
    out = {
        "lib": os.path.basename(_ffi.LIB_PATH), "lib_sha256": lib_build_id(_ffi.LIB_PATH), "tree_vertices": int(p.last_stats["j"]), "goals": m,
        "goals_connected": int(on.sum()), "rows": rows, "points": points, "call_ms": ts,
        "stage_ms": {k: [statistics.median(x[s] for x in v) for s in range(4)] for k, v in ms.items()},
        "bytes_read_back": {"routes_to_poses": 28 * m + 8 + 9 * rows, "routes_to_poses_points": 36 * m + 16 + 9 * rows + 16 * points},
        "host": {"poses": h, "paths_to_poses_ms": (t1 - t0) * 1e3, "poses_polyline_ms": (t2 - t1) * 1e3, "host_points": sum(len(x) for x in host_lines if x is not None)},
        "agreement": {"tolerance": TOL, "legs": legs, "legs_within_tol": legs - beyond, "legs_beyond_tol": beyond, "max_abs_dev_within": worst, "listed": listed[:16]},
        "length_equals_cost_bit_for_bit": True,
    }
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--goals", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host", type=int, default=256, help="poses whose host route is timed and scaled to --goals")
    ap.add_argument("--limit", type=int, default=420, help="seconds the child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_routes_wall.json"))
    ap.add_argument("--child", action="store_true", help="(internal) the measurement itself")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--goals", str(args.goals), "--warmup", str(args.warmup),
           "--reps", str(args.reps), "--host", str(args.host)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:  # nothing more is started on the device after a child that failed, faulted or ran out of time
        raise SystemExit("the child ended with status %d:\n%s" % (r.returncode, r.stderr[-3000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    m = res["goals"]
    out = {
        "what": "wall time of connect_poses, routes_to_poses and routes_to_poses(points=True) for %d goal poses against one Dubins-RRT* tree of BASELINE "
                "config 5's shape (2048x2048 noise grid seed 3, n=100000, r_rewire=64, rho=8, 64 headings, planner seed 0; goal poses from the free cells "
                "with uniform headings, seed 11), the three calls alternated in one process, %d rounds after %d warm-up calls; the host route "
                "(paths_to_poses + poses_polyline) timed on %d poses and scaled" % (m, args.reps, args.warmup, res["host"]["poses"]),
    }
    out.update({k: res[k] for k in ("goals", "tree_vertices", "goals_connected", "rows", "points", "lib", "lib_sha256")})
    for k, v in res["call_ms"].items():
        out[k] = spread(v)
    base = out["connect_poses"]["median_ms"]
    stage_names = ["decision (rrt_pose_goals_kernel)", "depth + scan", "rows + legs + lengths (+ point scan)", "points"]
    for k in ("routes_to_poses", "routes_to_poses_points"):
        out[k]["beyond_connect_poses_ms"] = out[k]["median_ms"] - base
        out[k]["stage_ms"] = dict(zip(stage_names, res["stage_ms"][k]))
        out[k]["bytes_read_back"] = res["bytes_read_back"][k]
    h = res["host"]
    scale = m / h["poses"]
    out["host_route"] = dict(h, scaled_to_all_goals_ms={"paths_to_poses": h["paths_to_poses_ms"] * scale, "poses_polyline": h["poses_polyline_ms"] * scale,
                                                        "both": (h["paths_to_poses_ms"] + h["poses_polyline_ms"]) * scale})
    out["agreement_with_host_polyline"] = res["agreement"]
    out["length_equals_cost_bit_for_bit"] = res["length_equals_cost_bit_for_bit"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
