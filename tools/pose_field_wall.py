#!/usr/bin/env python3
"""Wall time of pose_field against connect_poses over the same cells: windows of ONE Dubins tree of BASELINE config 5's shape (the tree
of tools/poses_wall.py: Dubins-RRT*, 2048 x 2048 noise grid seed 3, n = 100 000, r_rewire = 64, rho = 8, 64 headings).

    python tools/pose_field_wall.py [--reps 15] [--out profiles/pose_field_wall.json]

Windows of 32 x 32 and 64 x 64 cells in one open and one cluttered part of the map (chosen from the map and the tree: the 64 x 64
tile with the fewest obstacle cells among those with 20 tree vertices and more, and the one whose obstacle share is nearest 35 %
among those with 5 and more; the 32 x 32 window is the middle of the tile), each at any arrival heading and at one fixed heading.
connect_poses gets the same cells as goal poses, nh poses per cell for any heading: the only other way to these arrays.  The two
alternate in one process, `reps` calls each (a case whose calls are slow stops after --case-seconds with three of each or more, and
records how many it took); the medians, the range, the counters per cell of the window and the stage times of the
field are recorded, and the answers are compared for equality in the run (any heading: per cell the (cost, heading)-first of
connect_poses' nh answers).  The measurement runs in a child process under `timeout -k 10` of its own."""
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

CFG = dict(grid=2048, grid_seed=3, n=100000, r_rewire=64, rho=8.0, nh=64)  # bench.py CONFIGS[5], one query
FIXED_HEADING = 16


def places(og8, pts):
    """{"open": (x0, y0), "cluttered": (x0, y0)}: the corners of two 64 x 64 tiles"""
    T = 64
    nt = og8.shape[0] // T
    share = (og8 != 0).reshape(nt, T, nt, T).sum(axis=(1, 3)) / float(T * T)
    count = np.zeros((nt, nt), dtype=np.int64)
    np.add.at(count, (pts[:, 0] // T, pts[:, 1] // T), 1)
    open_ = np.where(count >= 20, share, np.inf)
    clutter = np.where(count >= 5, np.abs(share - 0.35), np.inf)
    out = {}
    for name, key in (("open", open_), ("cluttered", clutter)):
        tx, ty = np.unravel_index(int(np.argmin(key)), key.shape)
        out[name] = dict(x0=int(tx) * T, y0=int(ty) * T, obstacle_share=float(share[tx, ty]), tree_vertices_in_tile=int(count[tx, ty]))
    return out


def spread(ts):
    return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}


def child(args):
    from rrtplanner_amd import _ffi, hostprep, posefield
    from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pairs

    og = perlin_occupancygrid(CFG["grid"], CFG["grid"], thresh=0.33, seed=CFG["grid_seed"])
    og8 = hostprep.og_nonzero(og)
    xs, xg = random_connected_pairs(og, np.random.default_rng(7), 1)[0]
    n, nh = CFG["n"], CFG["nh"]
    rng = np.random.default_rng(0)  # the planner's stream: n free cells, then n headings
    samples = hostprep.draw_free_samples(rng, np.argwhere(og == 0), n)
    heads = rng.integers(0, nh, size=n)
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    b = _ffi.Batch(ctx, 1, n, dubins=True)
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR, n, (int(xs[0]), int(xs[1]), 5), (int(xg[0]), int(xg[1]), 20), samples,
                              r2_rewire=hostprep.radius_threshold(CFG["r_rewire"]), headings=heads, rho=CFG["rho"], nh=nh)
    b.set_query(0, q)
    b.launch()
    b.sync()
    res = b.get_result(0)
    j = int(res.j)
    where = places(np.asarray(og8), np.asarray(res.pts[:j], dtype=np.int64))
    cases = []
    for place, at in where.items():
        for side in (32, 64):
            off = (64 - side) // 2
            window = (at["x0"] + off, at["y0"] + off, side, side)
            xx, yy = np.meshgrid(np.arange(window[0], window[0] + side), np.arange(window[1], window[1] + side), indexing="ij")
            cells = np.column_stack([xx.ravel(), yy.ravel()])
            free = int((np.asarray(og8)[window[0]:window[0] + side, window[1]:window[1] + side] == 0).sum())
            for mode, H in (("any heading", -1), ("heading %d" % FIXED_HEADING, FIXED_HEADING)):
                hs = np.arange(nh) if H < 0 else np.array([H])
                poses = np.column_stack([np.repeat(cells, len(hs), axis=0), np.tile(hs, len(cells))])
                for _ in range(args.warmup):
                    field = posefield.batch_pose_field(b, 0, window, H)
                    pv, pc = b.connect_poses(0, poses)
                tf, tp = [], []
                began = time.perf_counter()
                for _ in range(args.reps):  # the two in turns
                    if len(tf) >= 3 and time.perf_counter() - began > args.case_seconds:
                        break  # (a case of slow calls: fewer of them, and `calls` says how many)
                    t0 = time.perf_counter()
                    field = posefield.batch_pose_field(b, 0, window, H)
                    tf.append((time.perf_counter() - t0) * 1e3)
                    t0 = time.perf_counter()
                    pv, pc = b.connect_poses(0, poses)
                    tp.append((time.perf_counter() - t0) * 1e3)
                st, ms = posefield.pose_field_stats(b), posefield.pose_field_ms(b)
                words, sweeps = b.connect_poses_counts()
                pv, pc = pv.reshape(len(cells), len(hs)), pc.reshape(len(cells), len(hs))
                e = np.argmin(pc, axis=1)
                sel = (np.arange(len(cells)), e)
                same = (np.array_equal(field[0].ravel(), pv[sel]) and np.array_equal(field[1].ravel().view(np.int64), np.ascontiguousarray(pc[sel]).view(np.int64))
                        and np.array_equal(field[2].ravel(), np.where(pv[sel] >= 0, hs[e], -1)))
                if not same:
                    raise SystemExit("pose_field and connect_poses disagree on %s %s %s" % (place, window, mode))
                f, p = spread(tf), spread(tp)
                case = dict(place=place, window=list(window), mode=mode, cells=side * side, free_cells=free, connected=int((field[0] >= 0).sum()),
                            poses_per_cell=len(hs), pose_field=dict(f, stage_ms=dict(zip(("buckets", "decide", "remap", "read_back"), ms)),
                                                                    words_per_cell=st["words"] / (side * side), sweeps_per_cell=st["sweeps"] / (side * side),
                                                                    buckets_per_cell=st["buckets"] / (side * side)),
                            connect_poses=dict(p, words_per_cell=words / (side * side), sweeps_per_cell=sweeps / (side * side)),
                            connect_poses_over_pose_field=p["median_ms"] / f["median_ms"], answers_equal=True)
                print("# %s %s %s: field %.2f ms, connect_poses %.2f ms" % (place, window, mode, f["median_ms"], p["median_ms"]), file=sys.stderr, flush=True)
                cases.append(case)
    b.close()
    ctx.close()
    print(json.dumps(dict(tree_vertices=j, places=where, cases=cases)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--case-seconds", type=float, default=60.0, help="a case stops taking calls after this long, once it has three of each")
    ap.add_argument("--limit", type=int, default=1000, help="seconds the measuring child may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_field_wall.json"))
    ap.add_argument("--child", action="store_true", help="(internal) the measurement itself")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--warmup", str(args.warmup), "--reps", str(args.reps),
           "--case-seconds", str(args.case_seconds)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:  # nothing more is started on the device after a child that failed, faulted or ran out of time
        raise SystemExit("the measuring child ended with status %d" % r.returncode)
    res = json.loads(r.stdout.strip().splitlines()[-1])
    out = {"what": "pose_field against connect_poses over the same cells (nh poses per cell for any heading), wall time of a call (upload, kernels, "
                   "read-back), on one Dubins-RRT* tree of BASELINE config 5's shape (2048x2048 noise grid seed 3, n=100000, r_rewire=64, rho=8, 64 "
                   "headings, sample stream of seed 0); the two alternate in one process, %d warm-up and up to %d timed calls each (`calls`: a case stops "
                   "after %g s once it has three of each); the answers are compared for equality in the run" % (args.warmup, args.reps, args.case_seconds)}
    out.update(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
