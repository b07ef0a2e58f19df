"""CPU-side planned cases that more than one test module uses: maps, samples and the oracle's (or the oracle-backed stand-in
planner's) plan of them.  Nothing here needs the HIP library.  The cache of oracle_planned is per process and keyed by the case's own
parameters."""
import numpy as np

import oracle
import orchelp
import rerootref
from rrtplanner_amd import hostprep
from rrtplanner_amd import rrt as amd

G = orchelp.golden("plans_A.npz")
_cache = {}

# ------------------------------------------------------------------------------------------------ one wall on 64 x 48, the stand-in planner
WALL64_XS, WALL64_XG = np.array((3, 3)), np.array((55, 40))


def wall64_og():
    og = np.zeros((64, 48), dtype=np.int64)
    og[30:33, :36] = 1
    return og


def wall64_planned(n=300):
    p = orchelp.use_oracle(amd.RRTStar(wall64_og(), n, 12, pbar=False, seed=0))
    T, gv = p.plan(WALL64_XS, WALL64_XG)
    return p, T, gv


def pinned_goal_cases():
    """three goldens of different grids and planners whose goal was connected"""
    G = orchelp.golden("plans_A.npz")
    seen, out = set(), []
    for m in sorted(G.manifest, key=lambda m: -m["n"]):
        if m["alg"] in (0, 1) and m.get("rows") == m["n"] + 1 and m["vgoal"] > 50 and (m["grid"], m["alg"]) not in seen and m["grid"] != "empty43x100":
            seen.add((m["grid"], m["alg"]))
            out.append(m["id"])
    return out[:3]


# ------------------------------------------------------------------------------------------------ the maps of plans_A.npz, grown and re-rooted
GROW_CASES = [("noise200", 0, 300, 200, 11), ("noise200", 1, 300, 200, 12), ("maze64x96", 1, 250, 150, 13), ("square100", 0, 200, 120, 14),
              ("square100", 1, 200, 120, 15)]


def grow_setup(grid, alg, n, m, seed):
    og8 = oracle.og_u8(G.grid(grid))
    free = np.argwhere(og8 == 0)
    rng = np.random.default_rng(seed)
    xs, xg = free[rng.integers(len(free))], free[rng.integers(len(free))]
    samples = hostprep.draw_free_samples(rng, free, n + m)
    r2 = hostprep.radius_threshold(12) if alg else 0
    return og8, xs, xg, samples, r2


def hand_tree():
    """root (2, 2); 1 and 2 hang on it, 3 on 1, 4 on 3, 5 sits on the ROOT's cell and hangs on 2"""
    pts = np.array([(2, 2), (2, 10), (10, 2), (2, 16), (8, 16), (2, 2)])
    parent = np.array([-1, 0, 0, 1, 3, 2])
    vcost = np.array([0.0, 8.0, 8.0, 14.0, 20.0, 16.0])
    return pts, parent, vcost


def oracle_planned(grid, alg, n, seed):
    """the recipe of the issue: xs, xg as grow_setup draws them, then n samples; the oracle's plan"""
    key = (grid, alg, n, seed)
    if key not in _cache:
        og8, xs, xg, samples, r2 = grow_setup(grid, alg, n, 0, seed)
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2)
        _cache[key] = dict(og8=og8, xs=xs, xg=xg, samples=samples, r2=r2, st=st, ro=ro, n=n, alg=alg)
    return _cache[key]


MAZE = ("maze64x96", 1, 250, 13)
NOISE = ("noise200", 1, 1500, 16)


def one_way_edges(c):
    """the vertices k whose edge is free parent -> child and blocked child -> parent"""
    ro, og8 = c["ro"], c["og8"]
    return [k for k in range(1, ro.j) if oracle.collisionfree(og8, ro.pts[int(ro.parent[k])], ro.pts[k])[0]
            and not oracle.collisionfree(og8, ro.pts[k], ro.pts[int(ro.parent[k])])[0]]


def roots_behind(c, edges):
    """the candidate roots whose way to vertex 0 reverses one of `edges`"""
    ro = c["ro"]
    return [r for r in range(ro.j) if set(rerootref.path_to_root(ro.parent, ro.j, r)[:-1]) & set(edges)]
