"""Host restatement of the Dubins planners' goal decision for many goal poses against one tree: the check of the connect_poses
tests, and the workloads those tests share.

For a goal pose (gx, gy, gh):  c[k] = vcost[k] + oracle.dub_shortest(pose_k, goal).len over the vertices [0, j) -- the arithmetic of
include/rrt_dubins.h, which gcc and gfx950 evaluate bit for bit alike --, np.argsort(kind="stable"), then oracle.dub_sweep_cells in
that order until one sweep is free: every cell inside the grid and free, and the goal cell free.  A goal on an obstacle cell, or one
that no vertex reaches: -1 / inf.  Nothing is shortened by a bound: this is the literal (c, k) walk."""
import functools
import math

import numpy as np

import oracle
from rrtplanner_amd import hostprep, perlin_occupancygrid
from rrtplanner_amd.oggen import random_connected_pair

TWOPI = 2.0 * math.pi  # == DUB_TWOPI as a double


def theta(h, nh):
    return TWOPI * float(h) / float(nh)  # dub_heading: the product first, then the division


def costs(pts, head, vcost, j, goal, rho, nh):
    """c[k] for k in [0, j), float64"""
    gx, gy, gth = float(goal[0]), float(goal[1]), theta(goal[2], nh)
    c = np.empty(j, dtype=np.float64)
    for k in range(j):
        c[k] = vcost[k] + oracle.dub_shortest(float(pts[k, 0]), float(pts[k, 1]), theta(head[k], nh), gx, gy, gth, rho)[3]
    return c


def sweep_free(og8, a, ha, goal, rho, nh, length):
    """dub_sweep_free of oracle/dubins_oracle.c: a cell outside the grid blocks; then the goal cell"""
    if not math.isfinite(length):
        return False
    cells = oracle.dub_sweep_cells(a[0], a[1], theta(ha, nh), goal[0], goal[1], theta(goal[2], nh), rho, cap=int(length / 0.5) + 16)
    W, H = og8.shape
    inside = (cells[:, 0] >= 0) & (cells[:, 0] < W) & (cells[:, 1] >= 0) & (cells[:, 1] < H)
    if not inside.all() or np.any(og8[cells[:, 0], cells[:, 1]] != 0):
        return False
    return og8[goal[0], goal[1]] == 0


def connect_one(og8, pts, head, vcost, j, goal, rho, nh):
    """(vertex or -1, cost or inf, the winner's rank in (c, k) order or -1, c float64[j]) for one goal pose"""
    goal = tuple(int(v) for v in goal)
    c = costs(pts, head, vcost, j, goal, rho, nh)
    if og8[goal[0], goal[1]] != 0:
        return -1, np.inf, -1, c
    for rank, k in enumerate(np.argsort(c, kind="stable").tolist()):
        if sweep_free(og8, pts[k], head[k], goal, rho, nh, c[k] - vcost[k] if math.isfinite(c[k]) else np.inf):
            return k, c[k], rank, c
    return -1, np.inf, -1, c


def connect(og8, pts, head, vcost, j, goals, rho, nh, want_costs=False):
    """(vertex int32[M], cost float64[M], rank int64[M]) and, with want_costs, c float64[M, j]"""
    goals = np.asarray(goals).reshape(-1, 3)
    out = [connect_one(og8, pts, head, vcost, j, g, rho, nh) for g in goals]
    res = (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.float64),
           np.array([o[2] for o in out], dtype=np.int64))
    return res + (np.array([o[3] for o in out]).reshape(len(goals), j),) if want_costs else res


def any_heading(og8, pts, head, vcost, j, cell, rho, nh):
    """(vertex, cost, heading) of the (cost, heading)-smallest connected pose on `cell`; (-1, inf, -1) if none connects"""
    v, c, _ = connect(og8, pts, head, vcost, j, [(cell[0], cell[1], h) for h in range(nh)], rho, nh)
    e = int(np.argmin(c))
    return (int(v[e]), float(c[e]), e) if v[e] >= 0 else (-1, np.inf, -1)


# ------------------------------------------------------------------------------------------------------------- the workloads
#        grid        gseed n     star r    rho   nh   seed M
SPECS = {
    "A": ((96, 100), 2, 1400, 1, 20, 4.0, 16, 3, 24),
    "B": ((96, 100), 3, 1400, 1, 20, 1.0, 8, 5, 24),
    "C": ((300, 300), 1, 4000, 1, 40, 6.0, 64, 0, 12),  # j > 2 * 1024: more than two rounds of the workgroup
    "D": ((96, 100), 1, 600, 0, 0, 4.0, 16, 3, 24),
    "E": ((64, 64), 2, 300, 1, 12, 2.0, 64, 2, 24),
    "F": ((128, 128), 1, 1500, 1, 20, 25.0, 64, 6, 4),  # rho too wide for the map: the tree is the start alone, nothing connects
    "G1": ((64, 64), 2, 300, 1, 12, 3.0, 1, 2, 12),     # one heading
    "G256": ((64, 64), 2, 300, 1, 12, 3.0, 256, 2, 12),  # ... and as many as a heading byte holds
}


class Workload:
    pass


@functools.lru_cache(maxsize=None)
def workload(name, m_override=None):
    """The query, the oracle's tree, the goal poses and the answers of this file for them (computed once per process and shared;
    nobody writes to them)."""
    (W, H), gseed, n, star, r, rho, nh, seed, M = SPECS[name]
    if m_override is not None:
        M = m_override
    w = Workload()
    w.name, w.n, w.star, w.rho, w.nh = name, n, star, rho, nh
    w.og = perlin_occupancygrid(W, H, seed=gseed)
    w.og8 = oracle.og_u8(w.og)
    xs, xg = random_connected_pair(w.og, np.random.default_rng(11))
    w.xs, w.xg = (int(xs[0]), int(xs[1]), 5 % nh), (int(xg[0]), int(xg[1]), 20 % nh)
    rng = np.random.default_rng(seed)
    free = np.argwhere(w.og8 == 0)
    w.samples = hostprep.draw_free_samples(rng, free, n)
    w.heads = rng.integers(0, nh, n)
    w.r2 = hostprep.radius_threshold(r) if star else 0
    w.status, w.ro = oracle.dubins_plan(w.og8, n, star, w.xs, w.xg, w.samples, w.heads, r2_rewire=w.r2, rho=rho, nh=nh, logs=False)
    j = w.j = w.ro.j
    cells = free[rng.choice(len(free), M, replace=False)]
    rnd = [(int(c[0]), int(c[1]), int(rng.integers(0, nh))) for c in cells]
    if name.startswith("G"):
        v = j // 2
        pv = (int(w.ro.pts[v, 0]), int(w.ro.pts[v, 1]), int(w.ro.head[v]))
        w.goals = np.array([pv, (pv[0], pv[1], (pv[2] + 1) % nh), w.xs, w.xg] + rnd, dtype=np.int64)
        w.i_obstacle, w.i_own = None, 3
    else:
        ob = np.argwhere(w.og8 != 0)[0]
        w.goals = np.array(rnd + [(int(ob[0]), int(ob[1]), 0), w.xg, (0, 0, 0), (W - 1, H - 1, nh - 1)], dtype=np.int64)
        w.i_obstacle, w.i_own = M, M + 1
    w.vertex, w.cost, w.rank, w.c = connect(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, j, w.goals, rho, nh, want_costs=True)
    return w


def check_conditions(w):
    """what makes a comparison on workload w worth something: enough goals connect, enough of them past a blocked first candidate,
    the obstacle goal and the planner's own goal answer as the semantics say"""
    m = len(w.goals)
    if w.name == "F":
        assert w.status == -2 and not w.ro.found and w.j == 1 and np.all(w.vertex == -1) and np.all(np.isinf(w.cost))
    else:
        assert 2 * int((w.vertex >= 0).sum()) >= m, (w.name, int((w.vertex >= 0).sum()), m)
        assert 4 * int((w.rank > 0).sum()) >= m, (w.name, int((w.rank > 0).sum()), m)
    if w.i_obstacle is not None:
        assert w.vertex[w.i_obstacle] == -1 and w.cost[w.i_obstacle] == np.inf
    if w.ro.found:
        assert w.vertex[w.i_own] == w.ro.parent[w.ro.vgoal] and w.cost[w.i_own] == w.ro.vcost[w.ro.vgoal]
    else:
        assert w.vertex[w.i_own] == -1 and w.cost[w.i_own] == np.inf
