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
from rrtplanner_amd import _ffi, hostprep, perlin_occupancygrid
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins
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


# ------------------------------------------------------------------------------------- trees made for one purpose each
def made(name, og8, n, star, r, rho, nh, xs, xg, samples, heads, goals, logs=False):
    # (goals: a list of poses, or a function of the oracle's result that returns one)
    """a Workload from explicit parts: the oracle's tree for the stream (samples, heads), this file's answers for `goals`"""
    w = Workload()
    w.name, w.n, w.star, w.rho, w.nh = name, int(n), int(star), float(rho), int(nh)
    w.og8 = np.ascontiguousarray(og8, dtype=np.uint8)
    w.og = w.og8.astype(np.int64)
    w.xs, w.xg = tuple(int(v) for v in xs), tuple(int(v) for v in xg)
    w.samples, w.heads = np.ascontiguousarray(samples, dtype=np.int64).reshape(n, 2), np.ascontiguousarray(heads, dtype=np.int64).reshape(n)
    w.r2 = hostprep.radius_threshold(r) if star else 0
    w.status, w.ro = oracle.dubins_plan(w.og8, w.n, w.star, w.xs, w.xg, w.samples, w.heads, r2_rewire=w.r2, rho=w.rho, nh=w.nh, logs=logs)
    w.j = w.ro.j
    w.goals = np.array(goals(w.ro) if callable(goals) else goals, dtype=np.int64).reshape(-1, 3)
    w.i_obstacle, w.i_own = None, None
    w.vertex, w.cost, w.rank, w.c = connect(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, w.goals, w.rho, w.nh, want_costs=True)
    return w


def own_goal_row(w):
    """what plan() leaves for the query's own goal pose: (found, vgoal, parent of the goal row, its cost)"""
    ro = w.ro
    return (bool(ro.found), int(ro.vgoal)) + ((int(ro.parent[ro.vgoal]), float(ro.vcost[ro.vgoal])) if ro.found else (-1, np.inf))


# ---- exact ties.  An empty 100 x 100 map, the start at (20, 50) heading along +x.
TIE_START = (20, 50, 0)
TIE_PAIRS = ((4.0, 16), (3.0, 64), (1.5, 8))               # (rho, nh)
TIE_PLACES = {"first": (60, 0), "hundredth": (300, 117), "above_1024": (1800, 1560)}  # (n, the sample that repeats the start pose)


@functools.lru_cache(maxsize=None)
def tie_duplicate(rho, nh, star, place):
    """A sample on the start's cell with the start's heading: the oracle keys `sampled` on cells and does not mark the start's, so
    the pose is accepted once, with parent 0 and a word of length exactly 0.0 -- vertex w.dup has the start's pose and the
    start's cost, and c[0] == c[w.dup] for EVERY goal pose by construction.  The goals: every heading of one cell, poses ahead
    of the start, beside it and behind it, a border pose, and the planner's own goal.
    What the place decides: the thread and the pass of the kernel's scatter that handles the duplicate (vertex k goes to thread
    k % 1024 in pass k // 1024), hence the order in which the two arrive in their bucket.  It does NOT decide the round of the walk:
    the two share a bound, hence a bucket, and sit side by side in the sorted order whatever the duplicate's index is."""
    n, at = TIE_PLACES[place]
    og8 = np.zeros((100, 100), dtype=np.uint8)
    rng = np.random.default_rng(1000 + at)
    free = np.argwhere(og8 == 0)
    free = free[(free[:, 0] != TIE_START[0]) | (free[:, 1] != TIE_START[1])]  # nothing else may use up the start's cell
    samples = hostprep.draw_free_samples(rng, free, n)
    heads = rng.integers(0, nh, n)
    samples[at], heads[at] = TIE_START[:2], TIE_START[2]
    xg = (80, 58, 3 % nh)
    cell = (44, 47)
    goals = [(cell[0], cell[1], h) for h in range(nh)] + [(30, 50, 0), (90, 50, 0), (21, 50, 0), (20, 60, nh // 4), (8, 50, nh // 2), (20, 50, 0),
                                                           (99, 99, 0), (60, 20, nh - 1), xg]
    w = made(f"tie-duplicate rho {rho} nh {nh} star {star} {place}", og8, n, star, 20, rho, nh, TIE_START, xg, samples, heads, goals)
    pose = np.column_stack([w.ro.pts[:w.j], w.ro.head[:w.j]])
    same = np.flatnonzero((pose == np.array(TIE_START)).all(axis=1))
    w.dup = int(same[1]) if len(same) == 2 else -1
    return w


def check_tie_duplicate(w, place):
    j, k = w.j, w.dup
    assert k > 0 and w.ro.parent[k] == 0 and w.ro.vcost[k] == 0.0, (w.name, k)
    assert {"first": k == 1, "hundredth": 64 < k < 200, "above_1024": 1024 < k < j}[place], (w.name, k, j)
    assert np.array_equal(w.c[:, 0].view(np.int64), w.c[:, k].view(np.int64))  # equal bits, goal by goal
    assert not np.any(w.vertex == k), (w.name, np.flatnonzero(w.vertex == k))
    root = int((w.vertex == 0).sum())
    assert root >= 8 and np.all(w.rank[w.vertex == 0] == 0), (w.name, root)  # the tie is the winning key, not one further down
    assert own_goal_row(w)[2] != k


@functools.lru_cache(maxsize=None)
def tie_collinear(rho, nh, star, fillers):
    """(a) The start heads along +x, vertex 1 is (50, 50, 0), the goal (90, 50, 0): both reach it on a straight word and
    0 + 70 == 30 + 40 exactly.  `fillers` accepted poses of the far rows y >= 85 come between vertex 1 and ...
    (b) ... with one obstacle cell on the row y = 50 between vertex 1 and the goal, the start and vertex 1 are blocked.  L = (50, 42)
    and R = (50, 58), heading along +x, hang off vertex 1 by mirror-image words and reach the goal by mirror-image words: the tie is
    between the second and the third candidate.  (Mirror-image words are evaluated by different closed forms and need not agree in
    the last bit: the offset 8 is one at which they do for every pair of TIE_PAIRS, and check_tie_collinear holds it to that.)  Returns (a, b, iL, iR)."""
    og8 = np.zeros((100, 100), dtype=np.uint8)
    xg = (90, 50, 0)
    fill = [(60 - k % 50, 85 + 5 * (k // 50)) for k in range(fillers)]  # far rows, driven away from the goal: dearer than the tie
    fh = [nh // 2] * fillers
    cells = [(50, 50)] + fill
    a = made(f"tie-collinear rho {rho} nh {nh} star {star} fillers {fillers}", og8, len(cells) + 1, star, 20, rho, nh, TIE_START, xg,
             cells + [(0, 0)], [0] + fh + [0], [xg, (90, 50, 1 % nh), (70, 50, 0)])
    og8 = og8.copy()
    og8[70, 50] = 1
    cells = [(50, 50), (50, 42)] + fill + [(50, 58)]
    b = made(f"tie-mirror rho {rho} nh {nh} star {star} fillers {fillers}", og8, len(cells) + 1, star, 20, rho, nh, TIE_START, xg,
             cells + [(0, 0)], [0, 0] + fh + [0, 0], [xg, (90, 50, 1 % nh), (60, 50, 0)])
    return a, b, 2, fillers + 3


def check_tie_collinear(a, b, iL, iR):
    assert a.j == a.n and b.j == b.n  # every sample but the last was accepted
    assert a.c[0, 0] == a.c[0, 1] == 70.0 and (a.vertex[0], a.cost[0], a.rank[0]) == (0, 70.0, 0), (a.name, a.c[0, :2])
    assert np.all(a.c[0, 2:] > 70.0)
    for k, cell in ((iL, (50, 42)), (iR, (50, 58))):
        assert tuple(b.ro.pts[k]) == cell and b.ro.head[k] == 0 and b.ro.parent[k] == 1, (b.name, k)
    assert b.ro.vcost[iL] == b.ro.vcost[iR] and b.c[0, iL].view(np.int64) == b.c[0, iR].view(np.int64), (b.name, b.c[0, iL], b.c[0, iR])
    order = np.argsort(b.c[0], kind="stable")
    blocked = [k for k in order[:b.rank[0]].tolist()]
    assert b.rank[0] >= 1 and 0 in blocked and order[b.rank[0] + 1] == iR, (b.name, b.rank[0], order[:6])  # the cheaper ones are blocked, the next is R
    assert (b.vertex[0], b.cost[0]) == (iL, b.c[0, iL])
    assert sweep_free(b.og8, b.ro.pts[iR], b.ro.head[iR], tuple(b.goals[0]), b.rho, b.nh, b.c[0, iR] - b.ro.vcost[iR])  # R would connect


@functools.lru_cache(maxsize=None)
def tie_chain():
    """Every cost equal: the start (2, 12) heads along +x on a 1300 x 24 map, the samples are the cells (3, 12), (4, 12), ... with
    that heading, each joined to the one before by a straight word.  For the goal (1290, 12, 0) every vertex costs
    (x - 2) + (1290 - x) == 1288.0 and sees it; all bounds are equal, too (one bucket, scale == 0), and j > 1024: the walk takes two
    rounds.  Every comparison between lanes and between waves is a tie between two indices: a wave_min_f64_idx or a wave merge that is
    not strict on (c, k) gives another answer than vertex 0.  Between the ROUNDS the chain decides nothing by itself: the order inside
    the one bucket is the order in which the scatter's atomics land, vertex 0 lands among the first 1024 in practice, and every
    candidate of round 2 then has a higher index than the best of round 1."""
    og8 = np.zeros((1300, 24), dtype=np.uint8)
    j = 1100
    cells = [(x, 12) for x in range(3, 2 + j)]
    xg = (1290, 12, 0)
    w = made("tie-chain", og8, j, 0, 0, 4.0, 16, (2, 12, 0), xg, cells + [(0, 0)], [0] * j, [xg, (1290, 12, 4), (1200, 12, 0), (1290, 20, 0)])
    return w


def check_tie_chain(w):
    assert w.j == w.n == 1100 and np.all(w.ro.parent[1:w.j] == np.arange(w.j - 1)) and np.all(w.c[0] == 1288.0) and np.all(w.c[2] == 1198.0)
    assert w.vertex.tolist()[:3:2] == [0, 0] and w.cost[0] == 1288.0


# ---- trees of exactly j vertices.  The tree grows in the free left part of a 128 x 96 map; a wall x in [70, 73), open above
# y = 80, stands between it and some of the goals.
STRIDE_J = (1, 2, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049)
STRIDE_RHO, STRIDE_NH, STRIDE_START = 3.0, 16, (30, 48, 0)
#               first candidate ........  past blocked ones .......  behind the wall ....  on it ....  a vertex pose
#               the corners, and one more past blocked candidates: through the wall's opening
STRIDE_GOALS = [(12, 48, 8), (30, 62, 4), (45, 48, 0), (50, 44, 12), (100, 30, 0), (90, 10, 12), (71, 10, 0), (30, 48, 0),
                (0, 0, 10), (127, 95, 2), (0, 95, 6), (127, 0, 14), (100, 88, 0)]
I_WALL, I_BEHIND, I_VERTEX = 6, (4, 5), 7


def _stride_map():
    og8 = np.zeros((128, 96), dtype=np.uint8)
    og8[70:73, :80] = 1   # the wall
    og8[36:39, 40:57] = 1  # a screen in front of the start: what lies beyond it is reached from other vertices, past the root's blocked word
    return og8


@functools.lru_cache(maxsize=None)
def stride_tree(j, star):
    """A tree of exactly j vertices: the stream of seed j, cut after the sample that the oracle accepts as vertex j - 1.  (A Dubins
    sample is not always accepted, so n >= j; and the oracle refuses every sample once j == n -- the tree is full --, which a
    stream cut there never meets before its last sample: the accepts of the long stream are the accepts of the cut one.)"""
    og8 = _stride_map()
    cells = np.array([(x, y) for x in range(60) for y in range(96) if og8[x, y] == 0 and (x, y) != STRIDE_START[:2]])
    rng = np.random.default_rng(j)
    perm = cells[rng.permutation(len(cells))]
    hd = rng.integers(0, STRIDE_NH, len(cells))
    xg, r2 = (120, 90, 2), hostprep.radius_threshold(12) if star else 0
    n = 1
    if j > 1:
        long = min(len(cells), 2 * j + 64)
        st, ro = oracle.dubins_plan(og8, long, star, STRIDE_START, xg, perm[:long], hd[:long], r2_rewire=r2, rho=STRIDE_RHO, nh=STRIDE_NH)
        n = max(int(np.flatnonzero(ro.accept_log)[j - 2]) + 1, j)  # (n == j: every sample but the last is accepted, the last refused)
    return made(f"stride j {j} star {star}", og8, n, star, 12, STRIDE_RHO, STRIDE_NH, STRIDE_START, xg, perm[:n], hd[:n], STRIDE_GOALS)


def check_stride_tree(w, j):
    assert w.j == j, (w.name, w.n, w.j)
    v, rank = w.vertex, w.rank
    assert v[I_WALL] == -1 and v[I_VERTEX] == 0 and w.cost[I_VERTEX] == 0.0, (w.name, v)
    if j >= 63:
        assert (v >= 0).sum() >= 4 and (rank > 0).any() and (rank[v >= 0] == 0).any(), (w.name, v, rank)
    if j == 1:
        assert (v[[0, I_VERTEX]] == 0).all() and (v >= 0).sum() >= 2, (w.name, v)  # scale == 0 with a real answer: the root alone connects


# ---- a fuzz over small trees: the draw of test_dubins.py::test_device_dubins_fuzz_small, then M = 8 goal poses per tree
FUZZ_CASES, FUZZ_M, FUZZ_SEED = 120, 8, 99


@functools.lru_cache(maxsize=None)
def fuzz_cases():
    rng = np.random.default_rng(FUZZ_SEED)
    out = []
    for case in range(FUZZ_CASES):
        W, H = int(rng.integers(8, 70)), int(rng.integers(8, 70))
        og8 = (rng.uniform(size=(W, H)) < rng.choice([0.0, 0.1, 0.3])).astype(np.uint8)
        free = np.argwhere(og8 == 0)
        if free.shape[0] < 2:
            continue
        star = int(rng.integers(0, 2))
        n = int(rng.choice([1, 2, 17, 64, 100, 300, 800]))
        nh = int(rng.choice([1, 8, 64, 256]))
        rho = float(rng.choice([0.5, 1.5, 4.0, 12.0]))
        rr = float(rng.choice([2, 8, 20, 500]))
        a, b = free[rng.integers(0, free.shape[0])], free[rng.integers(0, free.shape[0])]
        xs, xg = (int(a[0]), int(a[1]), int(rng.integers(0, nh))), (int(b[0]), int(b[1]), int(rng.integers(0, nh)))
        srng = np.random.default_rng(case)
        samples = hostprep.draw_free_samples(srng, free, n)
        heads = srng.integers(0, nh, size=n)
        grng = np.random.default_rng(5000 + case)
        cells = np.column_stack([grng.integers(0, W, FUZZ_M - 2), grng.integers(0, H, FUZZ_M - 2), grng.integers(0, nh, FUZZ_M - 2)])

        def goals(ro, cells=cells, grng=grng, xg=xg):
            v = int(grng.integers(0, ro.j))  # ... the pose of a random vertex, and the query's own goal pose
            return cells.tolist() + [(int(ro.pts[v, 0]), int(ro.pts[v, 1]), int(ro.head[v])), xg]

        w = made(f"pose fuzz case {case}: {W}x{H} star {star} n {n} nh {nh} rho {rho} r {rr} xs {xs} xg {xg}", og8, n, star, rr, rho, nh, xs, xg,
                 samples, heads, goals, logs=True)
        w.rr, w.serial = rr, bool(case % 3 == 2)
        out.append(w)
    return out


def fuzz_coverage(cases):
    """(goals, connected, connected past a blocked first candidate) over all cases"""
    return (sum(len(w.goals) for w in cases), sum(int((w.vertex >= 0).sum()) for w in cases), sum(int((w.rank > 0).sum()) for w in cases))


# ------------------------------------------------------------------------------------- the independent audit (oracle/dubins_ref.c)
def goals_audit(w, vertex, cost):
    return oracle.dubins_goals_audit(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, w.goals, vertex, cost, rho=w.rho, nh=w.nh)


def assert_goals_audit_clean(a, vertex):
    """the policy of posecalls.assert_audit_clean for the goal decisions: every answer equal to dubins_ref.c's own, or within
    the stated tolerance / ambiguity -- never plainly different -- and the tolerance classes the exception, not the rule"""
    connected = int((np.asarray(vertex) >= 0).sum())
    assert a["answer_wrong"] == 0 and a["answer_blocked"] == 0 and a["cost_mismatch"] == 0 and a["missed"] == 0 and a["phantom"] == 0, a
    assert a["first_bad_goal"] == -1 and a["max_cost_err"] < 1e-8, a
    assert a["n_connected"] == connected and a["answer_is_argmin"] + a["answer_within_tol"] == connected, a
    assert a["answer_within_tol"] + a["answer_blocked_ambiguous"] <= max(3, len(vertex) // 1000), a


# ------------------------------------------------------------------------------------- a workload as the device and the planners take it
def device_query(w):
    return _ffi.make_query(_ffi.ALG_DUBINS_STAR if w.star else _ffi.ALG_DUBINS, w.n, w.xs, w.xg, w.samples, r2_rewire=w.r2, headings=w.heads,
                           rho=w.rho, nh=w.nh)


def planner_of(w):
    r = SPECS[w.name][4]
    args = (w.og, w.n) + ((r,) if w.star else ()) + (w.rho,)
    return (RRTStarDubins if w.star else RRTDubins)(*args, n_headings=w.nh, pbar=False, seed=SPECS[w.name][7])
