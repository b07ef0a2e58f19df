"""Host restatement of rrt_batch_pose_routes (Batch.pose_routes, RRTDubins / RRTStarDubins .routes_to_poses): the check of the
pose-routes tests.

Given the finished Dubins tree of oracle.dubins_plan (pts, head, parent; root 0) and, per goal pose, the vertex and cost that
poseref.connect (or posekeepref.connect_alive on a changed map) answers:
  rows    a Python parent walk from vertex[g] to the root, reversed, then the goal pose; id -1 for the goal row; none for vertex -1
  length  the Python sum, left to right from 0.0, of oracle.dub_shortest(row r, row r + 1).len -- the arithmetic of
          include/rrt_dubins.h, which gcc and gfx950 evaluate bit for bit alike
  points  per leg the samples of tests/dubpoints (dub_sweep_point of include/rrt_dubins_points.h in gcc: Python and numpy have no fused
          multiply-add), then the goal cell as doubles
Everything is CSR over the goals.  The points share a header with the kernel; what holds that header to something else is in
test_pose_routes_cpu.py: the oracle's own sweep cells, exactly, and numpy's libm polyline within 1e-8."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np

import oracle
import poseref
import posekeepref

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("dubpoints_build", os.path.join(_HERE, "dubpoints", "build.py"))
dubpoints = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dubpoints)


def leg(a, b, rho, nh):
    """(length, points float64 (nsamples, 2)) of the leg from pose a to pose b = (x, y, heading index)"""
    args = (float(a[0]), float(a[1]), poseref.theta(a[2], nh), float(b[0]), float(b[1]), poseref.theta(b[2], nh), float(rho))
    length = oracle.dub_shortest(*args)[3]
    assert np.isfinite(length), (a, b)
    cap = int(length / 0.5) + 2
    out = np.zeros((cap, 2), dtype=np.float64)
    got = C.c_double(0.0)
    n = dubpoints.lib().dubpoints_leg(*args, out.ctypes.data, cap, C.byref(got))
    assert 0 < n <= cap and got.value == length, (a, b, n, cap, got.value, length)  # the helper's word is the oracle's
    return length, out[:n]


def walk(parent, v, j):
    """the vertices root .. v"""
    ids = [int(v)]
    while ids[-1] != 0:
        ids.append(int(parent[ids[-1]]))
        assert 0 <= ids[-1] < j and len(ids) <= j, "the parent pointers do not lead to vertex 0"
    return ids[::-1]


class Routes:
    def route(self, g):
        return self.rows[self.offsets[g]:self.offsets[g + 1]]

    def path(self, g):
        return self.points[self.point_offsets[g]:self.point_offsets[g + 1]]

    def legs_of(self, g):
        """[(first point, points)] of the legs of goal g, the goal's own point excluded"""
        return [(a, n) for a, n in self.leg_spans[self.offsets[g]:self.offsets[g + 1]] if n >= 0]


def routes(pts, head, parent, j, goals, vertex, cost, rho, nh):
    """what Batch.pose_routes(points=True) returns for these goals, as a Routes: vertex int32[M], cost f64[M], length f64[M],
    offsets int64[M + 1], rows int32 (R, 3), ids int32[R], point_offsets int64[M + 1], points f64 (P, 2).
    leg_spans[r] = (offset of the first point of the leg that starts at row r, its points), (.., -1) for a goal row."""
    goals = np.asarray(goals, dtype=np.int64).reshape(-1, 3)
    m = len(goals)
    r = Routes()
    r.vertex, r.cost = np.asarray(vertex, dtype=np.int32), np.asarray(cost, dtype=np.float64)
    r.length = np.full(m, np.inf)
    rows, ids, chunks, spans = [], [], [], []
    r.offsets, r.point_offsets = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    seen = {}
    npoints = 0
    for g in range(m):
        if r.vertex[g] >= 0:
            vs = walk(parent, r.vertex[g], j)
            poses = [(int(pts[u][0]), int(pts[u][1]), int(head[u])) for u in vs] + [tuple(int(x) for x in goals[g])]
            total = 0.0
            for a, b in zip(poses[:-1], poses[1:]):
                if (a, b) not in seen:
                    seen[(a, b)] = leg(a, b, rho, nh)
                length, p = seen[(a, b)]
                total = total + length
                spans.append((npoints, len(p)))
                chunks.append(p)
                npoints += len(p)
            spans.append((npoints, -1))
            chunks.append(np.array([[float(goals[g][0]), float(goals[g][1])]]))
            npoints += 1
            r.length[g] = total
            rows += poses
            ids += vs + [-1]
        r.offsets[g + 1] = len(rows)
        r.point_offsets[g + 1] = npoints
    r.rows = np.array(rows, dtype=np.int32).reshape(-1, 3)
    r.ids = np.array(ids, dtype=np.int32)
    r.points = np.concatenate(chunks) if chunks else np.zeros((0, 2))
    r.leg_spans = spans
    return r


DEEP = 6  # goal poses added to a workload's own: the poses of its deepest vertices, whose routes are the longest the tree has


def depths(parent, j):
    d = np.zeros(j, dtype=np.int64)
    for k in range(1, j):
        d[k] = len(walk(parent, k, j)) - 1
    return d


class Case:
    pass


def _case(w, og8, alive):
    """workload w with DEEP more goal poses, answered on the map og8 over the vertices alive[k] (None: all), and the routes of that"""
    c = Case()
    c.w, c.og8 = w, og8
    ro = w.ro
    d = depths(ro.parent, w.j)
    if alive is not None:
        d = np.where(alive, d, -1)
    deep = np.argsort(-d, kind="stable")[:DEEP if w.j > 1 else 0]  # (a tree that is its root alone, workload F: nothing is added)
    extra = np.array([(int(ro.pts[u][0]), int(ro.pts[u][1]), int(ro.head[u])) for u in deep.tolist()], dtype=np.int64).reshape(-1, 3)
    c.goals = np.concatenate([w.goals, extra])
    if alive is None:
        v, cost, _ = poseref.connect(og8, ro.pts, ro.head, ro.vcost, w.j, extra, w.rho, w.nh)
        c.vertex, c.cost = np.concatenate([w.vertex, v]), np.concatenate([w.cost, cost])
    else:
        c.vertex, c.cost = posekeepref.connect_alive(og8, alive, ro.pts, ro.head, ro.vcost, c.goals, w.rho, w.nh)
    c.alive = alive
    c.routes = routes(ro.pts, ro.head, ro.parent, w.j, c.goals, c.vertex, c.cost, w.rho, w.nh)
    return c


@functools.lru_cache(maxsize=None)
def case(name):
    """workload `name` of poseref on its own map (computed once per process and shared; nobody writes to it)"""
    w = poseref.workload(name)
    return _case(w, w.og8, None)


@functools.lru_cache(maxsize=None)
def kept_case(name):
    """workload `name` after keep_pose_tree on posekeepref.changed(name)'s map"""
    k = posekeepref.changed(name)
    return _case(k.w, k.og8, k.alive)


def made_case(w):
    """a hand-made workload of poseref (made, stride_tree, tie_chain, tie_duplicate): its own goals, nothing added"""
    if "_pose_routes" not in w.__dict__:
        c = Case()
        c.w, c.og8, c.goals, c.vertex, c.cost, c.alive = w, w.og8, w.goals, w.vertex, w.cost, None
        c.routes = routes(w.ro.pts, w.ro.head, w.ro.parent, w.j, w.goals, w.vertex, w.cost, w.rho, w.nh)
        w._pose_routes = c
    return w._pose_routes


# ---- chains.  On an empty map the root reaches every goal at least as cheaply as any vertex of a chain does, and wins.  Here a wall
# above the chain's row, x < the last vertex's, blocks the rising word from every vertex but the last: the route is the whole chain.
CHAIN_RHO, CHAIN_NH, CHAIN_Y = 4.0, 16, 12


@functools.lru_cache(maxsize=None)
def chain(xs):
    """a chain of len(xs) vertices at (x, CHAIN_Y) heading along +x, the root first; the goals: behind the wall's end, one of them
    with another heading, and one that nothing reaches"""
    last = xs[-1]
    og8 = np.zeros((last + 40, 24), dtype=np.uint8)
    og8[:last, CHAIN_Y + 2:] = 1
    j = len(xs)
    cells = [(x, CHAIN_Y) for x in xs[1:]]
    goals = [(last + 9, CHAIN_Y + 8, 0), (last + 12, CHAIN_Y + 7, 1), (5, CHAIN_Y + 6, 0)]
    w = poseref.made(f"chain of {j} to x {last}", og8, j, 0, 0, CHAIN_RHO, CHAIN_NH, (xs[0], CHAIN_Y, 0), (last + 30, CHAIN_Y, 0), cells + [(0, 0)],
                     [0] * j, goals)
    return made_case(w)


def half_cell_chain():
    """spacing 4: every tree leg is a straight word of length 4.0, an exact multiple of DUB_DS"""
    return chain(tuple(range(2, 43, 4)))


def long_chain():
    """1100 vertices: a route of 1101 rows (the last vertex stands 8 cells off, so that its neighbour's word meets the wall)"""
    return chain(tuple(range(2, 1101)) + (1108,))


def pick(r, sel):
    """the Routes of the goals `sel` of r's alone, in that order: what a goal gets does not depend on the goals beside it"""
    s = Routes()
    s.vertex, s.cost, s.length = r.vertex[sel], r.cost[sel], r.length[sel]
    s.offsets = np.concatenate([[0], np.cumsum(np.diff(r.offsets)[sel])]).astype(np.int64)
    s.point_offsets = np.concatenate([[0], np.cumsum(np.diff(r.point_offsets)[sel])]).astype(np.int64)
    s.rows = np.concatenate([r.route(g) for g in sel])
    s.ids = np.concatenate([r.ids[r.offsets[g]:r.offsets[g + 1]] for g in sel])
    s.points = np.concatenate([r.path(g) for g in sel])
    return s


def small_calls_after_a_large_one(run, c, want, shortcut):
    """Scratch that was allocated for a large call serves a small one: on one batch (run() makes it) a call with 257 poses, the pose
    with the longest route of `want` (the reference of case c) tiled, then a call with that pose alone and one with three different
    poses.  Rows and points of each small call are read back through the stand-alone calls; every array equals, bit for bit, what
    the same call gives on a batch that made no call before it, and the reference."""
    by_rows = np.argsort(-np.diff(want.offsets), kind="stable")
    g = int(by_rows[0])
    three = [int(by_rows[1]), g, int(by_rows[2])]
    k = int(want.offsets[g + 1] - want.offsets[g])
    assert k >= 3 and len({tuple(c.goals[i]) for i in three}) == 3 and np.diff(want.offsets)[three].sum() < 257 * k
    fresh = []
    for sel in ([g], three):
        f = run()
        fresh.append(f.pose_routes(0, c.goals[sel], points=True, shortcut=shortcut))
        f.close()
    b = run()
    large = b.pose_routes(0, np.tile(c.goals[g], (257, 1)), points=True, shortcut=shortcut)
    assert np.array_equal(large[3], k * np.arange(258))
    for sel, alone in zip(([g], three), fresh):
        got = b.pose_routes(0, c.goals[sel], points=True, shortcut=shortcut)
        rows, ids = b.pose_routes_rows(int(got[3][-1]))
        points = b.pose_routes_points(int(got[6][-1]))
        assert np.array_equal(rows, got[4]) and np.array_equal(ids, got[5]) and np.array_equal(points.view(np.int64), got[7].view(np.int64))
        got = got[:4] + (rows, ids, got[6], points)
        same(got, pick(want, sel))
        for x, y in zip(got, alone):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    b.close()


def same(got, want, points=True):
    """every array of Batch.pose_routes against a Routes, exactly; the floats as raw bits"""
    names = ("vertex", "cost", "length", "offsets", "rows", "ids") + (("point_offsets", "points") if points else ())
    assert len(got) == len(names), len(got)
    for name, x in zip(names, got):
        y = getattr(want, name)
        assert x.dtype == y.dtype and x.shape == y.shape, (name, x.dtype, y.dtype, x.shape, y.shape)
        if x.dtype == np.float64:
            x, y = x.view(np.int64), y.view(np.int64)
        assert np.array_equal(x, y), (name, np.argwhere(x != y)[:8].tolist())
