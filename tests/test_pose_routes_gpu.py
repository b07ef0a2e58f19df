"""GPU: routes to many goal poses over a finished Dubins tree and the vehicle's path along them (rrt_pose_route_*_kernel,
rrt_batch_pose_routes / rrt_plan_pose_routes and their _rows / _points / _ms companions, _ffi.Batch.pose_routes / Context.pose_routes,
RRTDubins / RRTStarDubins .routes_to_poses).

Every comparison is exact: vertex, cost, length, offsets, rows, ids, point_offsets as integers or raw bits, and the points as raw
bits.  The check is poseroutesref.py: a Python parent walk, the oracle's words, a Python sum, and the points of tests/dubpoints (gcc).
What holds that restatement to things the kernel does not share, and what makes the workloads worth running, is asserted without
a GPU in test_pose_routes_cpu.py.  The refusals' texts are tests/golden/pose_routes_refusals.json.  The refusal for more points than
a call may have needs an output too large for a test and is not tested."""
import json
import os

import numpy as np
import pytest

import poseref
import posekeepref
import poseroutesref as prr
from posecalls import planned_batch, refused_with_golden_text
from rrtplanner_amd import RRTStar, _ffi

pytestmark = pytest.mark.gpu

C = _ffi.C
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_routes_refusals.json")) as f:
    GOLDEN = json.load(f)


def _both(b, c, q=0):
    """with and without points against the case's routes; the rows are the same rows"""
    full = b.pose_routes(q, c.goals, points=True)
    prr.same(full, c.routes)
    bare = b.pose_routes(q, c.goals)
    prr.same(bare, c.routes, points=False)
    return full


# ------------------------------------------------------------------------------------------------ 1. the workloads
@pytest.mark.parametrize("name", ["A", "B", "D", "E", "F", "G1", "G256"])
def test_workloads_on_a_batch(gpu_ctx, name):
    c = prr.case(name)
    b = planned_batch(gpu_ctx, c.w)
    _both(b, c)
    ms = b.pose_routes_ms()
    assert len(ms) == 4 and all(t >= 0.0 for t in ms) and ms[3] == 0.0  # (the last call asked for no points)
    if name == "F":
        got = b.pose_routes(0, c.goals, points=True)
        assert np.all(got[3] == 0) and np.all(got[6] == 0) and got[4].shape == (0, 3) and got[7].shape == (0, 2)
    b.close()


def test_the_one_sample_kernel_builds_the_same_tree(gpu_ctx):
    c = prr.case("E")
    b = planned_batch(gpu_ctx, c.w, serial=True)
    _both(b, c)
    b.close()


def test_workload_c_of_4000_vertices(gpu_ctx):
    c = prr.case("C")
    assert c.w.j > 2 * 1024 and (c.vertex >= 0).sum() >= 6
    b = planned_batch(gpu_ctx, c.w)
    _both(b, c)
    b.close()


# ------------------------------------------------------------------------------------------------ 2. trees made for one purpose each
def test_half_cell_legs_and_the_chain_of_1100_vertices(gpu_ctx):
    for c in (prr.half_cell_chain(), prr.long_chain()):
        b = planned_batch(gpu_ctx, c.w)
        _both(b, c)
        b.close()


@pytest.mark.parametrize("j", [1, 2, 63, 64, 65])
def test_trees_of_exactly_j_vertices(gpu_ctx, j):
    for star in (0, 1):
        c = prr.made_case(poseref.stride_tree(j, star))
        b = planned_batch(gpu_ctx, c.w)
        _both(b, c)
        b.close()


# ------------------------------------------------------------------------------------------------ 3. the other two ways in
@pytest.mark.parametrize("name", ["A", "D"])
def test_through_rrt_plan(gpu_ctx, name):
    c = prr.case(name)
    w = c.w
    gpu_ctx.set_grid(w.og8)
    q, keep = poseref.device_query(w)
    rc, res = gpu_ctx.plan(q, w.n)
    assert rc == w.status and res.j == w.j
    prr.same(gpu_ctx.pose_routes(c.goals, points=True), c.routes)
    prr.same(gpu_ctx.pose_routes(c.goals), c.routes, points=False)
    assert len(gpu_ctx.pose_routes_ms()) == 4


@pytest.mark.parametrize("name", ["A", "D"])  # RRTStarDubins, RRTDubins
def test_through_the_planners_with_an_open_heading(name):
    c = prr.case(name)
    w, r = c.w, c.routes
    p = poseref.planner_of(w)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j
    routes, length, paths = p.routes_to_poses(c.goals, points=True)
    host = p.paths_to_poses(T, c.goals)
    assert np.array_equal(length.view(np.int64), r.length.view(np.int64))
    for g in range(len(c.goals)):
        if r.vertex[g] < 0:
            assert routes[g] is None and paths[g] is None and host[g] is None
            continue
        assert routes[g].dtype == np.int64 and np.array_equal(routes[g], r.route(g)) and np.array_equal(routes[g], host[g])  # row for row
        assert np.array_equal(paths[g].view(np.int64), r.path(g).view(np.int64))
    routes2, length2 = p.routes_to_poses(c.goals)
    assert np.array_equal(length2.view(np.int64), length.view(np.int64)) and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(routes, routes2))
    # any arrival heading: the (cost, heading)-smallest connected pose of the cell, then its route
    cells = [tuple(int(x) for x in c.goals[g][:2]) for g in (0, 1, w.i_obstacle)]
    want = [poseref.any_heading(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, cell, w.rho, w.nh) for cell in cells]
    assert want[0][0] >= 0 and want[2][0] == -1
    goals = np.array([(cell[0], cell[1], max(h, 0)) for cell, (_, _, h) in zip(cells, want)], dtype=np.int64)
    ref = prr.routes(w.ro.pts, w.ro.head, w.ro.parent, w.j, goals, [v for v, _, _ in want], [cst for _, cst, _ in want], w.rho, w.nh)
    routes, length, paths = p.routes_to_poses([(cell[0], cell[1], -1) for cell in cells], points=True)
    assert np.array_equal(length.view(np.int64), ref.length.view(np.int64))
    for g in range(3):
        if ref.vertex[g] < 0:
            assert routes[g] is None and paths[g] is None
        else:
            assert np.array_equal(routes[g], ref.route(g)) and np.array_equal(paths[g].view(np.int64), ref.path(g).view(np.int64))
    with pytest.raises(ValueError) as e:  # routes_to stays the refusal it is
        p.routes_to(c.goals[:, :2])
    assert str(e.value) == GOLDEN["dubins_planner_routes_to"][1]


# ------------------------------------------------------------------------------------------------ 4. the number of poses
def test_no_pose_one_pose_and_a_workgroup_of_them(gpu_ctx):
    c = prr.case("E")
    r = c.routes
    g = int(np.argmax(np.diff(r.offsets)))  # the pose with the longest route
    b = planned_batch(gpu_ctx, c.w)
    got = b.pose_routes(0, np.zeros((0, 3), dtype=np.int32), points=True)
    assert [len(x) for x in got] == [0, 0, 0, 1, 0, 0, 1, 0] and got[3][0] == 0 and got[6][0] == 0
    assert b.pose_routes_rows(0)[0].shape == (0, 3) and b.pose_routes_points(0).shape == (0, 2)
    k, n = int(r.offsets[g + 1] - r.offsets[g]), int(r.point_offsets[g + 1] - r.point_offsets[g])
    for m in (1, 255, 256, 257):
        vertex, cost, length, offsets, rows, ids, point_offsets, points = b.pose_routes(0, np.tile(c.goals[g], (m, 1)), points=True)
        assert np.all(vertex == r.vertex[g]) and np.all(cost.view(np.int64) == r.cost[g:g + 1].view(np.int64)) and np.all(length.view(np.int64) == cost.view(np.int64))
        assert np.array_equal(offsets, k * np.arange(m + 1)) and np.array_equal(point_offsets, n * np.arange(m + 1))
        assert np.array_equal(rows, np.tile(r.route(g), (m, 1))) and np.array_equal(ids, np.tile(r.ids[r.offsets[g]:r.offsets[g + 1]], m))
        assert np.array_equal(points.view(np.int64), np.tile(r.path(g), (m, 1)).view(np.int64))
    b.close()


def test_small_calls_after_a_large_one_on_the_same_batch(gpu_ctx):
    c = prr.case("E")
    prr.small_calls_after_a_large_one(lambda: planned_batch(gpu_ctx, c.w), c, c.routes, shortcut=False)


# ------------------------------------------------------------------------------------------------ 5. after a keep
def test_after_keep_pose_tree_and_back(gpu_ctx):
    c0, c1 = prr.case("A"), prr.kept_case("A")
    w = c0.w
    b = planned_batch(gpu_ctx, w)
    _both(b, c0)
    gpu_ctx.set_grid(c1.og8)
    assert np.array_equal(b.keep_pose_tree(0), c1.alive)
    with pytest.raises(_ffi.RRTError):  # the rows of the call before the keep are gone
        b.pose_routes_rows(len(c0.routes.rows))
    _both(b, c1)  # (its deep goal poses are those of the deepest ALIVE vertices)
    gpu_ctx.set_grid(w.og8)
    assert b.keep_pose_tree(0).all()
    _both(b, c0)  # every answer is restored
    b.close()


# ------------------------------------------------------------------------------------------------ 6. twice, and the shared scratch
def test_asked_twice_and_connect_poses_afterwards(gpu_ctx):
    c = prr.case("B")
    w = c.w
    b = planned_batch(gpu_ctx, w)
    first = b.connect_poses(0, w.goals)
    one = b.pose_routes(0, c.goals, points=True)
    two = b.pose_routes(0, c.goals, points=True)
    for x, y in zip(one, two):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y)
    prr.same(two, c.routes)
    assert b.connect_poses_counts()[0] > 0  # the decision's counters are this call's
    again = b.connect_poses(0, w.goals)
    for x, y in zip(first, again):
        assert np.array_equal(x, y)
    assert np.array_equal(again[0], w.vertex) and np.array_equal(again[1], w.cost)
    xyh, ids = b.pose_routes_rows(len(c.routes.rows))  # connect_poses leaves the rows and the points of the routes call alone
    assert np.array_equal(xyh, c.routes.rows) and np.array_equal(ids, c.routes.ids)
    assert np.array_equal(b.pose_routes_points(len(c.routes.points)).view(np.int64), c.routes.points.view(np.int64))
    b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    w = poseref.workload("E")
    c = prr.case("E")
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    L = _ffi.lib()
    refused_with_golden_text(GOLDEN, "no_plan", ctx.pose_routes, w.goals)
    s = _ffi.Batch(ctx, 1, w.n)
    refused_with_golden_text(GOLDEN, "non_dubins_batch", s.pose_routes, 0, w.goals)
    s.close()
    b = _ffi.Batch(ctx, 1, w.n, dubins=True)
    refused_with_golden_text(GOLDEN, "unfinished_query", b.pose_routes, 0, w.goals)
    refused_with_golden_text(GOLDEN, "rows_none", b.pose_routes_rows, 0)
    refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, 0)
    refused_with_golden_text(GOLDEN, "ms_none", b.pose_routes_ms)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    b.launch()
    b.sync()
    refused_with_golden_text(GOLDEN, "routes_on_a_dubins_batch", b.routes, 0, w.goals[:, :2])  # word for word what it was
    full = b.pose_routes(0, c.goals, points=True)
    prr.same(full, c.routes)
    rows, points = len(c.routes.rows), len(c.routes.points)
    refused_with_golden_text(GOLDEN, "rows_wrong_count", b.pose_routes_rows, rows + 1, asked=rows + 1, left=rows)
    refused_with_golden_text(GOLDEN, "points_wrong_count", b.pose_routes_points, points - 1, asked=points - 1, left=points)
    assert np.array_equal(b.pose_routes_rows(rows)[0], c.routes.rows)  # a wrong count drops nothing
    # a call without points leaves rows and no points
    b.pose_routes(0, c.goals)
    refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, points)
    # failed calls: each drops the rows and the points of the call before it
    g, vertex, cost = _ffi._pose_arrays(c.goals)
    m = len(g)
    length, offsets, po = np.zeros(m), np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    args = (vertex.ctypes.data, cost.ctypes.data, length.ctypes.data, offsets.ctypes.data)

    def raw(flags, point_offsets, poses=g):
        _ffi._check(ctx.handle, L.rrt_batch_pose_routes(b._h, 0, poses.ctypes.data, m, flags, *args, point_offsets))

    for key, call in (("unknown_flag", lambda: raw(2, po.ctypes.data)), ("null_point_offsets", lambda: raw(1, None))):
        b.pose_routes(0, c.goals, points=True)
        refused_with_golden_text(GOLDEN, key, call)
        refused_with_golden_text(GOLDEN, "rows_none", b.pose_routes_rows, rows)
        refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, points)
    raw(0, None)  # without the flag point_offsets may be NULL
    assert np.array_equal(offsets, c.routes.offsets)
    bad = g.copy()
    bad[1, 2] = w.nh
    b.pose_routes(0, c.goals, points=True)
    refused_with_golden_text(GOLDEN, "heading_out_of_range", lambda: raw(1, po.ctypes.data, bad), nh=w.nh)
    refused_with_golden_text(GOLDEN, "rows_none", b.pose_routes_rows, rows)
    # a rearm
    b.pose_routes(0, c.goals, points=True)
    b.rearm()
    refused_with_golden_text(GOLDEN, "rows_none", b.pose_routes_rows, rows)
    refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, points)
    b.launch()
    b.sync()
    prr.same(b.pose_routes(0, c.goals, points=True), c.routes)
    # the grid replaced by one of the same shape
    ctx2 = _ffi.Context(0)
    ctx2.set_grid(w.og8)
    b2 = _ffi.Batch(ctx2, 1, w.n, dubins=True)
    b2.set_query(0, q)
    b2.launch()
    b2.sync()
    ctx2.set_grid(posekeepref.blocks_map(w.og8, w.xs))
    refused_with_golden_text(GOLDEN, "grid_replaced", b2.pose_routes, 0, w.goals)
    b2.close()
    ctx2.close()
    b.close()
    ctx.close()


def test_the_straight_line_planners_refuse():
    w = poseref.workload("E")
    p = RRTStar(w.og, 50, 10, pbar=False)
    refused_with_golden_text(GOLDEN, "straight_line_planner", p.routes_to_poses, w.goals)
