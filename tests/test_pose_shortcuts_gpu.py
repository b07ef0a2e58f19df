"""GPU: routes to many goal poses shortened on the device (rrt_pose_route_cut_kernel, rrt_pose_route_pack_kernel,
rrt_batch_pose_shortcuts / rrt_plan_pose_shortcuts and their _ms companions, _ffi.Batch.pose_routes / Context.pose_routes with
shortcut=True, RRTDubins / RRTStarDubins .routes_to_poses(shortcut=True)).

Every comparison is exact: vertex, cost, length, offsets, rows, ids, point_offsets as integers or raw bits, and the points as raw
bits, by poseroutesref.same.  The check is poseshortref.py: the raw rows of poseroutesref, the greedy pass with the oracle's word and
poseref.sweep_free, lengths and points rebuilt with poseroutesref.leg.  What holds that restatement to the oracle's own cells, and what
the workloads exercise (routes shortened, blocked candidates, the second to fourth batch of 64 on the rings, a duplicate point on a
shortcut leg), is asserted without a GPU in test_pose_shortcuts_cpu.py.  The refusals' texts are
tests/golden/pose_shortcuts_refusals.json."""
import json
import os

import numpy as np
import pytest

import posegrowref
import poseref
import posekeepref
import poseroutesref as prr
import poseshortref as psr
from orchelp import bits
from posecalls import grow_poses_checked, planned_batch, planned_logged_batch, refused_with_golden_text
from rrtplanner_amd import RRTStar, _ffi

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_shortcuts_refusals.json")) as f:
    GOLDEN = json.load(f)


def _free_cells(og8, points):
    cells = np.floor(points + 0.5).astype(np.int64)
    assert np.all(og8[cells[:, 0], cells[:, 1]] == 0)


def _both(b, c, q=0, want=None):
    """with and without points against the case's shortened routes; every point rounds to a free cell of the active map"""
    want = psr.of_case(c) if want is None else want
    full = b.pose_routes(q, c.goals, points=True, shortcut=True)
    prr.same(full, want)
    _free_cells(c.og8, full[7])
    bare = b.pose_routes(q, c.goals, shortcut=True)
    prr.same(bare, want, points=False)
    return full


# ------------------------------------------------------------------------------------------------ 1. the workloads
@pytest.mark.parametrize("name", ["A", "B", "D", "E", "F", "G1", "G256"])
def test_workloads_on_a_batch(gpu_ctx, name):
    c = prr.case(name)
    b = planned_batch(gpu_ctx, c.w)
    _both(b, c)
    ms = b.pose_shortcuts_ms()
    assert len(ms) == 5 and all(t >= 0.0 for t in ms) and ms[4] == 0.0  # (the last call asked for no points)
    if name == "F":
        got = b.pose_routes(0, c.goals, points=True, shortcut=True)
        assert np.all(got[3] == 0) and np.all(got[6] == 0) and got[4].shape == (0, 3) and got[7].shape == (0, 2)
    b.close()


def test_the_one_sample_kernel_builds_the_same_tree(gpu_ctx):
    c = prr.case("E")
    b = planned_batch(gpu_ctx, c.w, serial=True)
    _both(b, c)
    b.close()


def test_workload_c_of_4000_vertices(gpu_ctx):
    c = prr.case("C")
    b = planned_batch(gpu_ctx, c.w)
    _both(b, c)
    b.close()


# ------------------------------------------------------------------------------------------------ 2. trees made for one purpose each
@pytest.mark.parametrize("name", ["small", "large"])
def test_rings_whose_anchors_meet_batches_of_blocked_candidates(gpu_ctx, name):
    c = psr.ring(name)
    b = planned_batch(gpu_ctx, c.w)
    _both(b, c)
    b.close()


def test_the_half_cell_chain_keeps_the_duplicate_point_of_a_shortcut_leg(gpu_ctx):
    c = prr.half_cell_chain()
    b = planned_batch(gpu_ctx, c.w)
    _both(b, c)
    b.close()


# ------------------------------------------------------------------------------------------------ 3. after a keep, and after a grow
@pytest.mark.parametrize("name", ["A", "C", "E"])
def test_after_keep_pose_tree(gpu_ctx, name):
    c = prr.kept_case(name)
    b = planned_batch(gpu_ctx, c.w)
    gpu_ctx.set_grid(c.og8)
    assert np.array_equal(b.keep_pose_tree(0), c.alive)
    _both(b, c)  # the sweeps on the new map, over the alive view, in the original vertex numbers
    b.close()


def test_after_grow_poses_in_the_new_numbering(gpu_ctx):
    k, s, _, _, _, g = posegrowref.planted("A")
    w = k.w
    b = planned_logged_batch(gpu_ctx, w, "block")
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive)
    grow_poses_checked(b, 0, w, g, g.ids, s, "block")
    v, cost, _ = poseref.connect(k.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    assert (v >= 0).sum() >= 4
    want = psr.routes(g.pts, g.head, g.parent, g.j, w.goals, v, cost, w.rho, w.nh, k.og8)
    assert psr.counts(want)[1] >= 1  # a route is shortened
    got = b.pose_routes(0, w.goals, points=True, shortcut=True)
    prr.same(got, want)
    _free_cells(k.og8, got[7])
    b.close()


def test_small_calls_after_a_large_one_on_the_same_batch(gpu_ctx):
    c = prr.case("E")
    prr.small_calls_after_a_large_one(lambda: planned_batch(gpu_ctx, c.w), c, psr.of_case(c), shortcut=True)


# ------------------------------------------------------------------------------------------------ 4. three queries, and the other ways in
def test_a_batch_of_three_queries_asked_at_the_second_and_the_third(gpu_ctx):
    c0, c1 = prr.case("E"), prr.kept_case("E")
    b = planned_logged_batch(gpu_ctx, c0.w, "block", Q=3)
    _both(b, c0, q=1)
    _both(b, c0, q=2)
    gpu_ctx.set_grid(c1.og8)
    assert np.array_equal(b.keep_pose_tree(2), c1.alive)
    _both(b, c1, q=2)
    b.close()


def test_through_rrt_plan(gpu_ctx):
    c = prr.case("A")
    w, want = c.w, psr.of_case(c)
    gpu_ctx.set_grid(w.og8)
    q, keep = poseref.device_query(w)
    rc, res = gpu_ctx.plan(q, w.n)
    assert rc == w.status and res.j == w.j
    prr.same(gpu_ctx.pose_routes(c.goals, points=True, shortcut=True), want)
    prr.same(gpu_ctx.pose_routes(c.goals, shortcut=True), want, points=False)
    assert len(gpu_ctx.pose_shortcuts_ms()) == 5


@pytest.mark.parametrize("name", ["A", "D"])  # RRTStarDubins, RRTDubins
def test_through_the_planners_with_an_open_heading(name):
    c = prr.case(name)
    w, r = c.w, psr.of_case(c)
    p = poseref.planner_of(w)
    p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j
    routes, length, paths = p.routes_to_poses(c.goals, points=True, shortcut=True)
    assert np.array_equal(length.view(np.int64), r.length.view(np.int64))
    for g in range(len(c.goals)):
        if r.vertex[g] < 0:
            assert routes[g] is None and paths[g] is None
            continue
        assert routes[g].dtype == np.int64 and np.array_equal(routes[g], r.route(g))
        assert np.array_equal(paths[g].view(np.int64), r.path(g).view(np.int64))
    routes2, length2 = p.routes_to_poses(c.goals, shortcut=True)
    assert np.array_equal(length2.view(np.int64), length.view(np.int64)) and all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(routes, routes2))
    # shortcut=False is the call it was
    plain, plain_length = p.routes_to_poses(c.goals)
    assert np.array_equal(plain_length.view(np.int64), c.routes.length.view(np.int64))
    assert all((a is None and c.routes.vertex[g] < 0) or np.array_equal(a, c.routes.route(g)) for g, a in enumerate(plain))
    # any arrival heading: the (cost, heading)-smallest connected pose of the cell, then its shortened route
    cells = [tuple(int(x) for x in c.goals[g][:2]) for g in (0, 1, w.i_obstacle)]
    want = [poseref.any_heading(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, cell, w.rho, w.nh) for cell in cells]
    assert want[0][0] >= 0 and want[2][0] == -1
    goals = np.array([(cell[0], cell[1], max(h, 0)) for cell, (_, _, h) in zip(cells, want)], dtype=np.int64)
    ref = psr.routes(w.ro.pts, w.ro.head, w.ro.parent, w.j, goals, [v for v, _, _ in want], [cst for _, cst, _ in want], w.rho, w.nh, w.og8)
    routes, length, paths = p.routes_to_poses([(cell[0], cell[1], -1) for cell in cells], points=True, shortcut=True)
    assert np.array_equal(length.view(np.int64), ref.length.view(np.int64))
    for g in range(3):
        if ref.vertex[g] < 0:
            assert routes[g] is None and paths[g] is None
        else:
            assert np.array_equal(routes[g], ref.route(g)) and np.array_equal(paths[g].view(np.int64), ref.path(g).view(np.int64))
    with pytest.raises(ValueError) as e:  # routes_to stays the refusal it is, with the keyword too
        p.routes_to(c.goals[:, :2], shortcut=True)
    assert str(e.value) == GOLDEN["dubins_planner_routes_to"][1]


# ------------------------------------------------------------------------------------------------ 5. twice, and the two calls in turn
def test_asked_twice_and_in_turn_with_the_plain_call(gpu_ctx):
    c = prr.case("B")
    raw, cut = c.routes, psr.of_case(c)
    assert len(cut.rows) < len(raw.rows) and len(cut.points) != len(raw.points)
    b = planned_batch(gpu_ctx, c.w)
    one = b.pose_routes(0, c.goals, points=True, shortcut=True)
    two = b.pose_routes(0, c.goals, points=True, shortcut=True)
    for x, y in zip(one, two):
        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y))
    prr.same(two, cut)
    cut_ms = b.pose_shortcuts_ms()
    assert len(cut_ms) == 5 and all(t >= 0.0 for t in cut_ms)
    # a plain call behind it: the read-back calls serve the plain rows and points, and the plain stage times are the plain call's
    prr.same(b.pose_routes(0, c.goals, points=True), raw)
    xyh, ids = b.pose_routes_rows(len(raw.rows))
    assert np.array_equal(xyh, raw.rows) and np.array_equal(ids, raw.ids)
    assert np.array_equal(b.pose_routes_points(len(raw.points)).view(np.int64), raw.points.view(np.int64))
    refused_with_golden_text(GOLDEN, "rows_wrong_count", b.pose_routes_rows, len(cut.rows), asked=len(cut.rows), left=len(raw.rows))
    plain_ms = b.pose_routes_ms()
    assert len(plain_ms) == 4 and all(t >= 0.0 for t in plain_ms)
    # ... and a shortcut call behind that one: its own rows and points; the plain stage times stay those of the plain call
    prr.same(b.pose_routes(0, c.goals, shortcut=True), cut, points=False)
    xyh, ids = b.pose_routes_rows(len(cut.rows))
    assert np.array_equal(xyh, cut.rows) and np.array_equal(ids, cut.ids)
    refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, len(cut.points))  # (that call asked for none)
    assert b.pose_routes_ms() == plain_ms and b.pose_shortcuts_ms()[4] == 0.0
    prr.same(b.pose_routes(0, c.goals, points=True, shortcut=True), cut)
    assert np.array_equal(b.pose_routes_points(len(cut.points)).view(np.int64), cut.points.view(np.int64))
    assert np.array_equal(b.connect_poses(0, c.w.goals)[0], c.w.vertex)  # the shared scratch answers connect_poses as before
    b.close()


# ------------------------------------------------------------------------------------------------ 6. the number of poses
def test_no_pose_one_pose_and_a_workgroup_of_them(gpu_ctx):
    c = prr.case("E")
    r = psr.of_case(c)
    g = int(np.argmax(np.diff(c.routes.offsets) - np.diff(r.offsets)))  # the pose whose route loses the most rows
    assert r.offsets[g + 1] - r.offsets[g] < c.routes.offsets[g + 1] - c.routes.offsets[g]
    b = planned_batch(gpu_ctx, c.w)
    got = b.pose_routes(0, np.zeros((0, 3), dtype=np.int32), points=True, shortcut=True)
    assert [len(x) for x in got] == [0, 0, 0, 1, 0, 0, 1, 0] and got[3][0] == 0 and got[6][0] == 0
    k, n = int(r.offsets[g + 1] - r.offsets[g]), int(r.point_offsets[g + 1] - r.point_offsets[g])
    for m in (1, 3, 4, 5, 257):  # a wavefront a pose: around a workgroup of four, and past a workgroup of the lane-per-pose kernels
        vertex, cost, length, offsets, rows, ids, point_offsets, points = b.pose_routes(0, np.tile(c.goals[g], (m, 1)), points=True, shortcut=True)
        assert np.all(vertex == r.vertex[g]) and np.all(cost.view(np.int64) == r.cost[g:g + 1].view(np.int64))
        assert np.all(length.view(np.int64) == r.length[g:g + 1].view(np.int64))
        assert np.array_equal(offsets, k * np.arange(m + 1)) and np.array_equal(point_offsets, n * np.arange(m + 1))
        assert np.array_equal(rows, np.tile(r.route(g), (m, 1))) and np.array_equal(ids, np.tile(r.ids[r.offsets[g]:r.offsets[g + 1]], m))
        assert np.array_equal(points.view(np.int64), np.tile(r.path(g), (m, 1)).view(np.int64))
    b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals
def test_refusals():
    c = prr.case("E")
    w, cut = c.w, psr.of_case(c)
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    L = _ffi.lib()
    refused_with_golden_text(GOLDEN, "no_plan", lambda: ctx.pose_routes(w.goals, shortcut=True))
    refused_with_golden_text(GOLDEN, "plan_ms_none", ctx.pose_shortcuts_ms)
    s = _ffi.Batch(ctx, 1, w.n)
    refused_with_golden_text(GOLDEN, "non_dubins_batch", lambda: s.pose_routes(0, w.goals, shortcut=True))
    s.close()
    b = _ffi.Batch(ctx, 1, w.n, dubins=True)
    refused_with_golden_text(GOLDEN, "unfinished_query", lambda: b.pose_routes(0, w.goals, shortcut=True))
    refused_with_golden_text(GOLDEN, "ms_none", b.pose_shortcuts_ms)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    b.launch()
    b.sync()
    b.pose_routes(0, c.goals, points=True)  # a plain call does not make stage times of the shortcut call
    refused_with_golden_text(GOLDEN, "ms_none", b.pose_shortcuts_ms)
    refused_with_golden_text(GOLDEN, "q_out_of_range", lambda: b.pose_routes(1, w.goals, shortcut=True))
    prr.same(b.pose_routes(0, c.goals, points=True, shortcut=True), cut)
    rows, points = len(cut.rows), len(cut.points)
    # failed calls: each drops the rows and the points of the call before it
    g, vertex, cost = _ffi._pose_arrays(c.goals)
    m = len(g)
    length, offsets, po = np.zeros(m), np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    args = (vertex.ctypes.data, cost.ctypes.data, length.ctypes.data, offsets.ctypes.data)

    def raw(flags, point_offsets, poses=g):
        _ffi._check(ctx.handle, L.rrt_batch_pose_shortcuts(b._h, 0, poses.ctypes.data, m, flags, *args, point_offsets))

    bad_h, bad_x = g.copy(), g.copy()
    bad_h[1, 2] = w.nh
    bad_x[0, :2] = (w.og8.shape[0], 0)
    for key, call, fmt in (("unknown_flag", lambda: raw(2, po.ctypes.data), {}), ("null_point_offsets", lambda: raw(1, None), {}),
                           ("heading_out_of_range", lambda: raw(1, po.ctypes.data, bad_h), dict(nh=w.nh)),
                           ("cell_outside", lambda: raw(1, po.ctypes.data, bad_x), dict(x=w.og8.shape[0], W=w.og8.shape[0], H=w.og8.shape[1]))):
        b.pose_routes(0, c.goals, points=True, shortcut=True)
        refused_with_golden_text(GOLDEN, key, call, **fmt)
        refused_with_golden_text(GOLDEN, "rows_none", b.pose_routes_rows, rows)
        refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, points)
    raw(0, None)  # without the flag point_offsets may be NULL
    assert np.array_equal(offsets, cut.offsets)
    # the plain call keeps its refusal of 0x2 with its own text: the shortcuts are not a flag of it
    with pytest.raises(_ffi.RRTError) as e:
        _ffi._check(ctx.handle, L.rrt_batch_pose_routes(b._h, 0, g.ctypes.data, m, 2, *args, po.ctypes.data))
    assert str(e.value) == "librrt_hip error -1: rrt_batch_pose_routes: flags=0x2, only RRT_POSE_ROUTES_POINTS is defined"
    # a rearm
    b.pose_routes(0, c.goals, points=True, shortcut=True)
    b.rearm()
    refused_with_golden_text(GOLDEN, "rows_none", b.pose_routes_rows, rows)
    refused_with_golden_text(GOLDEN, "points_none", b.pose_routes_points, points)
    b.launch()
    b.sync()
    prr.same(b.pose_routes(0, c.goals, points=True, shortcut=True), cut)
    # the grid replaced by one of the same shape
    ctx.set_grid(posekeepref.blocks_map(w.og8, w.xs))
    refused_with_golden_text(GOLDEN, "grid_replaced", lambda: b.pose_routes(0, w.goals, shortcut=True))
    b.close()
    ctx.close()


def test_the_straight_line_planners_refuse():
    w = poseref.workload("E")
    p = RRTStar(w.og, 50, 10, pbar=False)
    refused_with_golden_text(GOLDEN, "straight_line_planner", lambda: p.routes_to_poses(w.goals, shortcut=True))
