"""GPU: finished routes to many goals in one device call, with line-of-sight shortcuts (rrt_route_*_kernel, rrt_batch_routes /
rrt_batch_routes_rows / rrt_plan_routes / rrt_plan_routes_rows, _ffi.Batch.routes / Context.routes, RRT.routes_to).

Every comparison is exact (==, array_equal).  The one inequality, length <= cost * (1 + 1e-9), allows for rounding: a left-to-right
f64 sum can exceed the tree's own sum in the last bits, and 1e-9 is far above j * 2^-53 for any j the kernels take.  The check is routeref.py:
goalref's decision, the parent walk, every candidate of every anchor by the oracle's line walk, np.sqrt sums."""
import functools

import numpy as np
import pytest

import oracle
import routeref
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTStarDubins
from treecalls import corridor_map, free_goals, free_samples, march, plan_on_own_batch, refused_with_word, same_routes, wall_map

pytestmark = pytest.mark.gpu

INF = np.inf
def _wall_goals(og):
    """about 200 free goals, one in the closed box, some on obstacle cells"""
    return np.concatenate([free_goals(og, 197, 31), [[30, 130]], np.argwhere(og != 0)[::400][:6]])


@functools.lru_cache(maxsize=None)
def _planned(kind):
    """(planner, T, og8, (points, parent, vcosts, j), goals, reference raw, reference shortcut): one plan() and one pair of
    reference results per planner class, shared by the tests and left unchanged"""
    og = wall_map()
    p = {"std": lambda: amd.RRTStandard(og, 2000, pbar=False, seed=1), "star": lambda: amd.RRTStar(og, 2000, 30, pbar=False, seed=1),
         "informed": lambda: amd.RRTStarInformed(og, 2000, 30, 25, pbar=False, seed=1)}[kind]()
    T, gv = p.plan(np.array((5, 5)), np.array((190, 150)))
    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    og8 = oracle.og_u8(og)
    goals = _wall_goals(og)
    tree = (np.array(points), np.array(parent), np.array(vcosts), j)
    ref = [routeref.routes(og8, tree[0], tree[2], tree[1], j, goals, cut=cut) for cut in (False, True)]
    return p, T, og8, tree, goals, ref[0], ref[1]


# ------------------------------------------------------------------------------------------------ 1. raw routes
@pytest.mark.parametrize("kind", ["std", "star", "informed"])
def test_raw_routes_on_the_planners(kind):
    p, T, og8, (points, parent, vcosts, j), goals, want, _ = _planned(kind)
    got = p.device_context().routes(goals)
    same_routes(got, want)
    vertex, cost, length, offsets, xy, ids = got
    cv, cc = p.connect_goals(goals)
    assert np.array_equal(vertex, cv) and np.array_equal(cost, cc)
    assert offsets[0] == 0 and offsets[-1] == len(xy) == len(ids)
    none = vertex < 0
    assert none[197] and none[198:].all() and (~none).sum() >= 150  # the box, the obstacle cells
    assert np.all(np.diff(offsets)[none] == 0) and np.all(length[none] == INF) and np.all(np.isfinite(length[~none]))
    for g in np.flatnonzero(~none).tolist():
        route = p.route2gv(T, int(vertex[g]))
        lo, hi = offsets[g], offsets[g + 1]
        assert ids[lo:hi].tolist() == route + [-1]
        assert xy[lo:hi].tolist() == [points[u].tolist() for u in route] + [goals[g].tolist()]
    routes, length2 = p.routes_to(goals, shortcut=False)
    paths = p.paths_to(T, goals)
    assert np.array_equal(length2, length) and len(routes) == len(paths) == len(goals)
    for a, b in zip(routes, paths):
        assert (a is None and b is None) or (a.dtype == b.dtype == np.int64 and np.array_equal(a, b))
    if kind == "std":  # a vertex of RRTStandard costs its parent's cost plus the edge: the same sum in the same order
        assert np.array_equal(length[~none], cost[~none])


# ------------------------------------------------------------------------------------------------ 2. shortcuts
@pytest.mark.parametrize("kind", ["std", "star", "informed"])
def test_shortcut_routes_on_the_planners(kind):
    p, T, og8, (points, parent, vcosts, j), goals, raw, want = _planned(kind)
    # the reference result covers both outcomes before anything is asked of the device
    ok = want[0] >= 0
    shorter = ok & (np.diff(want[3]) < np.diff(raw[3]))
    same = ok & (np.diff(want[3]) == np.diff(raw[3]))
    print(kind, "connected", ok.sum(), "shorter", shorter.sum(), "unchanged", same.sum())
    assert shorter.sum() >= 100 and same.sum() >= 30
    assert np.all(want[2][shorter] < raw[2][shorter]) and np.array_equal(want[2][same], raw[2][same])
    got = p.device_context().routes(goals, shortcut=True)
    same_routes(got, want)
    vertex, cost, length, offsets, xy, ids = got
    assert np.array_equal(vertex, raw[0]) and np.array_equal(cost, raw[1])
    assert np.all(length[ok] <= cost[ok] * (1 + 1e-9)) and np.all(length[~ok] == INF)
    for g in np.flatnonzero(ok).tolist():
        pts, iv = xy[offsets[g]:offsets[g + 1]], ids[offsets[g]:offsets[g + 1]]
        assert iv[0] == 0 and iv[-1] == -1 and pts[-1].tolist() == goals[g].tolist()
        rid = raw[5][raw[3][g]:raw[3][g + 1]].tolist()
        at = [rid.index(i) for i in iv.tolist()]
        for a, b, pa, pb in zip(at[:-1], at[1:], pts[:-1], pts[1:]):
            assert b > a
            if b != a + 1:  # (a + 1 is a tree edge or the goal edge: taken untested)
                assert oracle.collisionfree(og8, pa, pb)[0]
    routes, length2 = p.routes_to(goals, shortcut=True)
    assert np.array_equal(length2, length)
    for g, r in enumerate(routes):
        assert (r is None) == (not ok[g])
        if r is not None:
            assert r.dtype == np.int64 and np.array_equal(r, xy[offsets[g]:offsets[g + 1]])


# ------------------------------------------------------------------------------------------------ 3. long routes
def test_routes_longer_than_a_workgroup_has_waves_and_a_wave_has_lanes(gpu_ctx):
    og, way = corridor_map()
    og8 = oracle.og_u8(og)
    samples = march(way)
    n = len(samples)
    goals = np.array([(190, 150), (100, 150), (30, 100), (110, 45), (190, 60), (70, 20), (5, 21), (0, 159)])
    st, ro = oracle.plan(og8, n, 0, way[0], (190, 150), samples, logs=False)
    raw, want = [routeref.routes(og8, ro.pts, ro.vcost, ro.parent, ro.j, goals, cut=cut) for cut in (False, True)]
    rows, kept = np.diff(raw[3]), np.diff(want[3])
    print("rows", rows.tolist(), "kept", kept.tolist())
    # on the oracle's tree, before anything is asked of the device: routes beyond 16 and 64 rows (here up to 191), which shortcuts
    # cut down a lot, and anchors whose winner lies beyond the first round of 16 candidates from the far end
    assert (rows > 64).sum() >= 4 and (rows > 16).sum() >= 5 and rows.max() > 128 and np.all(kept[rows > 64] * 4 < rows[rows > 64])
    beyond = 0
    for g in np.flatnonzero(rows > 64).tolist():
        rid = raw[5][raw[3][g]:raw[3][g + 1]].tolist()
        at = [rid.index(i) for i in want[5][want[3][g]:want[3][g + 1]].tolist()]
        beyond += sum(1 for b in at[1:] if rows[g] - 1 - b >= 16)
    assert beyond >= 20
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 0, n, way[0], (190, 150), samples)
    assert res.j == ro.j and np.array_equal(res.parent[:res.j], ro.parent[:ro.j]) and np.array_equal(res.pts[:res.j], ro.pts[:ro.j])
    same_routes(b.routes(0, goals), raw)
    same_routes(b.routes(0, goals, shortcut=True), want)
    same_routes(b.routes(0, goals), raw)  # (the shortcut pass rewrote its rows in place: the next call fills them again)
    b.close()


# ------------------------------------------------------------------------------------------------ 4. non-contiguous visibility
def test_the_largest_visible_row_wins_not_the_first_run_of_visible_ones(gpu_ctx):
    og8 = np.zeros((200, 160), dtype=np.uint8)
    og8[25:27, 0:41] = 1
    og8[0:101, 60:62] = 1
    s, A, B, C, g = (5, 50), (40, 50), (40, 20), (110, 30), (110, 80)
    samples = np.array([A, B, C, (0, 0)])  # (the last one is thrown away: with three samples the tree takes only s, A and B)
    gpu_ctx.set_grid(og8)
    st, ro = oracle.plan(og8, 4, 0, s, (199, 159), samples, logs=False)
    assert ro.j == 4 and ro.parent[:4].tolist() == [-1, 0, 1, 2]
    b, res = plan_on_own_batch(gpu_ctx, 0, 4, s, (199, 159), samples)
    assert res.parent[:4].tolist() == [-1, 0, 1, 2] and res.pts[:4].tolist() == [list(s), list(A), list(B), list(C)]
    raw = b.routes(0, [g])
    assert res.j == 4 and raw[0].tolist() == [3]
    assert raw[4].tolist() == [list(s), list(A), list(B), list(C), list(g)] and raw[5].tolist() == [0, 1, 2, 3, -1] and raw[3].tolist() == [0, 5]
    cut = b.routes(0, [g], shortcut=True)
    assert cut[0].tolist() == [3] and cut[1][0] == raw[1][0]
    assert cut[4].tolist() == [list(s), list(C), list(g)] and cut[5].tolist() == [0, 3, -1] and cut[3].tolist() == [0, 3]
    assert cut[2][0] == float(np.sqrt(np.float64(105 * 105 + 20 * 20)) + np.sqrt(np.float64(2500))) < raw[2][0]
    same_routes(cut, routeref.routes(og8, res.pts, res.vcost, res.parent, res.j, [g], cut=True))
    b.close()


# ------------------------------------------------------------------------------------------------ 5. bookkeeping
def test_more_goals_than_workgroups(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 1, 600, (5, 5), (190, 150), free_samples(og, 600, 4), r2=hostprep.radius_threshold(30))
    goals = np.concatenate([free_goals(og, 1480, 5), np.argwhere(og != 0)[::45][:20]])
    assert len(goals) == 1500
    for cut in (False, True):
        want = routeref.routes(og8, res.pts, res.vcost, res.parent, res.j, goals, cut=cut)
        same_routes(b.routes(0, goals, shortcut=cut), want)
        # the first m goals, m around one pass of the scan of the row counts (1024 values): a goal's route does not depend on the
        # other goals, so the reference is the front of the one above
        vertex, cost, length, offsets, xy, ids = want
        for m in (1023, 1024, 1025):
            rows = offsets[m]
            assert vertex[m - 1] >= 0 and rows > offsets[m - 1]  # (the goal at the edge has rows)
            same_routes(b.routes(0, goals[:m], shortcut=cut), (vertex[:m], cost[:m], length[:m], offsets[:m + 1], xy[:rows], ids[:rows]))
    b.close()


def test_no_goals_and_one_goal(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 0, 300, (5, 5), (190, 150), free_samples(og, 300, 4))
    for cut in (False, True):
        vertex, cost, length, offsets, xy, ids = b.routes(0, np.zeros((0, 2), dtype=np.int64), shortcut=cut)
        assert vertex.shape == cost.shape == length.shape == ids.shape == (0,) and offsets.tolist() == [0] and xy.shape == (0, 2)
        # the start itself: the root and the goal, two rows of the same point, no leg to test
        got = b.routes(0, (5, 5), shortcut=cut)
        assert got[0].tolist() == [0] and got[2].tolist() == [0.0] and got[4].tolist() == [[5, 5], [5, 5]] and got[5].tolist() == [0, -1]
        # a goal nothing sees, alone: no rows at all
        got = b.routes(0, [(30, 130)], shortcut=cut)
        assert got[0].tolist() == [-1] and got[2].tolist() == [INF] and got[3].tolist() == [0, 0] and got[4].shape == (0, 2)
    b.close()


def test_a_batch_of_three_queries(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    ns = [300, 1500, 800]
    b = _ffi.Batch(gpu_ctx, 3, max(ns))
    keeps = []
    for q, n in enumerate(ns):
        qu, keep = _ffi.make_query(1, n, (5 + q, 5), (190, 150 - q), free_samples(og, n, 10 + q), r2_rewire=hostprep.radius_threshold(25))
        keeps.append(keep)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    goals = free_goals(og, 60, 13)
    res = b.get_result(1)
    assert res.pts[0].tolist() == [6, 5]
    for cut in (False, True):
        same_routes(b.routes(1, goals, shortcut=cut), routeref.routes(og8, res.pts, res.vcost, res.parent, res.j, goals, cut=cut))
    b.close()


def test_large_grid_batch_on_a_small_grid():
    og = wall_map()
    og8 = oracle.og_u8(og)
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    b, res = plan_on_own_batch(ctx, 1, 1500, (5, 5), (190, 150), free_samples(og, 1500, 14), r2=hostprep.radius_threshold(30), large_grid=True)
    assert b.kernel_name() == "rrt_pipe_large_kernel" and res.j > 500
    goals = np.concatenate([free_goals(og, 80, 22), [[30, 130]]])
    raw, want = [routeref.routes(og8, res.pts, res.vcost, res.parent, res.j, goals, cut=cut) for cut in (False, True)]
    assert (np.diff(want[3]) < np.diff(raw[3])).sum() >= 20
    same_routes(b.routes(0, goals), raw)
    same_routes(b.routes(0, goals, shortcut=True), want)
    b.close()
    ctx.close()


def test_connect_goals_is_what_it_was_and_rows_go_with_their_call(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 1, 1000, (5, 5), (190, 150), free_samples(og, 1000, 15), r2=hostprep.radius_threshold(25))
    goals = free_goals(og, 300, 16)
    refused_with_word(_ffi.RRT_E_ARG, "no routes", b.routes_rows, 0)
    before = b.connect_goals(0, goals)
    got = b.routes(0, goals, shortcut=True)
    after = b.connect_goals(0, goals[:40])  # (fewer goals: the routes' rows stay those of the 300)
    assert np.array_equal(before[0], got[0]) and np.array_equal(before[1], got[1])
    assert np.array_equal(before[0][:40], after[0]) and np.array_equal(before[1][:40], after[1])
    rows = int(got[3][-1])
    xy, ids = b.routes_rows(rows)
    assert np.array_equal(xy, got[4]) and np.array_equal(ids, got[5])
    refused_with_word(_ffi.RRT_E_ARG, "rows=", b.routes_rows, rows - 1)
    refused_with_word(_ffi.RRT_E_ARG, "rows=", b.routes_rows, rows + 1)
    b.rearm()
    refused_with_word(_ffi.RRT_E_ARG, "no routes", b.routes_rows, rows)
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.routes, 0, goals)
    b.launch()
    refused_with_word(_ffi.RRT_E_ARG, "no routes", b.routes_rows, rows)
    b.sync()
    refused_with_word(_ffi.RRT_E_ARG, "no routes", b.routes_rows, rows)
    same_routes(b.routes(0, goals, shortcut=True), got)
    # a call that is refused leaves no rows behind either
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.routes, 0, [(200, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "no routes", b.routes_rows, rows)
    b.close()


@pytest.mark.parametrize("cut", [False, True])
def test_small_calls_after_a_large_one_on_the_same_batch(gpu_ctx, cut):
    """scratch that was allocated for a large call serves a small one: 257 goals, the goal with the longest route tiled, then that
    goal alone and three different goals, their rows read back through routes_rows"""
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)

    def run():
        return plan_on_own_batch(gpu_ctx, 1, 1000, (5, 5), (190, 150), free_samples(og, 1000, 15), r2=hostprep.radius_threshold(25))

    b, res = run()
    goals = free_goals(og, 60, 16)
    want = routeref.routes(og8, res.pts, res.vcost, res.parent, res.j, goals, cut=cut)
    by_rows = np.argsort(-np.diff(want[3]), kind="stable")
    g = int(by_rows[0])
    three = [int(by_rows[1]), g, int(by_rows[2])]
    k = int(want[3][g + 1] - want[3][g])
    assert k >= 3 and len({tuple(goals[i]) for i in three}) == 3 and np.diff(want[3])[three].sum() < 257 * k
    large = b.routes(0, np.tile(goals[g], (257, 1)), shortcut=cut)
    assert np.array_equal(large[3], k * np.arange(258))
    for sel in ([g], three):
        got = b.routes(0, goals[sel], shortcut=cut)
        xy, ids = b.routes_rows(int(got[3][-1]))
        assert np.array_equal(xy, got[4]) and np.array_equal(ids, got[5])
        got = got[:4] + (xy, ids)
        same_routes(got, routeref.routes(og8, res.pts, res.vcost, res.parent, res.j, goals[sel], cut=cut))
        f, _ = run()  # a batch that made no call before this one
        same_routes(got, f.routes(0, goals[sel], shortcut=cut))
        f.close()
    b.close()


def test_refusals():
    ctx = _ffi.Context(0)
    og = wall_map()
    ctx.set_grid(oracle.og_u8(og))
    L = _ffi.lib()
    refused_with_word(_ffi.RRT_E_ARG, "no rrt_plan", ctx.routes, [(5, 5)])
    samples = free_samples(og, 500, 17)
    b = _ffi.Batch(ctx, 2, 500)
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.routes, 0, [(5, 5)])
    q, keep = _ffi.make_query(1, 500, (5, 5), (190, 150), samples, r2_rewire=900)
    b.set_query(0, q)
    refused_with_word(_ffi.RRT_E_ARG, "not launched", b.routes, 0, [(5, 5)])
    b.launch()
    b.sync()
    want = b.routes(0, [(150, 150)], shortcut=True)
    refused_with_word(_ffi.RRT_E_ARG, "q=2", b.routes, 2, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "q=-1", b.routes, -1, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.routes, 1, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.routes, 0, [(5, 5), (200, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.routes, 0, [(5, -1)])
    refused_with_word(_ffi.RRT_E_ARG, "at most", b.routes, 0, np.zeros(((1 << 20) + 1, 2), dtype=np.int32))
    # the C calls themselves: NULL arguments, an unknown flag
    g = np.array([[150, 150]], dtype=np.int32)
    v, c, ln, off = np.zeros(1, np.int32), np.zeros(1), np.zeros(1), np.zeros(2, np.int64)
    args = [g.ctypes.data, 1, 0, v.ctypes.data, c.ctypes.data, ln.ctypes.data, off.ctypes.data]
    assert L.rrt_batch_routes(None, 0, *args) == _ffi.RRT_E_ARG
    for k in (0, 3, 4, 5, 6):
        assert L.rrt_batch_routes(b._h, 0, *[None if i == k else a for i, a in enumerate(args)]) == _ffi.RRT_E_ARG, k
    assert L.rrt_batch_routes(b._h, 0, *[2 if i == 2 else a for i, a in enumerate(args)]) == _ffi.RRT_E_ARG
    assert L.rrt_batch_routes_rows(None, None, None, 0) == _ffi.RRT_E_ARG and L.rrt_plan_routes_rows(None, None, None, 0) == _ffi.RRT_E_ARG
    assert L.rrt_plan_routes(None, *args) == _ffi.RRT_E_ARG
    assert L.rrt_batch_routes(b._h, 0, *args) == _ffi.RRT_OK and off.tolist() == [0, int(np.diff(b.routes(0, [(150, 150)])[3])[0])]
    assert L.rrt_batch_routes_rows(b._h, None, None, int(off[1])) == _ffi.RRT_E_ARG
    b.rearm()
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.routes, 0, [(5, 5)])
    b.launch()
    b.sync()
    # the grid replaced between run and call: same shape, another generation
    ctx.set_grid(oracle.og_u8(og))
    refused_with_word(_ffi.RRT_E_ARG, "replaced", b.routes, 0, [(150, 150)])
    b.rearm()
    b.launch()
    b.sync()
    same_routes(b.routes(0, [(150, 150)], shortcut=True), want)
    ctx.set_grid(np.zeros((64, 64), dtype=np.uint8))
    refused_with_word(_ffi.RRT_E_ARG, "shape", b.routes, 0, [(5, 5)])
    b.close()
    # an Informed query that reached the goal region waits for its unit ball
    b = _ffi.Batch(ctx, 1, 300)
    free = np.argwhere(np.zeros((64, 64)) == 0)
    s = hostprep.draw_free_samples(np.random.default_rng(18), free, 300)
    q, keep = _ffi.make_query(2, 300, (5, 5), (40, 40), s, r2_rewire=400, goal_d2=900, Cmat=hostprep.rotation_to_world_frame(np.array((5, 5)), np.array((40, 40))))
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert b.get_result(0).status == _ffi.RRT_NEED_UNITBALL
    refused_with_word(_ffi.RRT_E_ARG, "unit-ball", b.routes, 0, [(5, 5)])
    b.close()
    # a Dubins batch
    hd = np.random.default_rng(19).integers(0, 16, size=300)
    b = _ffi.Batch(ctx, 1, 300, dubins=True)
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR, 300, (5, 5, 0), (40, 40, 3), s, r2_rewire=400, headings=hd, rho=3.0, nh=16)
    b.set_query(0, q)
    b.launch()
    b.sync()
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "Dubins", b.routes, 0, [(5, 5)])
    b.close()
    ctx.close()
    with pytest.raises(ValueError, match="Dubins"):
        RRTStarDubins(np.zeros((64, 64), dtype=int), 100, 20, 3.0, pbar=False).routes_to([(5, 5)])


def test_the_planner_keeps_its_state_rules():
    p, T, og8, tree, goals, raw, want = _planned("std")
    q = amd.RRTStandard(wall_map(), 500, pbar=False, seed=3)
    with pytest.raises(RuntimeError, match="plan"):
        q.routes_to(goals)
    q.plan(np.array((5, 5)), np.array((190, 150)))
    routes, length = q.routes_to([(150, 150), (30, 130)], shortcut=True)
    assert routes[1] is None and length[1] == INF and routes[0][0].tolist() == [5, 5] and routes[0][-1].tolist() == [150, 150]
    assert q.routes_to(np.zeros((0, 2), dtype=np.int64))[0] == []
    with pytest.raises(ValueError, match="outside"):
        q.routes_to([(200, 0)])
    q.set_n(500)
    with pytest.raises(RuntimeError, match="plan"):
        q.routes_to(goals, shortcut=True)
