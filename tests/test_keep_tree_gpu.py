"""GPU: a finished tree kept when the map changes (rrt_keep_*_kernel, rrt_batch_keep_tree / rrt_plan_keep_tree, _ffi.Batch.keep_tree /
Context.keep_tree, RRT.keep_tree / RRT.keep_tree_resident), and the goals and routes calls over the view it installs.

Every comparison is exact (==, array_equal).  The check is keepref.py: every edge by the oracle's literal line walk from the parent
to the child, every vertex by its own walk to the root, then goalref / routeref on the alive vertices alone against the new map."""
import numpy as np
import pytest

import goalref
import keepref
import oracle
import routeref
import treecalls as tc
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.oggen import DeviceGrids, perlin_occupancygrid, random_connected_pair

pytestmark = pytest.mark.gpu

INF = np.inf
XS, XG = np.array((5, 5)), np.array((190, 150))


def _new_map(og):
    """the wall map of the goals tests after the change: a wall segment across the corridor between the two walls, which the tree
    uses on its way to the right third; a piece of the second wall and a piece of the closed box removed"""
    o = og.copy()
    o[70:133, 80:83] = 1
    o[133:136, 100:112] = 0
    o[20:41, 128:132] = 0
    return o


def _goals(og2):
    """free goals of the new map, one in the box that was closed, some on obstacle cells"""
    return np.concatenate([tc.free_goals(og2, 57, 31), [[30, 130]], np.argwhere(og2 != 0)[::400][:4]])


def _tree(p, T):
    _, points, parent, vcosts = T.__dict__["_lazy"]
    return np.array(points), np.array(parent), np.array(vcosts), p.last_stats["j"]


def _planner(kind, og, n=2000, seed=1):
    return {"std": lambda: amd.RRTStandard(og, n, pbar=False, seed=seed), "star": lambda: amd.RRTStar(og, n, 30, pbar=False, seed=seed),
            "informed": lambda: amd.RRTStarInformed(og, n, 30, 25, pbar=False, seed=seed),
            "correct": lambda: amd.RRTStar(og, n, 30, pbar=False, seed=seed, rewire="correct")}[kind]()


def _check_planner(p, T, og2, goals):
    """keep_tree(og2) on a planner that has planned, and every call over the view, against keepref on the tree T holds.
    Returns (alive, raw reference, shortcut reference)"""
    pts, parent, vcost, j = _tree(p, T)
    og28 = oracle.og_u8(og2)
    want_alive, raw = keepref.routes(og28, pts, parent, vcost, j, goals)
    _, cut = keepref.routes(og28, pts, parent, vcost, j, goals, cut=True)
    alive = p.keep_tree(og2)
    assert alive.dtype == bool and alive.shape == (j,)
    assert np.array_equal(alive, want_alive), np.flatnonzero(alive != want_alive)[:8]
    v, c = p.connect_goals(goals)
    assert np.array_equal(v, raw[0]) and np.array_equal(c, raw[1])
    tc.same_routes(p.device_context().routes(goals), raw)
    tc.same_routes(p.device_context().routes(goals, shortcut=True), cut)
    tc.same_routes(p.device_context().routes(goals), raw)
    routes, length = p.routes_to(goals, shortcut=True)
    assert np.array_equal(length, cut[2])
    paths = p.paths_to(T, goals)  # the parent walks on the T the caller holds: the vertex numbers are the original ones
    for g, path in enumerate(paths):
        lo, hi = raw[3][g], raw[3][g + 1]
        assert (path is None and lo == hi) or np.array_equal(path, raw[4][lo:hi])
        if path is not None:
            assert p.route2gv(T, int(v[g])) == raw[5][lo:hi - 1].tolist() and alive[raw[5][lo:hi - 1]].all()
    return alive, raw, cut


# ------------------------------------------------------------------------------------------------ 1. the planner classes
@pytest.mark.parametrize("kind", ["std", "star", "informed"])
def test_the_planners_keep_their_tree_on_a_changed_map(kind):
    og = tc.wall_map()
    og2 = _new_map(og)
    goals = _goals(og2)
    p = _planner(kind, og)
    T, gv = p.plan(XS, XG)
    pts, parent, vcost, j = _tree(p, T)
    assert j > 64 and j % 64 != 0 and j % 256 != 0
    v0, c0 = p.connect_goals(goals)
    alive, raw, cut = _check_planner(p, T, og2, goals)
    # the case is not trivial, on the host check alone
    v = raw[0]
    legs = np.abs(pts[1:j] - pts[parent[1:j]]).max(axis=1)
    print(kind, "j", j, "cut", int((~alive).sum()), "moved", int(((v != v0) & (v >= 0) & (v0 >= 0)).sum()), "new", int(((v0 < 0) & (v >= 0)).sum()),
          "edges beyond 64 cells", int((legs > 64).sum()))
    assert 0.05 * j <= (~alive).sum() <= 0.95 * j
    assert ((v != v0) & (v >= 0) & (v0 >= 0)).any() and ((v0 < 0) & (v >= 0)).any() and v0[57] == -1 and v[57] >= 0  # (57: the box)
    assert (legs > 64).any()
    assert np.array_equal(p.og, og2) and p._tree_resident == "device"
    # the tree itself is what it was: a new keep starts from all of it (8. has the answers)
    assert np.array_equal(p.keep_tree(og), np.ones(j, dtype=bool))


# ------------------------------------------------------------------------------------------------ 2. an unchanged map
def test_an_unchanged_map_keeps_every_vertex_of_a_reference_mode_tree():
    og = tc.wall_map()
    goals = _goals(_new_map(og))
    p = _planner("star", og, n=1200, seed=2)
    T, gv = p.plan(XS, XG)
    ctx = p.device_context()
    before = [p.connect_goals(goals), ctx.routes(goals), ctx.routes(goals, shortcut=True)]
    alive = p.keep_tree(og.copy())
    assert alive.all() and len(alive) == p.last_stats["j"]
    after = [p.connect_goals(goals), ctx.routes(goals), ctx.routes(goals, shortcut=True)]
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert x.dtype == y.dtype and np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 3. the root blocked
def test_a_blocked_root_leaves_nothing():
    og = tc.wall_map()
    p = _planner("star", og, n=600, seed=3)
    T, gv = p.plan(XS, XG)
    og2 = og.copy()
    og2[5, 5] = 1
    goals = np.array([(5, 5), (6, 6), (150, 150), (30, 130)])
    alive = p.keep_tree(og2)
    assert not alive.any() and len(alive) == p.last_stats["j"]
    v, c = p.connect_goals(goals)
    assert v.tolist() == [-1] * 4 and np.all(c == INF)
    for cut in (False, True):
        vertex, cost, length, offsets, xy, ids = p.device_context().routes(goals, shortcut=cut)
        assert vertex.tolist() == [-1] * 4 and np.all(cost == INF) and np.all(length == INF) and offsets.tolist() == [0] * 5 and len(xy) == len(ids) == 0
        routes, length = p.routes_to(goals, shortcut=cut)
        assert routes == [None] * 4 and np.all(length == INF)
    assert p.paths_to(T, goals) == [None] * 4


# ------------------------------------------------------------------------------------------------ 4. a deep tree
def test_a_chain_deeper_than_128_edges_is_cut_near_its_start(gpu_ctx):
    og, way = tc.corridor_map()
    og8 = oracle.og_u8(og)
    samples = tc.march(way)
    n = len(samples)
    gpu_ctx.set_grid(og8)
    b, res = tc.plan_on_own_batch(gpu_ctx, 0, n, way[0], (190, 150), samples)
    j = res.j
    depth = keepref.depth(res.parent, j)
    assert depth.max() >= 129  # 8 or more doubling rounds
    deepest = [int(np.argmax(depth))]
    while deepest[-1] != 0:
        deepest.append(int(res.parent[deepest[-1]]))
    hit = deepest[-6]  # the fifth vertex of the longest chain: its cell becomes an obstacle
    og2 = og8.copy()
    og2[res.pts[hit][0], res.pts[hit][1]] = 1
    gpu_ctx.set_grid(og2)
    alive = b.keep_tree(0)
    want = keepref.alive(og2, res.pts, res.parent, j)
    assert np.array_equal(alive, want) and not alive[hit] and 0 < alive.sum() < 16 and not alive[depth >= 129].any()
    # ... and the other way round: the whole chain alive needs every round
    gpu_ctx.set_grid(og8)
    assert b.keep_tree(0).all()
    goals = np.array([(190, 150), (100, 150), (30, 100), (5, 21)])
    tc.same_routes(b.routes(0, goals, shortcut=True), routeref.routes(og8, res.pts, res.vcost, res.parent, j, goals, cut=True))
    b.close()


# ------------------------------------------------------------------------------------------------ 5. parents with higher indices
def test_a_rewired_tree_whose_parents_come_after_their_children():
    og = tc.wall_map()
    og2 = _new_map(og)
    goals = _goals(og2)
    p = _planner("correct", og)
    T, gv = p.plan(XS, XG)
    pts, parent, vcost, j = _tree(p, T)
    assert (parent[1:j] > np.arange(1, j)).sum() > 100
    alive, raw, cut = _check_planner(p, T, og2, goals)
    assert 0.05 * j <= (~alive).sum() <= 0.95 * j
    # the unchanged map: the rewire tested its edges from the child's side, this walk goes from the parent's -- whatever that
    # cuts, it is what the host check cuts
    alive0, _, _ = _check_planner(p, T, og, goals)
    assert alive0.sum() >= j - 16


# ------------------------------------------------------------------------------------------------ 6. a large grid
def test_a_tree_of_the_large_grid_kernel():
    W, H = 2304, 48
    og = np.zeros((W, H), dtype=np.int64)
    og[700:704, :36] = 1
    og[1500:1504, 12:] = 1
    og2 = og.copy()
    og2[1100:1103, 10:] = 1         # a wall added
    og2[1500:1504, 30:40] = 0
    goals = tc.free_goals(og2, 30, 5)
    p = amd.RRTStar(og, 1500, 60, pbar=False, seed=3)
    T, gv = p.plan(np.array((5, 5)), np.array((2290, 40)))
    assert p.last_route == "kernel-large"
    pts, parent, vcost, j = _tree(p, T)
    legs = np.abs(pts[1:j] - pts[parent[1:j]]).max(axis=1)
    assert (legs > 256).any()  # more than one group of four ballot steps
    v0, c0 = p.connect_goals(goals)
    alive, raw, cut = _check_planner(p, T, og2, goals)
    assert 0.05 * j <= (~alive).sum() <= 0.95 * j and (raw[0] != v0).any()


# ------------------------------------------------------------------------------------------------ 7. a batch of three queries
def test_one_query_of_a_batch_is_kept_and_the_others_stay_refused(gpu_ctx):
    og = tc.wall_map()
    og8, og28 = oracle.og_u8(og), oracle.og_u8(_new_map(og))
    gpu_ctx.set_grid(og8)
    ns = [300, 1500, 800]
    b = _ffi.Batch(gpu_ctx, 3, max(ns))
    keeps = []
    for q, n in enumerate(ns):
        qu, keep = _ffi.make_query(1, n, (5 + q, 5), (190, 150 - q), tc.free_samples(og, n, 10 + q), r2_rewire=hostprep.radius_threshold(25))
        keeps.append(keep)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    goals = tc.free_goals(_new_map(og), 40, 13)
    res = [b.get_result(q) for q in range(3)]
    first = b.routes(1, goals, shortcut=True)
    gpu_ctx.set_grid(og28)
    for q in range(3):
        tc.refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_goals, q, goals)
    alive = b.keep_tree(1)
    want_alive, want = keepref.routes(og28, res[1].pts, res[1].parent, res[1].vcost, res[1].j, goals, cut=True)
    assert np.array_equal(alive, want_alive) and 0 < alive.sum() < res[1].j
    tc.same_routes(b.routes(1, goals, shortcut=True), want)
    v, c = b.connect_goals(1, goals)
    assert np.array_equal(v, want[0]) and np.array_equal(c, want[1])
    ms = b.keep_tree_ms()
    assert len(ms) == 3 and all(t >= 0.0 for t in ms)
    for q in (0, 2):
        tc.refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_goals, q, goals)
        tc.refused_with_word(_ffi.RRT_E_ARG, "replaced", b.routes, q, goals)
    for q in range(3):  # the tree arrays are untouched
        again = b.get_result(q)
        assert again.j == res[q].j and again.vgoal == res[q].vgoal and again.found == res[q].found
        for name in ("pts", "vcost", "parent"):
            assert np.array_equal(getattr(again, name), getattr(res[q], name))
    # a second query kept next to the first: each has its own view
    alive2 = b.keep_tree(2)
    assert np.array_equal(alive2, keepref.alive(og28, res[2].pts, res[2].parent, res[2].j))
    tc.same_routes(b.routes(1, goals, shortcut=True), want)
    tc.same_routes(b.routes(2, goals), keepref.routes(og28, res[2].pts, res[2].parent, res[2].vcost, res[2].j, goals)[1])
    # rearm + launch drop the views: the queries run again, on the new map, and answer over their whole new trees
    b.rearm()
    tc.refused_with_word(_ffi.RRT_E_ARG, "not finished", b.keep_tree, 1)
    b.launch()
    b.sync()
    new = b.get_result(1)
    tc.same_routes(b.routes(1, goals, shortcut=True), routeref.routes(og28, new.pts, new.vcost, new.parent, new.j, goals, cut=True))
    gpu_ctx.set_grid(og8)
    b.rearm()
    b.launch()
    b.sync()
    tc.same_routes(b.routes(1, goals, shortcut=True), first)
    b.close()


def test_a_refused_set_query_leaves_a_kept_query_on_its_view(gpu_ctx):
    """A set_query that is refused replaces nothing: the query keeps its view and goes on answering over the alive vertices alone,
    never over its whole tree on the grid that cut it.  The same through rrt_plan, which reaches set_query on the context's own
    batch.  A set_query that is accepted drops the view with the tree."""
    og = tc.wall_map()
    og8, og28 = oracle.og_u8(og), oracle.og_u8(_new_map(og))
    goals = tc.free_goals(_new_map(og), 40, 13)
    n = 1500
    samples = tc.free_samples(og, n, 11)
    r2 = hostprep.radius_threshold(25)
    gpu_ctx.set_grid(og8)
    b, res = tc.plan_on_own_batch(gpu_ctx, 1, n, (5, 5), (190, 150), samples, r2=r2)
    gpu_ctx.set_grid(og28)
    alive = b.keep_tree(0)
    want_alive, want = keepref.routes(og28, res.pts, res.parent, res.vcost, res.j, goals, cut=True)
    assert np.array_equal(alive, want_alive) and 0 < alive.sum() < res.j
    whole = routeref.routes(og28, res.pts, res.vcost, res.parent, res.j, goals, cut=True)
    assert not np.array_equal(whole[0], want[0])  # (answering from the whole tree would show)
    too_many, keep1 = _ffi.make_query(1, n + 1, (5, 5), (190, 150), tc.free_samples(og, n + 1, 12), r2_rewire=r2)
    bad_alg, keep2 = _ffi.make_query(1, n, (5, 5), (190, 150), samples, r2_rewire=r2)
    bad_alg.alg = -1
    outside, keep3 = _ffi.make_query(1, n, (5, 5), (og.shape[0], 150), samples, r2_rewire=r2)
    for qu, word in ((too_many, "capacity"), (bad_alg, "alg=-1"), (outside, "outside")):
        tc.refused_with_word(_ffi.RRT_E_ARG, word, b.set_query, 0, qu)
        tc.same_routes(b.routes(0, goals, shortcut=True), want)
        v, c = b.connect_goals(0, goals)
        assert np.array_equal(v, want[0]) and np.array_equal(c, want[1])
    good, keep4 = _ffi.make_query(1, n, (5, 5), (190, 150), samples, r2_rewire=r2)
    b.set_query(0, good)
    tc.refused_with_word(_ffi.RRT_E_ARG, "not launched", b.connect_goals, 0, goals)
    b.close()
    # the context's own batch
    gpu_ctx.set_grid(og8)
    rc, r1 = gpu_ctx.plan(good, n)
    size = _ffi.C.c_int32(-1)
    assert _ffi.lib().rrt_plan_tree_size(gpu_ctx.handle, _ffi.C.byref(size)) == _ffi.RRT_OK and size.value == r1.j
    gpu_ctx.set_grid(og28)
    alive = gpu_ctx.keep_tree()
    want_alive, want = keepref.routes(og28, r1.pts, r1.parent, r1.vcost, r1.j, goals, cut=True)
    assert np.array_equal(alive, want_alive) and 0 < alive.sum() < r1.j
    tc.refused_with_word(_ffi.RRT_E_ARG, "alg=-1", gpu_ctx.plan, bad_alg, n)
    tc.same_routes(gpu_ctx.routes(goals, shortcut=True), want)
    v, c = gpu_ctx.connect_goals(goals)
    assert np.array_equal(v, want[0]) and np.array_equal(c, want[1])


# ------------------------------------------------------------------------------------------------ 8. back to the first map
def test_keeping_the_tree_for_the_first_map_again_restores_every_answer():
    og = tc.wall_map()
    og2 = _new_map(og)
    goals = _goals(og2)
    p = _planner("star", og, n=1000, seed=4)
    T, gv = p.plan(XS, XG)
    ctx = p.device_context()
    first = [p.connect_goals(goals), ctx.routes(goals), ctx.routes(goals, shortcut=True)]
    cut1 = p.keep_tree(og2)
    changed = ctx.routes(goals)
    assert not cut1.all() and not np.array_equal(changed[0], first[1][0])
    assert p.keep_tree(og).all()
    again = [p.connect_goals(goals), ctx.routes(goals), ctx.routes(goals, shortcut=True)]
    for a, b in zip(first, again):
        for x, y in zip(a, b):
            assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(p.keep_tree(og2), cut1)  # not cumulative in either direction
    tc.same_routes(ctx.routes(goals), changed)
    # a later plan() plans on the map that was kept last
    q = _planner("star", og2, n=1000, seed=4)
    q.rand_gen = np.random.default_rng(4)
    p.rand_gen = np.random.default_rng(4)
    Tp, Tq = p.plan(XS, XG)[0], q.plan(XS, XG)[0]
    for x, y in zip(_tree(p, Tp)[:3], _tree(q, Tq)[:3]):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 9. resident frames
def test_keep_tree_resident_on_the_next_frame():
    frames = perlin_occupancygrid(128, 128, thresh=0.33, frames=2, seed=5)
    xs, xg = random_connected_pair(frames[0], np.random.default_rng(2))
    p = amd.RRTStar(frames[0], 900, 24, pbar=False, seed=3)
    grids = DeviceGrids(p.device_context(), 128, 128, thresh=0.33, frames=2, seed=5)
    assert np.array_equal(grids.host, frames)
    p.set_og_resident(grids, 0)
    T, gv = p.plan(xs, xg)
    pts, parent, vcost, j = _tree(p, T)
    goals = tc.free_goals(frames[1], 40, 6)
    og28 = oracle.og_u8(grids.host[1])
    want_alive, want = keepref.routes(og28, pts, parent, vcost, j, goals, cut=True)
    assert 0 < want_alive.sum() < j
    alive = p.keep_tree_resident(grids, 1)
    assert grids.valid() and np.shares_memory(p.og, grids.host[1]) and np.array_equal(p.og, frames[1])  # nothing was uploaded
    assert np.array_equal(alive, want_alive)
    tc.same_routes(p.device_context().routes(goals, shortcut=True), want)
    assert p.keep_tree_resident(grids, 0).all()


# ------------------------------------------------------------------------------------------------ 10. one vertex, and refusals
def test_a_tree_of_the_start_alone(gpu_ctx):
    og = tc.wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = tc.plan_on_own_batch(gpu_ctx, 0, 1, (5, 5), (190, 150), np.array([[6, 6]]))
    assert res.j == 1
    og2 = og8.copy()
    og2[40, 40] = 1
    gpu_ctx.set_grid(og2)
    assert b.keep_tree(0).tolist() == [True]
    v, c = b.connect_goals(0, [(150, 10), (10, 100), (60, 60)])
    assert v.tolist() == [-1, 0, -1] and c[1] == float(np.sqrt(np.float64(25 + 95 * 95)))
    og2[5, 5] = 1
    gpu_ctx.set_grid(og2)
    assert b.keep_tree(0).tolist() == [False]
    assert b.connect_goals(0, [(10, 100)])[0].tolist() == [-1]
    b.close()


def test_trees_of_exactly_1_2_63_to_65_and_1023_to_1025_vertices(gpu_ctx):
    """the compaction's wave and pass edges (64 and 1024 vertices) and the one-round case of the pointer jumping (1 and 2 vertices): the
    trees of treecalls.SIZES, the cells of vertex j // 2 and of the last vertex turned into obstacles"""
    def check(b, q, c):
        pts, parent, vcost, j = tc.tree_of(b.get_result(q))
        assert j == c["ro"].j
        og2 = c["og8"].copy()
        for k in (j // 2, j - 1):
            og2[pts[k][0], pts[k][1]] = 1
        # four goals: two corners, and the cell behind either obstacle as the root sees it (on an empty map the root itself is the
        # cheapest vertex for every goal it sees: triangle inequality)
        goals = np.array([np.clip(pts[k] + np.sign(pts[k] - pts[0]), 0, 63) for k in (j // 2, j - 1)] + [(0, 0), (63, 63)])
        want, v, cost = keepref.connect(og2, pts, parent, vcost, j, goals)
        if j >= 3:
            assert want[0] and not want[j // 2] and not want[j - 1] and 0 < want.sum() < j
        else:
            assert want.tolist() == [[False], [True, False]][j - 1]
        gpu_ctx.set_grid(og2)
        alive = b.keep_tree(q)
        assert np.array_equal(alive, want), (j, np.flatnonzero(alive != want)[:8])
        gv, gc = b.connect_goals(q, goals)
        assert np.array_equal(gv, v) and np.array_equal(gc, cost), j

    cs = []
    for k in tc.SIZES[1:]:
        og8, xs, samples, n = tc.sized(k, 100 + k)
        cs.append(tc.oracle_case(og8, 0, n, xs, (63, 63), samples, 0))
    b = tc.shaped_batch(gpu_ctx, cs[0], "team", Q=len(cs), n_cap=1040)
    for q, c in enumerate(cs):
        tc.set_case_query(b, q, c)
    b.launch()
    b.sync()
    for q, c in enumerate(cs):
        assert c["ro"].j == tc.SIZES[q + 1]
        check(b, q, c)
    b.close()
    # the tree of one vertex: the start boxed in, on a map and in a batch of its own
    og8, xs, samples, n = tc.sized(1, 101)
    c = tc.oracle_case(og8, 0, n, xs, (63, 63) if tuple(xs) != (63, 63) else (0, 0), samples, 0)
    assert c["ro"].j == 1
    b = tc.shaped_batch(gpu_ctx, c, "team")
    tc.set_case_query(b, 0, c)
    b.launch()
    b.sync()
    check(b, 0, c)
    b.close()


def test_refusals():
    ctx = _ffi.Context(0)
    og = tc.wall_map()
    og8 = oracle.og_u8(og)
    ctx.set_grid(og8)
    L = _ffi.lib()
    tc.refused_with_word(_ffi.RRT_E_ARG, "no rrt_plan", ctx.keep_tree)
    samples = tc.free_samples(og, 500, 17)
    b = _ffi.Batch(ctx, 2, 500)
    tc.refused_with_word(_ffi.RRT_E_ARG, "no query set", b.keep_tree, 0)
    q, keep = _ffi.make_query(1, 500, (5, 5), (190, 150), samples, r2_rewire=900)
    b.set_query(0, q)
    tc.refused_with_word(_ffi.RRT_E_ARG, "not launched", b.keep_tree, 0)
    tc.refused_with_word(_ffi.RRT_E_ARG, "no rrt_batch_keep_tree", b.keep_tree_ms)
    b.launch()
    b.sync()
    tc.refused_with_word(_ffi.RRT_E_ARG, "q=2", b.keep_tree, 2)
    tc.refused_with_word(_ffi.RRT_E_ARG, "q=-1", b.keep_tree, -1)
    tc.refused_with_word(_ffi.RRT_E_ARG, "no query set", b.keep_tree, 1)
    n_alive = _ffi.C.c_int32(0)
    assert L.rrt_batch_keep_tree(None, 0, _ffi.C.byref(n_alive), None) == _ffi.RRT_E_ARG
    assert L.rrt_batch_keep_tree(b._h, 0, None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_keep_tree(None, _ffi.C.byref(n_alive), None) == _ffi.RRT_E_ARG
    assert L.rrt_batch_keep_tree(b._h, 0, _ffi.C.byref(n_alive), None) == _ffi.RRT_OK and n_alive.value == b.get_result(0).j  # no flags wanted
    want = b.routes(0, [(150, 150)], shortcut=True)
    # a set_query in a kept query's place drops its view with its tree
    b.set_query(0, q)
    tc.refused_with_word(_ffi.RRT_E_ARG, "not launched", b.connect_goals, 0, [(150, 150)])
    b.launch()
    b.sync()
    tc.same_routes(b.routes(0, [(150, 150)], shortcut=True), want)
    # another shape
    ctx.set_grid(np.zeros((64, 64), dtype=np.uint8))
    tc.refused_with_word(_ffi.RRT_E_ARG, "shape", b.keep_tree, 0)
    b.close()
    # an Informed query that waits for its unit ball has no finished tree
    b = _ffi.Batch(ctx, 1, 300)
    free = np.argwhere(np.zeros((64, 64)) == 0)
    s = hostprep.draw_free_samples(np.random.default_rng(18), free, 300)
    q, keep = _ffi.make_query(2, 300, (5, 5), (40, 40), s, r2_rewire=400, goal_d2=900, Cmat=hostprep.rotation_to_world_frame(np.array((5, 5)), np.array((40, 40))))
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert b.get_result(0).status == _ffi.RRT_NEED_UNITBALL
    tc.refused_with_word(_ffi.RRT_E_ARG, "unit-ball", b.keep_tree, 0)
    b.close()
    # a Dubins batch
    hd = np.random.default_rng(19).integers(0, 16, size=300)
    b = _ffi.Batch(ctx, 1, 300, dubins=True)
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR, 300, (5, 5, 0), (40, 40, 3), s, r2_rewire=400, headings=hd, rho=3.0, nh=16)
    b.set_query(0, q)
    b.launch()
    b.sync()
    tc.refused_with_word(_ffi.RRT_E_UNSUPPORTED, "Dubins", b.keep_tree, 0)
    b.close()
    ctx.close()


def test_the_planner_keeps_its_state_rules():
    og = tc.wall_map()
    og2 = _new_map(og)
    p = amd.RRTStandard(og, 500, pbar=False, seed=3)
    with pytest.raises(RuntimeError, match="plan"):
        p.keep_tree(og2)
    p.plan(XS, XG)
    p.set_og(og2)
    with pytest.raises(RuntimeError, match="plan"):  # set_og still drops the tree
        p.keep_tree(og2)
    with pytest.raises(RuntimeError, match="plan"):
        p.connect_goals([(150, 150)])
    T, gv = p.plan(XS, XG)
    with pytest.raises(ValueError, match="planned on"):
        p.keep_tree(np.zeros((64, 64), dtype=np.int64))
    v0, c0 = p.connect_goals([(150, 150)])  # (the refusal changed nothing)
    alive = p.keep_tree(og)
    assert len(alive) == p.last_stats["j"]
    p.set_n(500)
    with pytest.raises(RuntimeError, match="plan"):
        p.keep_tree(og2)

    def costfn(vcosts, points, v, x):
        return vcosts[v] + 2.0 * amd.r2norm(points[v] - x)

    h = amd.RRTStar(np.zeros((48, 40), dtype=np.int64), 40, 12, costfn=costfn, pbar=False, seed=0)
    h.plan(np.array((3, 3)), np.array((40, 30)))
    assert h.last_route == "host"
    with pytest.raises(ValueError, match="host route"):
        h.keep_tree(np.zeros((48, 40), dtype=np.int64))
