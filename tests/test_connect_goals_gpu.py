"""GPU: many goals connected to a finished tree in one device call (rrt_goals_kernel / rrt_goals_large_kernel,
rrt_batch_connect_goals / rrt_plan_connect_goals, RRT.connect_goals / RRT.paths_to).

Every comparison is exact: vertices with ==, costs with array_equal.  The check is goalref.py (f64 costs, stable argsort, the
oracle's line walk), and for the planners' own goals plan() itself and oracle.plan."""
import numpy as np
import pytest

import goalref
import oracle
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTStarDubins
from treecalls import free_goals, free_samples, plan_on_own_batch, refused_with_word, same_snapshot, snapshot, wall_map

pytestmark = pytest.mark.gpu

TPB = 1024  # threads of the workgroup that decides a goal (rrt_kernel_abi.h)
INF = np.inf


def _check_rows(og8, res, goals, vertex, cost):
    rv, rc, tried = goalref.connect(og8, res.pts, res.vcost, res.j, goals)
    assert np.array_equal(vertex, rv), np.flatnonzero(vertex != rv)[:8]
    assert np.array_equal(cost, rc)
    return rv, rc, tried


# ------------------------------------------------------------------------------------------------ against plan() and the oracle
@pytest.mark.parametrize("kind", ["std", "star", "informed"])
def test_the_planners_own_goal_gets_the_parent_and_cost_plan_gave_it(kind):
    og = wall_map()
    xs, xg = np.array((5, 5)), np.array((190, 150))
    p = {"std": lambda: amd.RRTStandard(og, 2000, pbar=False, seed=1), "star": lambda: amd.RRTStar(og, 2000, 30, pbar=False, seed=1),
         "informed": lambda: amd.RRTStarInformed(og, 2000, 30, 25, pbar=False, seed=1)}[kind]()
    T, gv = p.plan(xs, xg)
    assert gv == p.last_stats["j"] and gv > 100  # the goal was found: it is the row after the tree
    (u,) = T.pred[gv]
    vertex, cost = p.connect_goals([xg])
    assert vertex.dtype == np.int32 and cost.dtype == np.float64 and vertex.shape == cost.shape == (1,)
    assert vertex[0] == u and cost[0] == T.edges[u, gv]["cost"]
    v1, c1 = p.connect_goals(xg)  # a single point
    assert np.array_equal(v1, vertex) and np.array_equal(c1, cost)


@pytest.mark.parametrize("kind", ["star", "std"])
def test_other_goals_get_what_a_plan_towards_them_would_have_given(kind):
    """RRTStandard / RRTStar grow the same tree whatever the goal: oracle.plan on the same samples towards g_k connects g_k as
    row k of ONE connect_goals call on the tree grown towards another goal"""
    og = wall_map()
    og8 = oracle.og_u8(og)
    n, seed, xs = 2000, 2, (5, 5)
    alg, kw = (0, {}) if kind == "std" else (1, dict(r_rewire=30))
    r2 = hostprep.radius_threshold(30) if alg else 0
    goals = np.concatenate([free_goals(og, 10, 3), [[30, 130], [100, 100]]])  # ... one in the closed box, one anywhere
    p = (amd.RRTStar if alg else amd.RRTStandard)(og, n, pbar=False, seed=seed, **kw)
    p.plan(np.array(xs), np.array((190, 150)))
    vertex, cost = p.connect_goals(goals)
    samples = free_samples(og, n, seed)
    connected = 0
    for k, g in enumerate(goals):
        st, ro = oracle.plan(og8, n, alg, xs, g, samples, r2_rewire=r2, logs=False)
        if ro.found:
            assert (vertex[k], cost[k]) == (ro.parent[ro.j], ro.vcost[ro.j]), k
            connected += 1
        else:
            assert (vertex[k], cost[k]) == (-1, INF), k
    assert connected >= 10 and vertex[10] == -1


# ------------------------------------------------------------------------------------------------ the kernel's own paths
def test_more_goals_than_workgroups(gpu_ctx):
    """1500 goals on at most 512 workgroups: every workgroup decides several, reusing its slab and its LDS tables"""
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 1, 600, (5, 5), (190, 150), free_samples(og, 600, 4), r2=hostprep.radius_threshold(30))
    goals = np.concatenate([free_goals(og, 1480, 5), np.argwhere(og != 0)[::45][:20]])
    assert len(goals) == 1500
    vertex, cost = b.connect_goals(0, goals)
    rv, rc, tried = _check_rows(og8, res, goals, vertex, cost)
    assert (tried == 1).sum() > 100 and ((tried > 1) & (rv >= 0)).sum() > 100 and (rv < 0).sum() >= 20
    b.close()


def test_goals_whose_cheapest_vertex_is_behind_a_wall(gpu_ctx):
    """goals right behind a wall: the (cost, index)-smallest vertex is on the near side and blocked, the winner comes out of the
    full ordering; goals in the open: the smallest vertex sees them"""
    og = np.zeros((200, 160), dtype=np.int64)
    og[100:104, :130] = 1
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 1, 2000, (10, 20), (190, 20), free_samples(og, 2000, 6), r2=hostprep.radius_threshold(30))
    behind = np.array([(106, y) for y in range(10, 100, 3)])
    open_ = np.array([(60, y) for y in range(10, 150, 5)])
    vertex, cost = b.connect_goals(0, np.concatenate([behind, open_]))
    rv, rc, tried = _check_rows(og8, res, np.concatenate([behind, open_]), vertex, cost)
    assert np.all(tried[:len(behind)] > 1) and np.all(rv[:len(behind)] >= 0)  # the first candidate of each was blocked
    assert np.all(tried[len(behind):] == 1)
    b.close()


def test_unreachable_goals_get_minus_one_and_inf(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    b, res = plan_on_own_batch(gpu_ctx, 1, 600, (5, 5), (190, 150), free_samples(og, 600, 4), r2=hostprep.radius_threshold(30))
    goals = np.array([(67, 10), (20, 120), (30, 130), (25, 125), (150, 150)])  # on a wall, on the box, two in the box, one free
    assert og[67, 10] == 1 and og[20, 120] == 1 and og[30, 130] == 0
    vertex, cost = b.connect_goals(0, goals)
    _check_rows(og8, res, goals, vertex, cost)
    assert vertex[:4].tolist() == [-1] * 4 and np.all(cost[:4] == INF) and vertex[4] >= 0 and np.isfinite(cost[4])
    b.close()
    # a tree of the start alone (n = 1: j == 1) and a goal it does not see
    b, res = plan_on_own_batch(gpu_ctx, 0, 1, (5, 5), (190, 150), np.array([[6, 6]]))
    assert res.j == 1
    vertex, cost = b.connect_goals(0, [(150, 10), (10, 100)])
    _check_rows(og8, res, [(150, 10), (10, 100)], vertex, cost)
    assert vertex.tolist() == [-1, 0] and cost[0] == INF
    b.close()
    # xstart on an obstacle: nothing is ever accepted, and the start sees nothing
    samples = free_samples(og, 50, 7)
    st, ro = oracle.plan(og8, 50, 1, (67, 10), (190, 150), samples, r2_rewire=900, logs=False)
    b, res = plan_on_own_batch(gpu_ctx, 1, 50, (67, 10), (190, 150), samples, r2=900)
    assert res.j == ro.j == 1 and not ro.found
    vertex, cost = b.connect_goals(0, [(60, 10), (150, 150)])
    assert vertex.tolist() == [-1, -1] and np.all(cost == INF)
    b.close()


def _tie_query(ctx, first, fillers, last):
    """RRTStandard from (50, 50) on the samples `first`, then `fillers` cells of the far row y = 5, then `last`: every one is
    accepted.  Returns (batch, result, {cell: vertex})"""
    cells = list(first) + [(k, 5) for k in range(fillers)] + list(last)
    samples = np.array(cells + [(0, 0)])  # (one more, rejected: the tree is full)
    b, res = plan_on_own_batch(ctx, 0, len(samples), (50, 50), (99, 99), samples)
    assert res.j == len(cells) + 1
    pts = [tuple(p) for p in res.pts[:res.j].tolist()]
    return b, res, {c: pts.index(c) for c in cells}


@pytest.mark.parametrize("fillers", [0, 100])
def test_equal_costs_go_to_the_lower_index(fillers):
    ctx = _ffi.Context(0)
    # an empty grid: the vertex (50, 60) on the segment start -> goal costs exactly what the start costs, 10 + 30 == 0 + 40,
    # and both see the goal
    og8 = np.zeros((100, 100), dtype=np.uint8)
    ctx.set_grid(og8)
    b, res, at = _tie_query(ctx, [], fillers, [(50, 60)])
    iM = at[(50, 60)]
    assert iM == fillers + 1 and res.vcost[iM] + 30.0 == 40.0 == float(np.sqrt(np.float64(1600)))
    vertex, cost = b.connect_goals(0, [(50, 90)])
    rv, rc, tried = _check_rows(og8, res, [(50, 90)], vertex, cost)
    assert (vertex[0], cost[0]) == (0, 40.0) and tried[0] == 1
    b.close()
    # one obstacle cell between the start and the goal: the start is blocked; L = (44, 58) and R = (56, 58) both hang off the start
    # with cost 10.0, are equally far from the goal and see it
    og8[50, 70] = 1
    ctx.set_grid(og8)
    b, res, at = _tie_query(ctx, [(44, 58)], fillers, [(56, 58)])
    iL, iR = at[(44, 58)], at[(56, 58)]
    cL = res.vcost[iL] + np.sqrt(np.float64(36 + 32 * 32))
    assert res.vcost[iL] == res.vcost[iR] == 10.0 and iL == 1 and iR == fillers + 2  # (100 fillers: different waves own the two)
    vertex, cost = b.connect_goals(0, [(50, 90)])
    rv, rc, tried = _check_rows(og8, res, [(50, 90)], vertex, cost)
    assert (vertex[0], cost[0]) == (iL, cL) and tried[0] == 2
    assert oracle.collisionfree(og8, (56, 58), (50, 90))[0]
    b.close()
    ctx.close()


@pytest.mark.parametrize("j", [1, 63, 64, 65, TPB - 1, TPB, TPB + 1, 2049])
def test_tree_sizes_around_the_strides(gpu_ctx, j):
    """exactly j vertices: the tree grows in the empty left part (every distinct sample is accepted until the tree is full), the
    goals lie to the right, some behind a wall"""
    og = np.zeros((128, 96), dtype=np.int64)
    og[70:73, :80] = 1
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    cells = np.array([(x, y) for x in range(60) for y in range(96) if (x, y) != (0, 0)])
    samples = cells[np.random.default_rng(j).permutation(len(cells))[:j]]
    b, res = plan_on_own_batch(gpu_ctx, 1, j, (0, 0), (120, 90), samples, r2=hostprep.radius_threshold(12))
    assert res.j == j
    goals = [(76, 5), (76, 40), (100, 70), (127, 0), (80, 90), (65, 50), (71, 10), (127, 95)]
    vertex, cost = b.connect_goals(0, goals)
    rv, rc, tried = _check_rows(og8, res, goals, vertex, cost)
    assert rv[6] == -1  # (on the wall)
    if j >= 63:
        assert (rv >= 0).sum() >= 4 and (rv[:2] == -1).all() and (tried[rv >= 0] > 1).any() and (tried == 1).any()
    b.close()


def test_every_way_a_tree_is_grown(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    n, samples, r2 = 2500, free_samples(og, 2500, 8), hostprep.radius_threshold(25)
    goals = free_goals(og, 40, 9)
    got, names = [], []
    for bkw in (dict(), dict(team=1), dict(serial=True)):
        b, res = plan_on_own_batch(gpu_ctx, 1, n, (5, 5), (190, 150), samples, r2=r2, **bkw)
        names.append(b.kernel_name())
        got.append(b.connect_goals(0, goals))
        if not bkw:
            _check_rows(og8, res, goals, *got[0])
        b.close()
    assert names[0].startswith("rrt_expand_block_kernel") and names[1] == "rrt_pipe_kernel" and names[2].startswith("rrt_expand_kernel")
    for v, c in got[1:]:
        assert np.array_equal(v, got[0][0]) and np.array_equal(c, got[0][1])


def test_a_batch_of_three_queries_with_different_n(gpu_ctx):
    og = wall_map()
    og8 = oracle.og_u8(og)
    gpu_ctx.set_grid(og8)
    ns = [300, 5000, 1200]
    b = _ffi.Batch(gpu_ctx, 3, max(ns))
    keeps = []
    for q, n in enumerate(ns):
        qu, keep = _ffi.make_query(1, n, (5 + q, 5), (190, 150 - q), free_samples(og, n, 10 + q), r2_rewire=hostprep.radius_threshold(25))
        keeps.append(keep)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    goals = free_goals(og, 30, 13)
    for q in (2, 0):
        res = b.get_result(q)
        assert res.pts[0].tolist() == [5 + q, 5]
        _check_rows(og8, res, goals, *b.connect_goals(q, goals))
    b.close()


# ------------------------------------------------------------------------------------------------ large grids
def test_large_grid_batch_and_planner():
    W, H = 4096, 8
    og = np.zeros((W, H), dtype=np.int64)
    og[2000:2003, :6] = 1
    og8 = oracle.og_u8(og)
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    b, res = plan_on_own_batch(ctx, 1, 400, (1, 1), (4090, 6), free_samples(og, 400, 14), r2=hostprep.radius_threshold(500), large_grid=True)
    assert b.kernel_name() == "rrt_pipe_large_kernel" and res.j > 100
    goals = [(0, 0), (4095, 7), (4095, 0), (0, 7), (2004, 2), (1999, 3), (2001, 3), (3000, 4)]
    rv, rc, tried = _check_rows(og8, res, goals, *b.connect_goals(0, goals))
    assert rv[6] == -1 and (rv >= 0).sum() == 7 and (tried[rv >= 0] > 1).any()
    b.close()
    ctx.close()
    p = amd.RRTStar(og, 400, 500, pbar=False, seed=14)
    T, gv = p.plan(np.array((1, 1)), np.array((4090, 6)))
    assert p.last_route == "kernel-large"
    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    vertex, cost = p.connect_goals(goals)
    rv, rc, _ = goalref.connect(og8, points, vcosts, j, goals)
    assert np.array_equal(vertex, rv) and np.array_equal(cost, rc)


# ------------------------------------------------------------------------------------------------ the batch afterwards
def test_the_batch_is_left_as_it_was(gpu_ctx):
    og = wall_map()
    gpu_ctx.set_grid(oracle.og_u8(og))
    b, res = plan_on_own_batch(gpu_ctx, 1, 3000, (5, 5), (190, 150), free_samples(og, 3000, 15), r2=hostprep.radius_threshold(25))
    before = snapshot(res)
    goals = free_goals(og, 700, 16)
    first = b.connect_goals(0, goals)
    assert same_snapshot(before, snapshot(b.get_result(0)))
    second = b.connect_goals(0, goals)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])
    b.rearm()
    b.launch()
    b.sync()
    assert same_snapshot(before, snapshot(b.get_result(0)))
    third = b.connect_goals(0, goals[:5])  # (and fewer goals than before)
    assert np.array_equal(first[0][:5], third[0]) and np.array_equal(first[1][:5], third[1])
    v0, c0 = b.connect_goals(0, np.zeros((0, 2), dtype=np.int64))
    assert v0.shape == c0.shape == (0,)
    b.close()


def test_refusals():
    ctx = _ffi.Context(0)
    og = wall_map()
    ctx.set_grid(oracle.og_u8(og))
    refused_with_word(_ffi.RRT_E_ARG, "no rrt_plan", ctx.connect_goals, [(5, 5)])
    samples = free_samples(og, 500, 17)
    b = _ffi.Batch(ctx, 2, 500)
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.connect_goals, 0, [(5, 5)])
    q, keep = _ffi.make_query(1, 500, (5, 5), (190, 150), samples, r2_rewire=900)
    b.set_query(0, q)
    refused_with_word(_ffi.RRT_E_ARG, "not launched", b.connect_goals, 0, [(5, 5)])
    b.launch()
    b.sync()
    b.connect_goals(0, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "q=2", b.connect_goals, 2, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "q=-1", b.connect_goals, -1, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.connect_goals, 1, [(5, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.connect_goals, 0, [(5, 5), (200, 5)])
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.connect_goals, 0, [(5, -1)])
    refused_with_word(_ffi.RRT_E_ARG, "at most", b.connect_goals, 0, np.zeros(((1 << 20) + 1, 2), dtype=np.int32))
    b.rearm()
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.connect_goals, 0, [(5, 5)])
    b.launch()
    b.sync()
    want = b.connect_goals(0, [(150, 150)])
    # the grid replaced between run and call: same shape, another generation
    ctx.set_grid(oracle.og_u8(og))
    refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_goals, 0, [(150, 150)])
    b.rearm()
    b.launch()
    b.sync()
    got = b.connect_goals(0, [(150, 150)])
    assert got[0][0] == want[0][0] and got[1][0] == want[1][0]
    ctx.set_grid(np.zeros((64, 64), dtype=np.uint8))
    refused_with_word(_ffi.RRT_E_ARG, "shape", b.connect_goals, 0, [(5, 5)])
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
    refused_with_word(_ffi.RRT_E_ARG, "unit-ball", b.connect_goals, 0, [(5, 5)])
    b.close()
    # a Dubins batch
    hd = np.random.default_rng(19).integers(0, 16, size=300)
    b = _ffi.Batch(ctx, 1, 300, dubins=True)
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR, 300, (5, 5, 0), (40, 40, 3), s, r2_rewire=400, headings=hd, rho=3.0, nh=16)
    b.set_query(0, q)
    b.launch()
    b.sync()
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "Dubins", b.connect_goals, 0, [(5, 5)])
    b.close()
    ctx.close()
    with pytest.raises(ValueError, match="Dubins"):
        RRTStarDubins(np.zeros((64, 64), dtype=int), 100, 20, 3.0, pbar=False).connect_goals([(5, 5)])


# ------------------------------------------------------------------------------------------------ paths
def test_paths_to():
    og = wall_map()
    og8 = oracle.og_u8(og)
    xs = np.array((5, 5))
    p = amd.RRTStandard(og, 2500, pbar=False, seed=20)
    T, gv = p.plan(xs, np.array((190, 150)))
    goals = np.concatenate([free_goals(og, 25, 21), [[30, 130], [67, 10]]])
    vertex, cost = p.connect_goals(goals)
    paths = p.paths_to(T, goals)
    assert len(paths) == len(goals) and [pt is None for pt in paths] == (vertex < 0).tolist()
    assert paths[-1] is None and paths[-2] is None and sum(pt is not None for pt in paths) >= 20
    for pt, g, v, c in zip(paths, goals, vertex, cost):
        if pt is None:
            continue
        assert pt.ndim == 2 and pt.shape[1] == 2 and pt[0].tolist() == xs.tolist() and pt[-1].tolist() == g.tolist()
        assert pt[-2].tolist() == T.nodes[int(v)]["pt"].tolist()
        length = 0.0  # RRTStandard: a vertex costs its parent's cost plus the edge, summed from the root in this order
        for a, bb in zip(pt[:-1], pt[1:]):
            assert oracle.collisionfree(og8, a, bb)[0]
            length = length + float(np.sqrt(np.float64(((bb - a) ** 2).sum())))
        assert length == c
    # the same from a graph that has been materialised
    T.adj  # noqa: B018
    again = p.paths_to(T, goals[:3])
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(again, paths[:3]))
    # state: a new grid or n invalidates the tree until the next plan()
    p.set_n(2500)
    with pytest.raises(RuntimeError, match="plan"):
        p.connect_goals(goals)
    p.plan(xs, np.array((190, 150)))
    with pytest.raises(ValueError, match="outside"):
        p.connect_goals([(200, 0)])
    p.set_og(og)
    with pytest.raises(RuntimeError, match="plan"):
        p.connect_goals(goals)
