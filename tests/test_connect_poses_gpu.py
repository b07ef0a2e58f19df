"""GPU: many goal poses connected to a finished Dubins tree in one device call (rrt_pose_goals_kernel, rrt_batch_connect_poses /
rrt_plan_connect_poses, RRTDubins / RRTStarDubins .connect_poses / .paths_to_poses).

Every comparison is exact: vertices and costs with ==.  The check is poseref.py (the oracle's word and sweep, a stable argsort) on
the workloads it defines, and for the planners' own goals plan() itself and oracle.dubins_plan.  The conditions that make the made-up
trees below worth running (the ties are ties, the trees have exactly j vertices, the fuzz connects) are asserted without a GPU, in
test_connect_poses_cpu.py.  Only the independent audit (oracle/dubins_ref.c: libm, no shared header) has tolerances: its own."""
import numpy as np
import pytest

import oracle
import poseref
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins
from posecalls import planned_batch_and_result
from rrtplanner_amd.oggen import DeviceGrids
from treecalls import refused_with_word, same_snapshot, snapshot

pytestmark = pytest.mark.gpu

MAX_WORKGROUPS = 512  # POSES_MAX_SLABS of rrt_kernel_abi.h: the workgroups of one launch, each deciding goals g, g + 512, ...
INF = np.inf


def _same(got, w, rows=slice(None)):
    vertex, cost = got
    assert vertex.dtype == np.int32 and cost.dtype == np.float64
    assert np.array_equal(vertex, w.vertex[rows]), np.flatnonzero(vertex != w.vertex[rows])[:8]
    assert np.array_equal(cost, w.cost[rows]), np.flatnonzero(cost != w.cost[rows])[:8]


# ------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize("name", sorted(poseref.SPECS))
def test_workloads_against_the_restatement(gpu_ctx, name):
    w = poseref.workload(name)
    poseref.check_conditions(w)
    b, res = planned_batch_and_result(gpu_ctx, w)
    _same(b.connect_poses(0, w.goals), w)
    words, sweeps = b.connect_poses_counts()
    swept = w.rank[w.vertex >= 0] + 1
    free_unconnected = int(((w.vertex < 0) & (w.og8[w.goals[:, 0], w.goals[:, 1]] == 0)).sum())
    assert swept.sum() + free_unconnected * w.j <= sweeps <= words
    b.close()


def test_more_goals_than_workgroups_and_scratch_that_grows(gpu_ctx):
    """700 goals on at most 512 workgroups: every workgroup decides one or two, reusing its slab and its LDS tables; around it
    calls of 5 goals: the scratch grows once and is reused"""
    w = poseref.workload("E", 700 - 4)
    assert len(w.goals) == 700 > MAX_WORKGROUPS
    poseref.check_conditions(w)
    b, res = planned_batch_and_result(gpu_ctx, w)
    _same(b.connect_poses(0, w.goals[:5]), w, slice(0, 5))
    _same(b.connect_poses(0, w.goals), w)
    _same(b.connect_poses(0, w.goals[-5:]), w, slice(695, 700))
    v0, c0 = b.connect_poses(0, np.zeros((0, 3), dtype=np.int64))
    assert v0.shape == c0.shape == (0,) and b.connect_poses_counts() == (0, 0)
    b.close()


def test_a_batch_of_three_queries_each_with_its_own_rho_headings_and_tree(gpu_ctx):
    w = poseref.workload("A")
    gpu_ctx.set_grid(w.og8)
    free = np.argwhere(w.og8 == 0)
    par = [(4.0, 16, 1, 900), (5.0, 8, 0, 500), (6.0, 32, 1, 1400)]  # rho, nh, star, n
    b = _ffi.Batch(gpu_ctx, 3, 1400, dubins=True)
    keeps, refs = [], []
    for q, (rho, nh, star, n) in enumerate(par):
        rng = np.random.default_rng(40 + q)
        samples, heads = hostprep.draw_free_samples(rng, free, n), rng.integers(0, nh, n)
        xs, xg, r2 = (w.xs[0], w.xs[1], q % nh), (w.xg[0], w.xg[1], (3 + q) % nh), hostprep.radius_threshold(20) if star else 0
        qu, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR if star else _ffi.ALG_DUBINS, n, xs, xg, samples, r2_rewire=r2, headings=heads, rho=rho, nh=nh)
        keeps.append(keep)
        b.set_query(q, qu)
        refs.append(oracle.dubins_plan(w.og8, n, star, xs, xg, samples, heads, r2_rewire=r2, rho=rho, nh=nh, logs=False)[1])
    b.launch()
    b.sync()
    for q in (2, 0, 1):
        rho, nh, star, n = par[q]
        ro, res = refs[q], b.get_result(q)
        assert res.j == ro.j > 50 and np.array_equal(res.vcost[:ro.j], ro.vcost[:ro.j])
        goals = np.column_stack([free[np.random.default_rng(50).integers(0, len(free), 12)], np.random.default_rng(51).integers(0, 8, 12)])
        goals = np.concatenate([goals, [(ro.pts[ro.j, 0], ro.pts[ro.j, 1], ro.head[ro.j])] if ro.found else np.zeros((0, 3), dtype=np.int64)])
        rv, rc, rank = poseref.connect(w.og8, ro.pts, ro.head, ro.vcost, ro.j, goals, rho, nh)
        vertex, cost = b.connect_poses(q, goals)
        assert np.array_equal(vertex, rv) and np.array_equal(cost, rc) and (rv >= 0).sum() >= 6
        if ro.found:
            assert (vertex[-1], cost[-1]) == (ro.parent[ro.vgoal], ro.vcost[ro.vgoal])
    b.close()


# ------------------------------------------------------------------------------------------------ the counters
def test_counts_of_single_goals(gpu_ctx):
    w = poseref.workload("B")
    b, res = planned_batch_and_result(gpu_ctx, w)
    with pytest.raises(_ffi.RRTError) as e:
        b.connect_poses_counts()
    assert e.value.code == _ffi.RRT_E_ARG
    b.connect_poses(0, w.goals[w.i_obstacle])
    assert b.connect_poses_counts() == (0, 0)  # a goal on an obstacle cell: decided without a word
    unreachable = [g for g in range(len(w.goals)) if w.vertex[g] < 0 and w.og8[w.goals[g, 0], w.goals[g, 1]] == 0]
    assert unreachable
    v, c = b.connect_poses(0, w.goals[unreachable[0]])
    assert (v[0], c[0]) == (-1, INF)
    assert b.connect_poses_counts() == (w.j, w.j)  # nothing passes: every vertex is priced and swept
    seen = 0
    for g in np.flatnonzero(w.vertex >= 0)[:8].tolist():
        _same(b.connect_poses(0, w.goals[g]), w, slice(g, g + 1))
        words, sweeps = b.connect_poses_counts()
        assert w.rank[g] + 1 <= sweeps <= w.j and sweeps <= words <= w.j, (g, w.rank[g], words, sweeps)
        seen += w.rank[g] > 0
    assert seen >= 2
    b.close()


# ------------------------------------------------------------------------------------------------ the planners
@pytest.mark.parametrize("cls", [RRTStarDubins, RRTDubins])
def test_planners_end_to_end(cls):
    w = poseref.workload("A" if cls is RRTStarDubins else "D")
    args = (w.og, w.n) + ((20,) if cls is RRTStarDubins else ()) + (w.rho,)
    p = cls(*args, n_headings=w.nh, pbar=False, seed=SEEDS[w.name])
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    j = p.last_stats["j"]
    assert j == w.j and gv == j  # the planner draws the workload's stream: its tree is the oracle's, the goal row behind it
    vertex, cost, heading = p.connect_poses(w.goals)
    assert np.array_equal(vertex, w.vertex) and np.array_equal(cost, w.cost) and np.array_equal(heading, w.goals[:, 2])
    (u,) = T.pred[gv]
    assert vertex[w.i_own] == u and cost[w.i_own] == T.edges[u, gv]["cost"]
    # any heading: against the restatement over all headings of the cell
    cell = w.goals[0, :2]
    v1, c1, h1 = p.connect_poses((cell[0], cell[1], -1))
    assert (v1[0], c1[0], h1[0]) == poseref.any_heading(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, cell, w.rho, w.nh)
    # routes: tree edges from the root, then the goal
    poses = np.concatenate([w.goals[:6], [(cell[0], cell[1], -1)], w.goals[w.i_obstacle:w.i_obstacle + 2]])
    vertex, cost, heading = p.connect_poses(poses)
    routes = p.paths_to_poses(T, poses)
    assert [r is None for r in routes] == (vertex < 0).tolist() and routes[7] is None and sum(r is not None for r in routes) >= 4
    for r, g, v, h in zip(routes, poses, vertex, heading):
        if r is None:
            continue
        assert r.dtype == np.int64 and r.shape[1] == 3 and tuple(r[0]) == tuple(w.xs) and tuple(r[-1]) == (g[0], g[1], h)
        assert tuple(r[-2]) == (*w.ro.pts[v], w.ro.head[v])
        ids = p.route2gv(T, int(v))
        assert len(ids) == len(r) - 1
        for a, bb, row in zip(ids[:-1], ids[1:], r[1:]):
            assert w.ro.parent[bb] == a and tuple(row) == (*w.ro.pts[bb], w.ro.head[bb])
        line = p.poses_polyline(r)
        assert line.ndim == 2 and line.shape[1] == 2 and np.allclose(line[0], r[0, :2]) and np.allclose(line[-1], r[-1, :2], atol=1e-6)
    # state: a new n invalidates the tree until the next plan()
    p.set_n(w.n)
    with pytest.raises(RuntimeError, match="plan"):
        p.connect_poses(w.goals[:2])


SEEDS = {name: spec[7] for name, spec in poseref.SPECS.items()}


# ------------------------------------------------------------------------------------------------ the batch afterwards
def test_the_batch_is_left_as_it_was(gpu_ctx):
    w = poseref.workload("A")
    b, res = planned_batch_and_result(gpu_ctx, w)
    before = snapshot(res)
    _same(b.connect_poses(0, w.goals), w)
    assert same_snapshot(before, snapshot(b.get_result(0)))
    b.rearm()
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.connect_poses, 0, w.goals)  # until the query has finished again
    b.launch()
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.connect_poses, 0, w.goals)
    b.sync()
    assert same_snapshot(before, snapshot(b.get_result(0)))
    _same(b.connect_poses(0, w.goals), w)
    b.close()


def test_refusals():
    w = poseref.workload("E")
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    W, H = w.og8.shape
    ok = [(5, 5, 0)]
    refused_with_word(_ffi.RRT_E_ARG, "no rrt_plan", ctx.connect_poses, ok)
    b = _ffi.Batch(ctx, 2, w.n, dubins=True)
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.connect_poses, 0, ok)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    refused_with_word(_ffi.RRT_E_ARG, "not launched", b.connect_poses, 0, ok)
    b.launch()
    b.sync()
    want = b.connect_poses(0, w.goals[:3])
    _same(want, w, slice(0, 3))
    refused_with_word(_ffi.RRT_E_ARG, "q=2", b.connect_poses, 2, ok)
    refused_with_word(_ffi.RRT_E_ARG, "q=-1", b.connect_poses, -1, ok)
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.connect_poses, 1, ok)
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.connect_poses, 0, [(5, 5, 0), (W, 5, 0)])
    refused_with_word(_ffi.RRT_E_ARG, "outside", b.connect_poses, 0, [(5, -1, 0)])
    refused_with_word(_ffi.RRT_E_ARG, "heading", b.connect_poses, 0, [(5, 5, w.nh)])
    refused_with_word(_ffi.RRT_E_ARG, "heading", b.connect_poses, 0, [(5, 5, 0), (5, 5, -1)])  # the C ABI takes concrete headings only
    refused_with_word(_ffi.RRT_E_ARG, "at most", b.connect_poses, 0, np.zeros(((1 << 20) + 1, 3), dtype=np.int32))
    lib = _ffi.lib()
    v, c, g = np.zeros(1, dtype=np.int32), np.zeros(1), np.zeros((1, 3), dtype=np.int32)
    assert lib.rrt_batch_connect_poses(b._h, 0, None, 1, v.ctypes.data, c.ctypes.data) == _ffi.RRT_E_ARG
    assert lib.rrt_batch_connect_poses(b._h, 0, g.ctypes.data, 1, None, c.ctypes.data) == _ffi.RRT_E_ARG
    assert lib.rrt_batch_connect_poses(b._h, 0, g.ctypes.data, 1, v.ctypes.data, None) == _ffi.RRT_E_ARG
    assert lib.rrt_batch_connect_poses(None, 0, g.ctypes.data, 1, v.ctypes.data, c.ctypes.data) == _ffi.RRT_E_ARG
    assert lib.rrt_batch_connect_poses(b._h, 0, g.ctypes.data, -1, v.ctypes.data, c.ctypes.data) == _ffi.RRT_E_ARG
    assert lib.rrt_batch_connect_poses_counts(b._h, None) == _ffi.RRT_E_ARG
    # the refused calls changed nothing: the counts are still those of the last call that ran
    assert b.connect_poses_counts()[1] >= int((w.rank[:3] + 1)[w.vertex[:3] >= 0].sum())
    # the grid replaced between run and call: same shape, another generation
    ctx.set_grid(w.og8)
    refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_poses, 0, ok)
    b.rearm()
    b.launch()
    b.sync()
    _same(b.connect_poses(0, w.goals[:3]), w, slice(0, 3))
    ctx.set_grid(np.zeros((W + 8, H), dtype=np.uint8))
    refused_with_word(_ffi.RRT_E_ARG, "shape", b.connect_poses, 0, ok)
    b.close()
    # a batch of a straight-line planner: its call is connect_goals
    ctx.set_grid(w.og8)
    b = _ffi.Batch(ctx, 1, w.n)
    q, keep = _ffi.make_query(1, w.n, w.xs[:2], w.xg[:2], w.samples, r2_rewire=w.r2)
    b.set_query(0, q)
    b.launch()
    b.sync()
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "rrt_batch_connect_goals", b.connect_poses, 0, ok)
    b.connect_goals(0, [(5, 5)])
    b.close()
    ctx.close()


def test_a_tree_whose_own_goal_is_unreachable_is_accepted():
    """workload F through rrt_plan: status -2, the tree is the start alone and complete; its own goal and a free pose answer -1 / inf"""
    w = poseref.workload("F")
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    q, keep = poseref.device_query(w)
    rc, res = ctx.plan(q, w.n)
    assert rc == _ffi.RRT_E_GOAL_UNREACHABLE and res.j == 1
    vertex, cost = ctx.connect_poses(w.goals)
    assert np.array_equal(vertex, w.vertex) and np.array_equal(cost, w.cost) and np.all(vertex == -1)
    ctx.close()


# ------------------------------------------------------------------------------------------------ exact ties
def _goal_row_of_plan(ctx, w):
    """the query through rrt_plan, both kernels: the tree and the goal row (go2goal_phase<true>'s decision) are the oracle's"""
    ctx.set_grid(w.og8)
    for serial in (False, True):
        q, keep = poseref.device_query(w)
        rc, res = ctx.plan(q, w.n, serial=serial)
        ro = w.ro
        live = ro.j + (1 if ro.found else 0)
        assert rc == w.status and (res.j, res.found, res.vgoal) == (ro.j, ro.found, ro.vgoal), (w.name, serial)
        assert np.array_equal(res.parent[:live], ro.parent[:live]) and np.array_equal(res.vcost[:live], ro.vcost[:live]), (w.name, serial)
        assert np.array_equal(res.pts[:live], ro.pts[:live]) and np.array_equal(res.head[:live], ro.head[:live]), (w.name, serial)
        _same(ctx.connect_poses(w.goals), w)  # ... and rrt_plan_connect_poses on that tree


def _asked_twice(ctx, w):
    """the order inside a bucket may differ between launches, the answer may not"""
    b, res = planned_batch_and_result(ctx, w)
    first = b.connect_poses(0, w.goals)
    _same(first, w)
    _same(b.connect_poses(0, w.goals), w)
    for g in range(min(3, len(w.goals))):  # ... nor with the goal asked alone
        _same(b.connect_poses(0, w.goals[g]), w, slice(g, g + 1))
    b.close()
    return first


@pytest.mark.parametrize("place", list(poseref.TIE_PLACES))
@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_a_duplicate_of_the_start_pose_never_wins(gpu_ctx, rho, nh, place):
    for star in (0, 1):
        w = poseref.tie_duplicate(rho, nh, star, place)
        poseref.check_tie_duplicate(w, place)
        vertex, cost = _asked_twice(gpu_ctx, w)
        assert not np.any(vertex == w.dup) and (vertex == 0).sum() >= 8
        _goal_row_of_plan(gpu_ctx, w)


@pytest.mark.parametrize("fillers", [0, 100])
def test_equal_costs_go_to_the_lower_index(gpu_ctx, fillers):
    for rho, nh in poseref.TIE_PAIRS:
        for star in (0, 1):
            a, b, iL, iR = poseref.tie_collinear(rho, nh, star, fillers)
            poseref.check_tie_collinear(a, b, iL, iR)
            vertex, cost = _asked_twice(gpu_ctx, a)
            assert (vertex[0], cost[0]) == (0, 70.0)
            vertex, cost = _asked_twice(gpu_ctx, b)
            assert vertex[0] == iL and cost[0] == b.c[0, iL] == b.c[0, iR]
            _goal_row_of_plan(gpu_ctx, a)
            _goal_row_of_plan(gpu_ctx, b)


def test_a_chain_in_which_every_cost_is_equal(gpu_ctx):
    """1100 vertices, one bucket, two rounds, every cost 1288.0: vertex 0.  Every merge of lanes and of waves is a tie here; the
    merge of the two rounds is one only if the scatter puts vertex 0 behind position 1023, which it does not in practice (see
    poseref.tie_chain and DESIGN.md 4.2g: the round merge's order on equal costs is not pinned by any test)"""
    w = poseref.tie_chain()
    poseref.check_tie_chain(w)
    vertex, cost = _asked_twice(gpu_ctx, w)
    assert (vertex[0], cost[0]) == (0, 1288.0)
    _goal_row_of_plan(gpu_ctx, w)


# ------------------------------------------------------------------------------------------------ trees around the strides
@pytest.mark.parametrize("j", poseref.STRIDE_J)
def test_tree_sizes_around_the_strides(gpu_ctx, j):
    for star in (0, 1):
        w = poseref.stride_tree(j, star)
        poseref.check_stride_tree(w, j)
        b, res = planned_batch_and_result(gpu_ctx, w)
        _same(b.connect_poses(0, w.goals), w)
        for g, goal in enumerate(w.goals):  # asked alone: what the counters must say follows from the semantics
            _same(b.connect_poses(0, goal), w, slice(g, g + 1))
            words, sweeps = b.connect_poses_counts()
            if w.vertex[g] >= 0:
                assert w.rank[g] + 1 <= sweeps <= words <= j, (w.name, g, w.rank[g], words, sweeps)
            elif w.og8[goal[0], goal[1]] == 0:
                assert (words, sweeps) == (j, j), (w.name, g, words, sweeps)
            else:
                assert (words, sweeps) == (0, 0), (w.name, g, words, sweeps)
        b.close()


# ------------------------------------------------------------------------------------------------ a fuzz over small trees
def test_pose_goals_fuzz_small(gpu_ctx):
    cases = poseref.fuzz_cases()
    assert len(cases) >= 100
    for w in cases:
        try:
            gpu_ctx.set_grid(w.og8)
            q, keep = poseref.device_query(w)
            rc, res = gpu_ctx.plan(q, w.n, logs=True, serial=w.serial)
            ro = w.ro
            live = ro.j + (1 if ro.found else 0)
            assert rc == w.status and (res.j, res.found, res.vgoal) == (ro.j, ro.found, ro.vgoal)
            assert np.array_equal(res.nearest_log, ro.nearest_log) and np.array_equal(res.accept_log, ro.accept_log)
            assert np.array_equal(res.pts[:live], ro.pts[:live]) and np.array_equal(res.head[:live], ro.head[:live])
            assert np.array_equal(res.parent[:live], ro.parent[:live]) and np.array_equal(res.vcost[:live], ro.vcost[:live])
            assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near
            _same(gpu_ctx.connect_poses(w.goals), w)
        except AssertionError as e:
            raise AssertionError(w.name) from e
    goals, connected, past_blocked = poseref.fuzz_coverage(cases)
    assert 4 * connected >= goals and 20 * past_blocked >= goals


# ------------------------------------------------------------------------------------------------ the independent audit
def _audit_of_the_devices_answers(ctx, w):
    b, res = planned_batch_and_result(ctx, w)
    vertex, cost = b.connect_poses(0, w.goals)
    b.close()
    a = poseref.goals_audit(w, vertex, cost)
    poseref.assert_goals_audit_clean(a, vertex)
    _same((vertex, cost), w)
    return a, vertex


def test_independent_audit_of_the_devices_answers(gpu_ctx):
    """the DEVICE's (vertex, cost) for every goal against oracle/dubins_ref.c, which shares no header with the kernel: on more than
    two rounds of vertices, on the stride tree of 2049, and on a tie tree -- where the duplicate has the start's pose, so libm gives
    both the same cost and the audit's first minimum must be the answer itself"""
    a, vertex = _audit_of_the_devices_answers(gpu_ctx, poseref.workload("C"))
    assert a["n_connected"] >= 6
    a, vertex = _audit_of_the_devices_answers(gpu_ctx, poseref.stride_tree(2049, 1))
    assert a["n_connected"] >= 4
    w = poseref.tie_duplicate(4.0, 16, 1, "above_1024")
    a, vertex = _audit_of_the_devices_answers(gpu_ctx, w)
    assert a["answer_is_argmin"] == a["n_connected"] == len(w.goals) and a["answer_within_tol"] == 0


# ------------------------------------------------------------------------------------------------ resident frames
def test_a_tree_of_one_resident_frame_is_refused_on_the_other(gpu_ctx):
    """Resident frames share one grid generation: only the grid's address tells the tree's frame from the active one."""
    grids = DeviceGrids(gpu_ctx, 96, 100, thresh=0.33, frames=2, seed=5)
    og = [np.ascontiguousarray(f != 0, dtype=np.uint8) for f in grids.host]
    assert not np.array_equal(og[0], og[1])
    free = np.argwhere(og[0] == 0)
    rng = np.random.default_rng(8)
    n, rho, nh = 400, 3.0, 16
    a, c = free[rng.integers(0, len(free), 2)]
    goals = np.column_stack([free[rng.integers(0, len(free), 12)], rng.integers(0, nh, 12)])
    w = poseref.made("frames", og[0], n, 1, 15, rho, nh, (a[0], a[1], 3), (c[0], c[1], 7), hostprep.draw_free_samples(rng, free, n), rng.integers(0, nh, n), goals)
    assert w.j > 50 and (w.vertex >= 0).sum() >= 4
    grids.select(0)
    generation = gpu_ctx.grid_generation()
    b = _ffi.Batch(gpu_ctx, 1, n, dubins=True)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert b.get_result(0).j == w.j
    _same(b.connect_poses(0, w.goals), w)
    counts = b.connect_poses_counts()
    grids.select(1)
    refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_poses, 0, w.goals)
    assert gpu_ctx.grid_generation() == generation and b.connect_poses_counts() == counts  # (the refused call ran nothing)
    grids.select(0)
    _same(b.connect_poses(0, w.goals), w)  # the tree is still there: no new launch of the query
    b.close()
