"""GPU: a finished Dubins tree kept when the map changes (rrt_pose_keep_edge_kernel, rrt_batch_keep_pose_tree / rrt_plan_keep_pose_tree,
_ffi.Batch.keep_pose_tree / Context.keep_pose_tree, RRTDubins / RRTStarDubins .keep_pose_tree / .keep_pose_tree_resident), and
connect_poses over the view it installs.

Every comparison is exact (==, array_equal): the alive bytes, n_alive (which _ffi checks against the bytes), connect_poses' vertex
and cost.  The check is posekeepref.py: every edge by the oracle's word and sweep, every vertex by its own walk to the root, then
poseref.connect on the alive vertices alone against the new map.  What makes the maps and trees worth running is asserted without a
GPU, in test_keep_pose_tree_cpu.py."""
import numpy as np
import pytest

import oracle
import poseref
import posekeepref
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.dubins import RRTStarDubins
from posecalls import planned_batch
from rrtplanner_amd.oggen import DeviceGrids
from treecalls import refused_with_word

pytestmark = pytest.mark.gpu

INF = np.inf
WORKLOADS = ["E", "D", "A", "B"]


def _same(alive, got, k):
    vertex, cost = got
    assert alive.dtype == bool and alive.shape == (k.w.j,)
    assert np.array_equal(alive, k.alive), np.flatnonzero(alive != k.alive)[:8]
    assert vertex.dtype == np.int32 and cost.dtype == np.float64
    assert np.array_equal(vertex, k.vertex), np.flatnonzero(vertex != k.vertex)[:8]
    assert np.array_equal(cost, k.cost), np.flatnonzero(cost != k.cost)[:8]


def _keep_on_a_batch(ctx, k, serial=False):
    w = k.w
    b = planned_batch(ctx, w, serial)
    ctx.set_grid(k.og8)
    _same(b.keep_pose_tree(0), b.connect_poses(0, w.goals), k)
    return b


# ------------------------------------------------------------------------------------------------ 1. the workloads, three ways
@pytest.mark.parametrize("name", WORKLOADS)
def test_workloads_on_a_batch(gpu_ctx, name):
    k = posekeepref.changed(name)
    for serial in (False, True):  # the 16-samples-per-round kernel and the one-sample kernel built the tree
        b = _keep_on_a_batch(gpu_ctx, k, serial)
        ms = b.keep_tree_ms()  # the three stages of either keep call
        assert len(ms) == 3 and all(t >= 0.0 for t in ms)
        b.close()


@pytest.mark.parametrize("name", WORKLOADS)
def test_workloads_through_rrt_plan(gpu_ctx, name):
    k = posekeepref.changed(name)
    w = k.w
    gpu_ctx.set_grid(w.og8)
    q, keep = poseref.device_query(w)
    rc, res = gpu_ctx.plan(q, w.n)
    assert rc == w.status and res.j == w.j
    gpu_ctx.set_grid(k.og8)
    refused_with_word(_ffi.RRT_E_ARG, "replaced", gpu_ctx.connect_poses, w.goals)
    _same(gpu_ctx.keep_pose_tree(), gpu_ctx.connect_poses(w.goals), k)
    assert len(gpu_ctx.keep_tree_ms()) == 3


@pytest.mark.parametrize("name", WORKLOADS)
def test_workloads_through_the_planners(name):
    k = posekeepref.changed(name)
    w = k.w
    p = poseref.planner_of(w)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j  # the planner draws the workload's stream: its tree is the oracle's
    og2 = k.og8.astype(np.int64)
    alive = p.keep_pose_tree(og2)
    vertex, cost, heading = p.connect_poses(w.goals)
    _same(alive, (vertex, cost), k)
    assert np.array_equal(heading, w.goals[:, 2]) and p.og is og2 and p._tree_resident == "device"
    # the planners' straight-line calls keep raising
    with pytest.raises(ValueError, match="Dubins"):
        p.keep_tree(og2)
    # not cumulative: the first map again restores every answer
    assert p.keep_pose_tree(w.og).all()
    v0, c0, _ = p.connect_poses(w.goals)
    assert np.array_equal(v0, w.vertex) and np.array_equal(c0, w.cost)


# ------------------------------------------------------------------------------------------------ 2. the chain
def test_a_chain_of_1100_vertices_cut_at_one_cell(gpu_ctx):
    k = posekeepref.chain_cut()
    w = k.w
    b = _keep_on_a_batch(gpu_ctx, k)
    assert not k.alive.all() and k.alive[:600].all() and not k.alive[800:].any()
    # ... and the other way round: the whole chain alive needs every round of the pointer jumping
    gpu_ctx.set_grid(w.og8)
    assert b.keep_pose_tree(0).all()
    v, c = b.connect_poses(0, w.goals)
    assert np.array_equal(v, w.vertex) and np.array_equal(c, w.cost)
    b.close()


# ------------------------------------------------------------------------------------------------ 3. a zero-length edge
def test_a_duplicate_of_the_start_pose_hangs_on_a_zero_length_edge(gpu_ctx):
    for rho, nh in poseref.TIE_PAIRS:
        for star in (0, 1):
            w = poseref.tie_duplicate(rho, nh, star, "first")
            assert w.dup == 1 and w.ro.parent[1] == 0 and w.ro.vcost[1] == 0.0
            whole = posekeepref.kept(w, w.og8)
            assert whole.alive.all()
            b = _keep_on_a_batch(gpu_ctx, whole)
            cut = posekeepref.kept(w, posekeepref.blocks_map(w.og8, w.xs))
            assert cut.alive[1] and 0 < cut.alive.sum() < w.j
            gpu_ctx.set_grid(cut.og8)
            _same(b.keep_pose_tree(0), b.connect_poses(0, w.goals), cut)
            b.close()


# ------------------------------------------------------------------------------------------------ 4. trees around the strides
@pytest.mark.parametrize("j", posekeepref.STRIDE_KEEP_J)
def test_tree_sizes_around_the_lane_wave_and_workgroup_edges(gpu_ctx, j):
    for star in (0, 1):
        k = posekeepref.stride_cut(j, star)
        assert k.w.j == j
        b = _keep_on_a_batch(gpu_ctx, k)
        whole = posekeepref.kept(k.w, k.w.og8)
        gpu_ctx.set_grid(whole.og8)
        _same(b.keep_pose_tree(0), b.connect_poses(0, k.w.goals), whole)
        b.close()


# ------------------------------------------------------------------------------------------------ 5. one heading, and 256
@pytest.mark.parametrize("name", ["G1", "G256"])
def test_one_heading_and_as_many_as_a_byte_holds(gpu_ctx, name):
    k = posekeepref.changed(name)
    assert 0 < k.alive.sum() < k.w.j and (k.vertex >= 0).any()
    _keep_on_a_batch(gpu_ctx, k).close()


# ------------------------------------------------------------------------------------------------ 6. the root blocked
def test_a_blocked_root_leaves_nothing(gpu_ctx):
    k = posekeepref.root_blocked(poseref.workload("E"))
    assert not k.alive.any() and np.all(k.vertex == -1) and np.all(k.cost == INF)
    b = _keep_on_a_batch(gpu_ctx, k)
    assert b.connect_poses_counts() == (0, 0)
    b.close()


# ------------------------------------------------------------------------------------------------ 7. back to the first map
def test_keeping_the_tree_for_the_first_map_again_restores_every_answer(gpu_ctx):
    k = posekeepref.changed("A")
    w = k.w
    b = planned_batch(gpu_ctx, w)
    first = b.connect_poses(0, w.goals)
    before = b.get_result(0)
    gpu_ctx.set_grid(k.og8)
    cut = b.keep_pose_tree(0)
    _same(cut, b.connect_poses(0, w.goals), k)
    gpu_ctx.set_grid(w.og8)
    assert b.keep_pose_tree(0).all()
    again = b.connect_poses(0, w.goals)
    for x, y in zip(first, again):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert np.array_equal(again[0], w.vertex) and np.array_equal(again[1], w.cost)
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), cut)  # not cumulative in either direction
    after = b.get_result(0)  # the tree arrays are never written
    for name in ("pts", "vcost", "parent", "head"):
        assert np.array_equal(getattr(before, name), getattr(after, name))
    # rearm drops the view: the query is unfinished, then runs again on the new map and answers over its whole new tree
    b.rearm()
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.keep_pose_tree, 0)
    refused_with_word(_ffi.RRT_E_ARG, "not finished", b.connect_poses, 0, w.goals)
    b.launch()
    b.sync()
    new = b.get_result(0)
    st, ro = oracle.dubins_plan(k.og8, w.n, w.star, w.xs, w.xg, w.samples, w.heads, r2_rewire=w.r2, rho=w.rho, nh=w.nh, logs=False)
    assert new.j == ro.j and np.array_equal(new.parent[:ro.j], ro.parent[:ro.j])
    v, c, _ = poseref.connect(k.og8, ro.pts, ro.head, ro.vcost, ro.j, w.goals, w.rho, w.nh)
    got = b.connect_poses(0, w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1], c)
    b.close()


# ------------------------------------------------------------------------------------------------ 8. a batch of three queries
def test_one_query_of_a_batch_is_kept_and_the_others_stay_refused(gpu_ctx):
    w = poseref.workload("E")
    og2 = posekeepref.blocks_map(w.og8, w.xs)
    gpu_ctx.set_grid(w.og8)
    free = np.argwhere(w.og8 == 0)
    par = [(2.0, 16, 1, 250), (3.0, 8, 0, 200), (2.5, 64, 1, 300)]  # rho, nh, star, n
    b = _ffi.Batch(gpu_ctx, 3, 300, dubins=True)
    keeps, made = [], []
    for q, (rho, nh, star, n) in enumerate(par):
        rng = np.random.default_rng(60 + q)
        samples, heads = hostprep.draw_free_samples(rng, free, n), rng.integers(0, nh, n)
        xs, xg = (w.xs[0], w.xs[1], q % nh), (w.xg[0], w.xg[1], (3 + q) % nh)
        goals = np.column_stack([free[rng.integers(0, len(free), 10)], rng.integers(0, nh, 10)])
        m = poseref.made(f"three {q}", w.og8, n, star, 12, rho, nh, xs, xg, samples, heads, goals)
        made.append(m)
        qu, keep = poseref.device_query(m)
        keeps.append(keep)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    for q, m in enumerate(made):
        assert b.get_result(q).j == m.j > 30
    gpu_ctx.set_grid(og2)
    for q, m in enumerate(made):
        refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_poses, q, m.goals)
    ks = [posekeepref.kept(m, og2) for m in made]
    _same(b.keep_pose_tree(1), b.connect_poses(1, made[1].goals), ks[1])
    assert 0 < ks[1].alive.sum() < made[1].j
    for q in (0, 2):
        refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_poses, q, made[q].goals)
    # a second query kept next to the first: each has its own view
    _same(b.keep_pose_tree(2), b.connect_poses(2, made[2].goals), ks[2])
    v, c = b.connect_poses(1, made[1].goals)
    assert np.array_equal(v, ks[1].vertex) and np.array_equal(c, ks[1].cost)
    refused_with_word(_ffi.RRT_E_ARG, "replaced", b.connect_poses, 0, made[0].goals)
    _same(b.keep_pose_tree(0), b.connect_poses(0, made[0].goals), ks[0])
    b.close()


# ------------------------------------------------------------------------------------------------ 9. resident frames
def test_two_resident_frames(gpu_ctx):
    grids = DeviceGrids(gpu_ctx, 96, 100, thresh=0.33, frames=2, seed=5)
    og = [np.ascontiguousarray(f != 0, dtype=np.uint8) for f in grids.host]
    both = np.argwhere((og[0] == 0) & (og[1] == 0))
    free = np.argwhere(og[0] == 0)
    rng = np.random.default_rng(8)
    n, rho, nh = 400, 3.0, 16
    a, c = both[rng.integers(0, len(both), 2)]
    goals = np.column_stack([both[rng.integers(0, len(both), 12)], rng.integers(0, nh, 12)])
    w = poseref.made("frames", og[0], n, 1, 15, rho, nh, (a[0], a[1], 3), (c[0], c[1], 7), hostprep.draw_free_samples(rng, free, n), rng.integers(0, nh, n), goals)
    k = posekeepref.kept(w, og[1])
    assert w.j > 50 and 0 < k.alive.sum() < w.j
    grids.select(0)
    generation = gpu_ctx.grid_generation()
    b = _ffi.Batch(gpu_ctx, 1, n, dubins=True)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert b.get_result(0).j == w.j
    _same(b.keep_pose_tree_resident(grids, 1), b.connect_poses(0, w.goals), k)
    assert gpu_ctx.grid_generation() == generation  # nothing was uploaded
    assert b.keep_pose_tree_resident(grids, 0).all()
    v, cst = b.connect_poses(0, w.goals)
    assert np.array_equal(v, w.vertex) and np.array_equal(cst, w.cost)
    b.close()


def test_the_planner_keeps_its_tree_on_the_next_resident_frame():
    w = poseref.workload("A")
    W, H = w.og8.shape
    p = RRTStarDubins(w.og, 500, 20, w.rho, n_headings=w.nh, pbar=False, seed=3)
    grids = DeviceGrids(p.device_context(), W, H, thresh=0.33, frames=2, seed=5)
    og = [np.ascontiguousarray(f != 0, dtype=np.uint8) for f in grids.host]
    both = np.argwhere((og[0] == 0) & (og[1] == 0))
    rng = np.random.default_rng(9)
    a, c = both[rng.integers(0, len(both), 2)]
    p.set_og_resident(grids, 0)
    xs, xg = (int(a[0]), int(a[1]), 3), (int(c[0]), int(c[1]), 7)
    try:
        T, gv = p.plan(np.array(xs), np.array(xg))
    except IndexError:  # (the planner's own goal unreachable: the tree is complete all the same)
        pass
    ctx = p.device_context()
    j = _ffi.C.c_int32(0)
    assert _ffi.lib().rrt_plan_tree_size(ctx.handle, _ffi.C.byref(j)) == _ffi.RRT_OK
    j = j.value
    # the tree from the oracle, on the planner's stream
    rng = np.random.default_rng(3)
    free = np.argwhere(og[0] == 0)
    samples = hostprep.draw_free_samples(rng, free, 500)
    heads = rng.integers(0, w.nh, 500)
    goals = np.column_stack([both[np.random.default_rng(10).integers(0, len(both), 12)], np.random.default_rng(11).integers(0, w.nh, 12)])
    m = poseref.made("planner frames", og[0], 500, 1, 20, w.rho, w.nh, xs, xg, samples, heads, goals)
    assert m.j == j > 50
    k = posekeepref.kept(m, og[1])
    assert 0 < k.alive.sum() < j
    alive = p.keep_pose_tree_resident(grids, 1)
    assert grids.valid() and np.shares_memory(p.og, grids.host[1])  # nothing was uploaded
    vertex, cost, _ = p.connect_poses(goals)
    _same(alive, (vertex, cost), k)
    assert p.keep_pose_tree_resident(grids, 0).all()


# ------------------------------------------------------------------------------------------------ 10. routes after a keep
def test_paths_to_poses_after_a_keep_stay_on_alive_vertices_and_free_legs():
    k = posekeepref.changed("A")
    w = k.w
    p = poseref.planner_of(w)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    og2 = k.og8.astype(np.int64)
    alive = p.keep_pose_tree(og2)
    assert np.array_equal(alive, k.alive)
    routes = p.paths_to_poses(T, w.goals)
    assert [r is None for r in routes] == (k.vertex < 0).tolist() and sum(r is not None for r in routes) >= 8
    for r, v in zip(routes, k.vertex.tolist()):
        if r is None:
            continue
        ids = p.route2gv(T, v)
        assert ids[0] == 0 and ids[-1] == v and alive[ids].all() and len(r) == len(ids) + 1
        for a, b in zip(r[:-1], r[1:]):  # every leg, the one to the goal pose included, by the oracle's word and sweep on the new map
            th0, th1 = poseref.theta(a[2], w.nh), poseref.theta(b[2], w.nh)
            length = oracle.dub_shortest(float(a[0]), float(a[1]), th0, float(b[0]), float(b[1]), th1, w.rho)[3]
            cells = oracle.dub_sweep_cells(int(a[0]), int(a[1]), th0, int(b[0]), int(b[1]), th1, w.rho, cap=int(length / 0.5) + 16)
            assert np.isfinite(length) and not np.any(k.og8[cells[:, 0], cells[:, 1]] != 0) and k.og8[b[0], b[1]] == 0
        line = p.poses_polyline(r)
        assert line.ndim == 2 and line.shape[1] == 2


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_refusals_in_their_order():
    w = poseref.workload("E")
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    L = _ffi.lib()
    n_alive = _ffi.C.c_int32(0)
    refused_with_word(_ffi.RRT_E_ARG, "no rrt_plan", ctx.keep_pose_tree)
    assert L.rrt_plan_keep_pose_tree(None, _ffi.C.byref(n_alive), None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_keep_pose_tree(ctx.handle, _ffi.C.byref(n_alive), None) == _ffi.RRT_E_ARG
    assert L.rrt_last_error_string(ctx.handle).decode().startswith("rrt_plan_keep_pose_tree: query 0 has not finished (no rrt_plan")
    # a straight-line batch: NULL first, then the kind of batch, before q is looked at
    s = _ffi.Batch(ctx, 1, w.n)
    assert L.rrt_batch_keep_pose_tree(None, 0, _ffi.C.byref(n_alive), None) == _ffi.RRT_E_ARG
    assert L.rrt_batch_keep_pose_tree(s._h, 7, None, None) == _ffi.RRT_E_ARG
    assert L.rrt_last_error_string(ctx.handle).decode() == "rrt_batch_keep_pose_tree: NULL"
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "rrt_batch_keep_pose_tree: not a Dubins batch (its edges are straight lines: use rrt_batch_keep_tree)", s.keep_pose_tree, 7)
    q, keep = _ffi.make_query(1, w.n, w.xs[:2], w.xg[:2], w.samples, r2_rewire=w.r2)
    s.set_query(0, q)
    s.launch()
    s.sync()
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "use rrt_batch_keep_tree", s.keep_pose_tree, 0)
    assert s.keep_tree(0).all()  # its own call
    s.close()
    # a Dubins batch: q, then the state of the query, then the grid's shape
    b = _ffi.Batch(ctx, 2, w.n, dubins=True)
    other = np.zeros((w.og8.shape[0] + 8, w.og8.shape[1]), dtype=np.uint8)
    ctx.set_grid(other)
    refused_with_word(_ffi.RRT_E_ARG, "rrt_batch_keep_pose_tree: q=2 of 2", b.keep_pose_tree, 2)
    refused_with_word(_ffi.RRT_E_ARG, "q=-1", b.keep_pose_tree, -1)
    refused_with_word(_ffi.RRT_E_ARG, "rrt_batch_keep_pose_tree: query 0 has not finished (no query set)", b.keep_pose_tree, 0)
    ctx.set_grid(w.og8)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    refused_with_word(_ffi.RRT_E_ARG, "not launched", b.keep_pose_tree, 0)
    refused_with_word(_ffi.RRT_E_ARG, "no rrt_batch_keep_tree", b.keep_tree_ms)
    b.launch()
    b.sync()
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.keep_pose_tree, 1)
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "rrt_batch_keep_tree: a Dubins batch (its edges are Dubins words between poses; these kernels test straight lines)",
             b.keep_tree, 0)  # word for word what it was
    assert L.rrt_batch_keep_pose_tree(b._h, 0, _ffi.C.byref(n_alive), None) == _ffi.RRT_OK and n_alive.value == w.j  # no flags wanted
    want = b.connect_poses(0, w.goals)
    assert np.array_equal(want[0], w.vertex) and np.array_equal(want[1], w.cost)
    ctx.set_grid(other)
    refused_with_word(_ffi.RRT_E_ARG, "rrt_batch_keep_pose_tree: the context's grid has another shape than the batch was created for", b.keep_pose_tree, 0)
    refused_with_word(_ffi.RRT_E_ARG, "no query set", b.keep_pose_tree, 1)  # (the query's state before the grid's shape)
    # the refusals changed nothing: back on a grid of the batch's shape the query is kept
    k = posekeepref.changed("E")
    ctx.set_grid(k.og8)
    _same(b.keep_pose_tree(0), b.connect_poses(0, w.goals), k)
    ms = b.keep_tree_ms()
    assert len(ms) == 3 and all(t >= 0.0 for t in ms)
    # a set_query in a kept query's place drops its view with its tree
    b.set_query(0, q)
    refused_with_word(_ffi.RRT_E_ARG, "not launched", b.connect_poses, 0, w.goals)
    b.close()
    ctx.close()
