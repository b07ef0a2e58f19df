"""GPU: a finished Dubins tree grown with new pose samples (rrt_pose_seed_heading_kernel behind the seed kernels of rrt_seed.h,
rrt_batch_grow_poses / rrt_plan_grow_poses, _ffi.Batch.grow_poses / Context.grow_poses, RRTDubins / RRTStarDubins .grow_poses) on both
Dubins kernels, and connect_poses / pose_routes / keep_pose_tree on the grown tree.

Every comparison is exact (==, array_equal, costs as raw bits).  The check is posegrowref.py -- posekeepref's alive vertices as the
seed, the loop over the oracle's words and sweeps, poseref's goal decision -- and, where nothing was cut, oracle/dubins_ref.c's audit
of the grown tree over the concatenated stream.  What makes the workloads worth running is asserted without a GPU, in
test_grow_poses_cpu.py."""
import ctypes
import functools

import numpy as np
import pytest

import oracle
import posegrowref
import posekeepref
import poseref
import poseroutesref
from posecalls import GROW_KERNELS, assert_audit_clean, grow_poses_checked, planned_logged_batch
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.dubins import RRTStarDubins
from treecalls import refused_with_word, tree_of

pytestmark = pytest.mark.gpu

WORKLOADS = ["A", "D", "E", "G1", "G256"]
STRIDE_J0 = (1, 2, 63, 64, 65, 1023, 1024, 1025)
STRIDE_PAD = (71, 10)  # a cell of poseref._stride_map()'s wall


def _poses_and_routes(b, q, og8, w, g, goals, connected=4):
    """connect_poses and pose_routes(points=True) of query q on the grown tree against poseref / poseroutesref over g's arrays"""
    v, c, _ = poseref.connect(og8, g.pts, g.head, g.vcost, g.j, goals, w.rho, w.nh)
    got = b.connect_poses(q, goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1].view(np.int64), c.view(np.int64)) and (v >= 0).sum() >= connected
    want = poseroutesref.routes(g.pts, g.head, g.parent, g.j, goals, v, c, w.rho, w.nh)
    poseroutesref.same(b.pose_routes(q, goals, points=True), want)


@functools.lru_cache(maxsize=None)
def _uncut_a():
    w = poseref.workload("A")
    s = posegrowref.more_poses(w, w.og8, 600, seed=posegrowref.UNCUT_A_SEED)
    return w, s, posegrowref.grow_workload(w, w.og8, None, s)


# ------------------------------------------------------------------------------------------------ 1. the cut workloads, planted streams
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
@pytest.mark.parametrize("name", WORKLOADS)
def test_a_kept_tree_grows_back_behind_the_blocks(gpu_ctx, name, kernel):
    k, s, _, _, _, g = posegrowref.planted(name)
    w = k.w
    b = planned_logged_batch(gpu_ctx, w, kernel)
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive)
    grow_poses_checked(b, 0, w, g, g.ids, s, kernel)
    if name == "A":
        _poses_and_routes(b, 0, k.og8, w, g, w.goals)
    b.close()


# ------------------------------------------------------------------------------------------------ 2. nothing cut, more than a ring
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_an_uncut_tree_grown_by_600_samples_is_audited(gpu_ctx, kernel):
    w, s, g = _uncut_a()
    assert g.j0 % 128 != 0 and len(s) == 600 > 128 and g.j > g.j0 + 64  # more than DB_RING samples from a j0 that is no multiple of it
    b = planned_logged_batch(gpu_ctx, w, kernel)
    res = grow_poses_checked(b, 0, w, g, np.arange(w.j), s, kernel)
    _poses_and_routes(b, 0, w.og8, w, g, w.goals)
    a = oracle.dubins_audit(w.og8, w.n + 600, w.star, np.concatenate([w.samples, s[:, :2]]), np.concatenate([w.heads, s[:, 2]]), res.pts, res.head, res.vcost,
                            res.parent, res.j, r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    assert a["n_accepted"] == res.j - 1
    assert_audit_clean(a, w.star)
    b.close()


# ------------------------------------------------------------------------------------------------ 3. seeds around the strides
@pytest.mark.parametrize("j0", STRIDE_J0)
def test_seeds_around_the_lane_wave_and_workgroup_edges(gpu_ctx, j0):
    for star in (0, 1):
        w = poseref.stride_tree(j0, star)
        assert w.j == j0
        stream = posegrowref.accepted_stream(w, STRIDE_PAD, 48)
        s = posegrowref.more_poses(w, w.og8, 40, seed=j0)
        g = posegrowref.grow_workload(w, w.og8, None, s, n=stream[2])
        assert g.j0 == j0 and (g.j > g.j0 or j0 == 1)
        for kernel in GROW_KERNELS:
            b = planned_logged_batch(gpu_ctx, w, kernel, stream=stream)
            grow_poses_checked(b, 0, w, g, np.arange(j0), s, kernel)
            b.close()


def test_a_cut_stride_tree_across_a_workgroup_of_the_seed_kernels(gpu_ctx):
    """the seed with a view of more than 256 vertices on both sides of the cut (SEED_TPB lanes a workgroup)"""
    k = posekeepref.stride_cut(1025, 1)
    w = k.w
    assert k.alive.sum() > 256 and (~k.alive).sum() > 64
    stream = posegrowref.accepted_stream(w, STRIDE_PAD, 48)
    s = posegrowref.more_poses(w, k.og8, 40, seed=3)
    g = posegrowref.grow_workload(w, k.og8, k.alive, s, n=stream[2])
    for kernel in GROW_KERNELS:
        b = planned_logged_batch(gpu_ctx, w, kernel, stream=stream)
        gpu_ctx.set_grid(k.og8)
        assert np.array_equal(b.keep_pose_tree(0), k.alive)
        grow_poses_checked(b, 0, w, g, g.ids, s, kernel)
        b.close()


# ------------------------------------------------------------------------------------------------ 4. no sample, one sample
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
@pytest.mark.parametrize("m", [0, 1])
def test_no_sample_is_go2goal_alone_and_one_sample(gpu_ctx, m, kernel):
    k = posekeepref.changed("E")
    w = k.w
    s = posegrowref.planted_stream(k)[0]
    first = int(np.flatnonzero(posegrowref.planted("E")[5].accept_log)[0])  # a sample the seed accepts
    s = s[first:first + m]
    g = posegrowref.grow_workload(w, k.og8, k.alive, s)
    assert g.j == g.j0 + m
    b = planned_logged_batch(gpu_ctx, w, kernel)
    gpu_ctx.set_grid(k.og8)
    b.keep_pose_tree(0)
    res = grow_poses_checked(b, 0, w, g, g.ids, s, kernel)
    assert (res.sum_j, res.sum_near) == ((0, 0) if m == 0 else (g.j0, g.sum_near))
    b.close()


# ------------------------------------------------------------------------------------------------ 5. the query filled exactly
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_a_stream_that_fills_the_query_exactly(gpu_ctx, kernel):
    w, s = posegrowref.fill_exactly()
    assert w.j == posegrowref.FILL_J and w.j + len(s) == w.n
    full = posegrowref.grow_workload(w, w.og8, None, s)
    assert full.accept_log.all() and full.j == w.n and not full.found and full.status == posegrowref.ST_OK and full.vgoal == 0
    short = posegrowref.grow_workload(w, w.og8, None, s[:-1])
    assert short.j == w.n - 1 and not short.found and short.status == posegrowref.ST_UNREACHABLE  # the fall-back goes by the query's own n
    for g, stream in ((full, s), (short, s[:-1])):
        b = planned_logged_batch(gpu_ctx, w, kernel)
        res = grow_poses_checked(b, 0, w, g, np.arange(w.j), stream, kernel)
        assert res.status == (_ffi.RRT_OK if g is full else _ffi.RRT_E_GOAL_UNREACHABLE)
        if g is full:
            refused_with_word(_ffi.RRT_E_ARG, "room for 0", b.grow_poses, 0, s[:1])
            j0, _, _ = b.grow_poses(0, s[:0])  # ... and none is asked for: go2goal alone, on a full tree
            assert j0 == w.n
            b.launch()
            b.sync()
            assert b.get_result(0).j == w.n
        b.close()


# ------------------------------------------------------------------------------------------------ 6. the root blocked
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_a_blocked_root_is_refused_and_the_tree_stays(gpu_ctx, kernel):
    w = poseref.workload("E")
    k = posekeepref.root_blocked(w)
    b = planned_logged_batch(gpu_ctx, w, kernel)
    before = b.get_result(0)
    gpu_ctx.set_grid(k.og8)
    assert not b.keep_pose_tree(0).any()
    refused_with_word(_ffi.RRT_E_ARG, "rrt_batch_grow_poses: no vertex of query 0 is alive", b.grow_poses, 0, posegrowref.more_poses(w, k.og8, 5))
    after = b.get_result(0)
    for name in ("pts", "vcost", "parent", "head"):
        assert np.array_equal(getattr(before, name), getattr(after, name))
    assert (after.status, after.j, after.found, after.vgoal) == (before.status, before.j, before.found, before.vgoal)
    gpu_ctx.set_grid(w.og8)  # the first map again: every vertex is back, and the tree grows
    assert b.keep_pose_tree(0).all()
    s = posegrowref.more_poses(w, w.og8, 30)
    grow_poses_checked(b, 0, w, posegrowref.grow_workload(w, w.og8, None, s), np.arange(w.j), s, kernel)
    b.close()


# ------------------------------------------------------------------------------------------------ 7. grown twice; kept, grown, kept, grown
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_two_grows_in_a_row(gpu_ctx, kernel):
    w = poseref.workload("E")
    s1, s2 = posegrowref.more_poses(w, w.og8, 50, seed=41), posegrowref.more_poses(w, w.og8, 50, seed=42)
    g1 = posegrowref.grow_workload(w, w.og8, None, s1)
    pts, head, parent, vcost, j = tree_of(g1)
    ids, sp, sh, sc, spar = posegrowref.seed(pts, head, parent, vcost, j)
    g2 = posegrowref.grow(w.og8, w.star, w.n, w.xg, w.r2, w.rho, w.nh, sp, sh, sc, spar, s2)
    assert g1.j > g1.j0 and g2.j0 == g1.j and g2.j > g2.j0
    b = planned_logged_batch(gpu_ctx, w, kernel)
    grow_poses_checked(b, 0, w, g1, np.arange(w.j), s1, kernel)
    grow_poses_checked(b, 0, w, g2, ids, s2, kernel)
    b.close()


@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_kept_grown_kept_on_a_third_map_and_grown(gpu_ctx, kernel):
    k, s1, _, _, _, g1 = posegrowref.planted("A")
    w = k.w
    og3 = posekeepref.blocks_map(w.og8, w.xs, seed=8)
    pts, head, parent, vcost, j = tree_of(g1)
    alive3 = posekeepref.alive(og3, pts, head, parent, j, w.rho, w.nh)
    ids, sp, sh, sc, spar = posegrowref.seed(pts, head, parent, vcost, j, alive3)
    s2 = posegrowref.more_poses(w, og3, j - len(ids), seed=43)
    g2 = posegrowref.grow(og3, w.star, w.n, w.xg, w.r2, w.rho, w.nh, sp, sh, sc, spar, s2)
    assert 8 < len(ids) < j - 8 and g2.j > g2.j0 and not np.array_equal(og3, k.og8)
    b = planned_logged_batch(gpu_ctx, w, kernel)
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive)
    grow_poses_checked(b, 0, w, g1, g1.ids, s1, kernel)
    gpu_ctx.set_grid(og3)
    refused_with_word(_ffi.RRT_E_ARG, "not kept on it (rrt_batch_keep_pose_tree)", b.grow_poses, 0, s2)
    assert np.array_equal(b.keep_pose_tree(0), alive3)
    grow_poses_checked(b, 0, w, g2, ids, s2, kernel)
    _poses_and_routes(b, 0, og3, w, g2, w.goals, connected=1)
    b.close()


# ------------------------------------------------------------------------------------------------ 8. one query of three
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_one_query_of_three_grows_and_the_others_stay(gpu_ctx, kernel):
    k, s, _, _, _, g = posegrowref.planted("E")
    w = k.w
    b = planned_logged_batch(gpu_ctx, w, kernel, Q=3)
    before = [b.get_result(q) for q in range(3)]
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(1), k.alive)
    grow_poses_checked(b, 1, w, g, g.ids, s, kernel)
    for q in (0, 2):
        after = b.get_result(q)
        for name in ("pts", "vcost", "parent", "head", "nearest_log", "accept_log", "j_log"):
            assert np.array_equal(getattr(before[q], name), getattr(after, name)), (q, name)
        assert (after.status, after.j, after.found, after.vgoal, after.sum_j) == (before[q].status, before[q].j, before[q].found, before[q].vgoal, before[q].sum_j)
    b.close()


# ------------------------------------------------------------------------------------------------ 9. the seed belongs to its grid
def test_a_launch_after_set_grid_on_another_map_is_refused_and_rearm_lifts_it(gpu_ctx):
    k = posekeepref.changed("E")
    w = k.w
    b = planned_logged_batch(gpu_ctx, w, "block")
    s = posegrowref.more_poses(w, w.og8, 40)
    j0, _, _ = b.grow_poses(0, s)
    gpu_ctx.set_grid(k.og8)
    refused_with_word(_ffi.RRT_E_ARG, "seeded by rrt_batch_grow", b.launch)
    b.rearm()  # drops the grow: the query runs again from its sample buffer as it then stands, rows [j0, j0 + m) replaced
    b.launch()
    b.sync()
    res = b.get_result(0)
    samples, heads = np.array(w.samples), np.array(w.heads)
    samples[j0:j0 + 40], heads[j0:j0 + 40] = s[:, :2], s[:, 2]
    st, ro = oracle.dubins_plan(k.og8, w.n, w.star, w.xs, w.xg, samples, heads, r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    assert res.status == st and res.j == ro.j and np.array_equal(res.parent[:ro.j], ro.parent[:ro.j]) and np.array_equal(res.head[:ro.j], ro.head[:ro.j])
    assert np.array_equal(res.accept_log, ro.accept_log)
    b.close()


# ------------------------------------------------------------------------------------------------ 10. refusals
def _raw(b, q, s, m):
    j0, log0 = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _ffi._check(b.ctx.handle, _ffi.lib().rrt_batch_grow_poses(b._h, q, s.ctypes.data, m, ctypes.byref(j0), None, ctypes.byref(log0)))


def test_refusals_name_the_call_and_change_nothing(gpu_ctx):
    w = poseref.workload("E")
    W, H = w.og8.shape
    b = planned_logged_batch(gpu_ctx, w, "block")
    before = b.get_result(0)
    ok = posegrowref.more_poses(w, w.og8, 4)
    who = "rrt_batch_grow_poses: "
    bad = ok.copy()
    bad[2, 2] = w.nh
    refused_with_word(_ffi.RRT_E_ARG, who + f"sample 2 has heading {w.nh}, query 0 has headings [0, {w.nh})", b.grow_poses, 0, bad)
    bad[2, 2] = -1
    refused_with_word(_ffi.RRT_E_ARG, who + "sample 2 has heading -1", b.grow_poses, 0, bad)
    bad = ok.copy()
    bad[1, 0] = W
    refused_with_word(_ffi.RRT_E_ARG, who + f"sample 1 = ({W}, {bad[1, 1]}) outside the {W}x{H} grid", b.grow_poses, 0, bad)
    refused_with_word(_ffi.RRT_E_ARG, who + "m=-1", _raw, b, 0, np.ascontiguousarray(ok, dtype=np.int32), -1)
    room = w.n - w.j
    refused_with_word(_ffi.RRT_E_ARG, who + f"{w.j} vertices and m={room + 1} samples exceed the query's n={w.n}: room for {room}", b.grow_poses, 0, posegrowref.more_poses(w, w.og8, room + 1))
    refused_with_word(_ffi.RRT_E_ARG, who + "q=1 of 1", b.grow_poses, 1, ok)
    # the straight-line call keeps its answer for a Dubins batch
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, "rrt_batch_grow: a Dubins batch (the seed kernels carry no headings)", b.grow, 0, ok[:, :2])
    gpu_ctx.set_grid(np.zeros((W + 1, H), dtype=np.uint8))
    refused_with_word(_ffi.RRT_E_ARG, who + "the context's grid changed shape since the batch was created", b.grow_poses, 0, ok)
    gpu_ctx.set_grid(w.og8)
    refused_with_word(_ffi.RRT_E_ARG, "not kept on it (rrt_batch_keep_pose_tree)", b.grow_poses, 0, ok)  # the same cells, another generation
    assert b.keep_pose_tree(0).all()
    after = b.get_result(0)
    for name in ("pts", "vcost", "parent", "head"):
        assert np.array_equal(getattr(before, name), getattr(after, name))
    assert (after.status, after.j, after.found, after.vgoal) == (before.status, before.j, before.found, before.vgoal)
    v, c = b.connect_poses(0, w.goals)  # ... and the view of the last keep still answers
    assert np.array_equal(v, w.vertex) and np.array_equal(c, w.cost)
    b.close()
    # an unfinished query, and a batch that is not a Dubins batch
    u = _ffi.Batch(gpu_ctx, 1, w.n, dubins=True)
    qu, keep = poseref.device_query(w)
    u.set_query(0, qu)
    refused_with_word(_ffi.RRT_E_ARG, who + "query 0 has not finished", u.grow_poses, 0, ok)
    u.close()
    p = _ffi.Batch(gpu_ctx, 1, 100)
    refused_with_word(_ffi.RRT_E_UNSUPPORTED, who + "not a Dubins batch (its samples are cells and its edges straight lines: use rrt_batch_grow)", p.grow_poses, 0, ok)
    p.close()


def test_through_rrt_plan(gpu_ctx):
    k, s, _, _, _, g = posegrowref.planted("D")  # RRTDubins: the planner without a near set
    w = k.w
    gpu_ctx.set_grid(w.og8)
    qu, keep = poseref.device_query(w)
    rc, res = gpu_ctx.plan(qu, w.n)
    assert rc == w.status and res.j == w.j
    gpu_ctx.set_grid(k.og8)
    with pytest.raises(_ffi.RRTError) as e:
        gpu_ctx.grow_poses(s, w.n)
    assert e.value.code == _ffi.RRT_E_ARG and "rrt_plan_grow_poses: " in str(e.value) and "rrt_batch_keep_pose_tree" in str(e.value) and not e.value.seeded
    assert np.array_equal(gpu_ctx.keep_pose_tree(), k.alive)
    rc, res, j0, old_id = gpu_ctx.grow_poses(s, w.n, logs=False)
    assert rc == g.status and j0 == g.j0 and np.array_equal(old_id, g.ids)
    live = g.j + g.found
    assert (res.j, res.found, res.vgoal) == (g.j, g.found, g.vgoal) and np.array_equal(res.parent[:live], g.parent[:live])
    assert np.array_equal(res.head[:live], g.head[:live]) and np.array_equal(res.vcost[:live].view(np.int64), g.vcost[:live].view(np.int64))
    assert len(gpu_ctx.grow_ms()) == 3
    v, c, _ = poseref.connect(k.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    got = gpu_ctx.connect_poses(w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1], c)


# ------------------------------------------------------------------------------------------------ 11. the planner classes
def test_a_seeded_rrtstardubins_plans_keeps_and_grows():
    k = posekeepref.changed("E")
    w = k.w
    r, seed = poseref.SPECS["E"][4], poseref.SPECS["E"][7]
    p = RRTStarDubins(w.og, w.n, r, w.rho, n_headings=w.nh, pbar=False, seed=seed)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j and p._grow_j0 == w.j
    og2 = k.og8.astype(np.int64)
    assert np.array_equal(p.keep_pose_tree(og2), k.alive) and p._grow_j0 == int(k.alive.sum())
    m = int((~k.alive).sum())
    rng = np.random.default_rng(seed)  # a generator in the planner's state: plan() drew n cells and n headings
    hostprep.draw_free_samples(rng, np.argwhere(w.og8 == 0), w.n)
    rng.integers(0, w.nh, w.n)
    cells = hostprep.draw_free_samples(rng, np.argwhere(og2 == 0), m)
    s = np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), rng.integers(0, w.nh, m)])
    g = posegrowref.grow_workload(w, k.og8, k.alive, s)
    assert g.j > g.j0 and g.found
    with pytest.raises(ValueError, match=f"room for {w.n - g.j0} more samples"):
        p.grow_poses(w.n - g.j0 + 1)
    T, gv = p.grow_poses(m)
    assert gv == g.vgoal and np.array_equal(p.last_grow_ids, g.ids) and p._grow_j0 == g.j and p._tree_resident == "device"
    assert (p.last_stats["j"], p.last_stats["sum_j"], p.last_stats["sum_near"]) == (g.j, g.sum_j, g.sum_near)
    live = g.j + 1
    assert T.number_of_nodes() == w.n + 1 and T.number_of_edges() == g.j
    for v in range(live):
        assert tuple(T.nodes[v]["pt"]) == tuple(g.pts[v]) and T.nodes[v]["heading"] == g.head[v], v
    assert tuple(T.nodes[w.n]["pt"]) == w.xg[:2] and T.nodes[w.n]["heading"] == w.xg[2]
    for u, v, d in T.edges(data=True):
        assert u == g.parent[v] and d["cost"] == g.vcost[v], (u, v)
        length = oracle.dub_shortest(float(g.pts[u, 0]), float(g.pts[u, 1]), poseref.theta(g.head[u], w.nh), float(g.pts[v, 0]), float(g.pts[v, 1]),
                                     poseref.theta(g.head[v], w.nh), w.rho)[3]
        assert abs(d["dist"] - length) < 1e-9 * (1.0 + length)  # (the host's libm words: dubins.py's head comment)
    # the pose calls work on the grown tree in its new numbering, and it is kept and grown again
    v, c, _ = poseref.connect(k.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    pv, pc, ph = p.connect_poses(w.goals)
    assert np.array_equal(pv, v) and np.array_equal(pc, c)
    routes, length = p.routes_to_poses(w.goals)
    paths = p.paths_to_poses(T, w.goals)
    for e in range(len(w.goals)):
        assert (routes[e] is None) == (v[e] < 0) == (paths[e] is None)
        if v[e] >= 0:
            assert np.array_equal(routes[e], paths[e]) and length[e] == c[e]
    assert p.keep_pose_tree(og2).all()  # every edge of the grown tree was accepted on this map
    T2, gv2 = p.grow_poses(5)
    assert p.last_stats["j"] >= g.j and np.array_equal(p.last_grow_ids, np.arange(g.j))
