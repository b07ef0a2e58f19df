"""CPU: the restatement of grow_poses (posegrowref.py) pinned to the oracle, the conditions that make the GPU comparisons of
test_grow_poses_gpu.py worth something -- asserted on the restatement alone --, the binding, and the planners' refusals before any
device call."""
import ctypes

import numpy as np
import pytest

import oracle
import posegrowref
import posekeepref
import poseref
from posecalls import assert_audit_clean
from rrtplanner_amd import _ffi
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

WORKLOADS = ["A", "D", "E", "G1", "G256"]


# ------------------------------------------------------------------------------------------------ a grown uncut tree IS the longer plan
@pytest.mark.parametrize("name", WORKLOADS)
def test_an_uncut_tree_grown_is_the_oracles_plan_of_the_longer_stream(name):
    w = poseref.workload(name)
    m = min(w.n - w.j, 300)
    assert m >= 100 and w.j > 64
    s = posegrowref.more_poses(w, w.og8, m)
    g = posegrowref.grow_workload(w, w.og8, None, s)
    st, rl = oracle.dubins_plan(w.og8, w.n + m, w.star, w.xs, w.xg, np.concatenate([w.samples, s[:, :2]]), np.concatenate([w.heads, s[:, 2]]),
                                r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    live = rl.j + rl.found
    assert g.j0 == w.j and (g.j, g.found, g.vgoal, g.status) == (rl.j, rl.found, rl.vgoal, st) and g.j > w.j + 20
    assert np.array_equal(g.pts[:live], rl.pts[:live]) and np.array_equal(g.head[:live], rl.head[:live])
    assert np.array_equal(g.parent[:live], rl.parent[:live])
    assert np.array_equal(g.vcost[:live].view(np.int64), rl.vcost[:live].view(np.int64))
    if rl.found:  # the goal row: row j and row n of either
        assert tuple(g.pts[g.n]) == tuple(rl.pts[w.n + m]) == w.xg[:2] and g.head[g.n] == rl.head[w.n + m] == w.xg[2]
        assert g.vcost[g.n] == rl.vcost[w.n + m] == rl.vcost[rl.j] and g.parent[g.j] == rl.parent[rl.j]
    assert np.array_equal(g.accept_log, rl.accept_log[w.n:]) and np.array_equal(g.nearest_log, rl.nearest_log[w.n:])
    assert 0 < g.accept_log.sum() < m
    # the statistics of the m iterations are the longer plan's less the first plan's
    ro = w.ro
    assert (g.sum_j, g.sum_cells_nn, g.sum_near) == (rl.sum_j - ro.sum_j, rl.sum_cells_nn - ro.sum_cells_nn, rl.sum_near - ro.sum_near)


def test_the_stream_of_the_audited_grow_is_one_the_audit_policy_takes():
    """The GPU test sends the tree of uncut A grown by 600 samples through oracle/dubins_ref.c's audit under posecalls.assert_audit_clean's policy.
    How many decisions fall into the audit's ambiguous classes is a property of the stream: the oracle's OWN tree of this one has to
    pass the policy, or no device could."""
    w = poseref.workload("A")
    s = posegrowref.more_poses(w, w.og8, 600, seed=posegrowref.UNCUT_A_SEED)
    samples, heads = np.concatenate([w.samples, s[:, :2]]), np.concatenate([w.heads, s[:, 2]])
    st, rl = oracle.dubins_plan(w.og8, w.n + 600, w.star, w.xs, w.xg, samples, heads, r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    a = oracle.dubins_audit(w.og8, w.n + 600, w.star, samples, heads, rl.pts, rl.head, rl.vcost, rl.parent, rl.j, r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    assert a["n_accepted"] == rl.j - 1 and rl.j > w.j + 100 and w.j % 128 != 0
    assert_audit_clean(a, w.star)


# ------------------------------------------------------------------------------------------------ what the cut workloads show
@pytest.mark.parametrize("name", WORKLOADS)
def test_the_six_blocks_cut_enough_and_nearly_every_alive_vertex_moves(name):
    k = posekeepref.changed(name)
    w = k.w
    cut, j = int((~k.alive).sum()), w.j
    assert 8 * cut >= j and k.alive[0] and k.alive.sum() >= 8, (name, cut, j)  # an eighth of the tree at least, and a seed is left
    ids = np.flatnonzero(k.alive)
    moved = ids != np.arange(len(ids))
    assert 4 * moved.sum() >= 3 * len(ids), (name, int(moved.sum()), len(ids))
    if w.nh > 1:  # a seed that copies headings without gathering them cannot pass: the old vertex k had another heading
        other = w.ro.head[:j][ids][moved] != w.ro.head[:j][np.arange(len(ids))][moved]
        assert 2 * other.sum() >= moved.sum(), (name, int(other.sum()), int(moved.sum()))


@pytest.mark.parametrize("name", WORKLOADS)
def test_a_random_stream_is_accepted_in_part_and_misses_the_cut_cells(name):
    k = posekeepref.changed(name)
    w = k.w
    m = int((~k.alive).sum())
    s = posegrowref.more_poses(w, k.og8, m, seed=78)
    g = posegrowref.grow_workload(w, k.og8, k.alive, s)
    assert 0.20 <= g.accept_log.mean() <= 0.65, (name, g.accept_log.mean())
    cut_cells = {(int(x), int(y)) for x, y in w.ro.pts[:w.j][~k.alive]}
    hits = sum((int(x), int(y)) in cut_cells for x, y, _ in s)
    assert hits <= 3, (name, hits)  # ... so the tests plant such samples


@pytest.mark.parametrize("name", WORKLOADS)
def test_the_planted_stream_lands_on_cut_cells_and_on_the_start(name):
    k, s, rows, row_start, row_ob, g = posegrowref.planted(name)
    w = k.w
    assert len(s) == int((~k.alive).sum()) == len(g.accept_log) and g.j0 == int(k.alive.sum()) and g.j0 + len(s) <= w.n
    cut_cells = {(int(x), int(y)) for x, y in w.ro.pts[:w.j][~k.alive]}
    alive_cells = {(int(x), int(y)) for x, y in w.ro.pts[:w.j][k.alive]}
    assert len(rows) >= 4
    for r in rows.tolist():
        c = (int(s[r, 0]), int(s[r, 1]))
        assert c in cut_cells and c not in alive_cells and k.og8[c] == 0
    assert tuple(s[row_start, :2]) == w.xs[:2] and k.og8[int(s[row_ob, 0]), int(s[row_ob, 1])] != 0
    # the restatement accepts at least one of each: a cut vertex's cell is a vertex again, and the start's cell is drawn once
    assert g.accept_log[rows].sum() >= 1 and g.accept_log[row_start] == 1 and g.accept_log[row_ob] == 0
    assert 0.20 <= g.accept_log.mean() <= 0.65, (name, g.accept_log.mean())
    v = g.j0 + int(g.accept_log[:row_start].sum())  # the vertex on the start's cell: its nearest vertex is the root
    assert tuple(g.pts[v]) == w.xs[:2] and g.head[v] == s[row_start, 2] and g.nearest_log[row_start] == 0


def test_the_seed_keeps_order_costs_and_headings_and_renumbers_parents():
    k = posekeepref.changed("A")
    ro, j = k.w.ro, k.w.j
    ids, sp, sh, sc, spar = posegrowref.seed(ro.pts, ro.head, ro.parent, ro.vcost, j, k.alive)
    assert np.array_equal(ids, np.flatnonzero(k.alive)) and np.all(np.diff(ids) > 0) and ids[0] == 0 and spar[0] == -1
    assert np.array_equal(sp, ro.pts[:j][ids]) and np.array_equal(sh, ro.head[:j][ids]) and np.array_equal(sc, ro.vcost[:j][ids])
    assert np.array_equal(ids[spar[1:]], ro.parent[:j][ids][1:])
    whole = posegrowref.seed(ro.pts, ro.head, ro.parent, ro.vcost, j)
    assert np.array_equal(whole[0], np.arange(j)) and np.array_equal(whole[4][1:], ro.parent[1:j]) and whole[4][0] == -1
    assert tuple(k.w.xs[:2]) not in posegrowref.sampled_of(sp)


def test_go2goal_fallbacks_follow_the_querys_own_n():
    w = poseref.workload("F")  # rho too wide for the map: the tree is the start alone and nothing connects
    assert w.j == 1 and not w.ro.found
    s = posegrowref.more_poses(w, w.og8, 3)
    g = posegrowref.grow_workload(w, w.og8, None, s)
    assert g.j == 1 and not g.found and g.status == posegrowref.ST_UNREACHABLE and g.vgoal == 0 and g.rows == w.n


# ------------------------------------------------------------------------------------------------ binding and arguments, no device
def test_the_binding_declares_the_grow_poses_calls():
    for s in ("rrt_batch_grow_poses", "rrt_plan_grow_poses"):
        assert s in _ffi.SYMBOLS
    L = _ffi.lib()
    assert L.rrt_batch_grow_poses.argtypes[1] is ctypes.c_int32 and len(L.rrt_batch_grow_poses.argtypes) == 7 and len(L.rrt_plan_grow_poses.argtypes) == 6
    j0 = ctypes.c_int32(0)  # NULL handles are refused before anything touches a device
    assert L.rrt_batch_grow_poses(None, 0, None, 0, ctypes.byref(j0), None, ctypes.byref(j0)) == _ffi.RRT_E_ARG
    assert L.rrt_plan_grow_poses(None, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    assert hasattr(_ffi.Batch, "grow_poses") and hasattr(_ffi.Context, "grow_poses")


def test_pose_samples_are_rows_of_three():
    s = _ffi._grow_pose_samples(np.array([[3, 7, 1], [200, 150, 63]], dtype=np.int64))
    assert s.dtype == np.int32 and s.tolist() == [[3, 7, 1], [200, 150, 63]] and s.flags["C_CONTIGUOUS"]
    assert _ffi._grow_pose_samples(np.zeros((0, 3), dtype=np.int64)).shape == (0, 3)
    with pytest.raises(ValueError, match=r"\(m, 3\)"):
        _ffi._grow_pose_samples(np.zeros((4, 2), dtype=np.int64))


def test_the_planners_refuse_before_any_plan():
    og = np.zeros((32, 32), dtype=np.int64)
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 8, pbar=False), amd.RRTStarInformed(og, 50, 8, 4, pbar=False)):
        with pytest.raises(ValueError, match="grow_poses: .*use grow "):  # the straight-line planners are sent to grow
            p.grow_poses(5)
        assert p._ctx is None  # nothing was created on the way
    for p in (RRTDubins(og, 50, 4.0, pbar=False), RRTStarDubins(og, 50, 8, 4.0, pbar=False)):
        with pytest.raises(RuntimeError, match="grow_poses: no tree on the device"):
            p.grow_poses(5)
        with pytest.raises(ValueError, match="grow: RRTStandard and RRTStar only"):  # grow keeps its text
            p.grow(5)
        assert p._ctx is None
    p = RRTStarDubins(og, 50, 8, 4.0, pbar=False, costfn=lambda vcosts, points, v, x: vcosts[v] + 1.0)
    with pytest.raises(ValueError, match="grow_poses: .*costfn"):
        p.grow_poses(5)
