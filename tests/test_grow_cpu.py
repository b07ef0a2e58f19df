"""CPU: the host restatement of grow (tests/growref.py) pinned against the oracle, its seed rules on hand-written trees, and the
binding and argument checks of RRT.grow / _ffi that need no device.

With nothing cut, growing the tree of oracle.plan(n) by m samples IS oracle.plan(n + m) on the concatenated samples as long as the
capacity rule `j != n` never bound in the n plan -- the maps are those of tests/golden/plans_A.npz, where the oracle itself is pinned
to the reference."""
import ctypes

import numpy as np
import pytest

import growref
import oracle
from plannedcases import GROW_CASES, grow_setup, hand_tree
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTStarDubins


def _same_tree(g, ro, rows):
    assert g.j == ro.j and g.found == ro.found and g.vgoal == ro.vgoal
    assert np.array_equal(g.pts[:rows], ro.pts[:rows]) and np.array_equal(g.parent[:rows], ro.parent[:rows])
    assert np.array_equal(g.vcost[:rows].view(np.int64), ro.vcost[:rows].view(np.int64))  # bit for bit


@pytest.mark.parametrize("grid,alg,n,m,seed", GROW_CASES)
def test_nothing_cut_one_grow_is_the_longer_plan(grid, alg, n, m, seed):
    og8, xs, xg, samples, r2 = grow_setup(grid, alg, n, m, seed)
    st0, r0 = oracle.plan(og8, n, alg, xs, xg, samples[:n], r2_rewire=r2)
    assert r0.j < n and (r0.accept_log == 0).any()  # the n plan rejected samples: `j != n` never bound in it
    st1, r1 = oracle.plan(og8, n + m, alg, xs, xg, samples, r2_rewire=r2)
    ids, sp, sc, spar = growref.seed(r0.pts, r0.parent, r0.vcost, r0.j)
    assert np.array_equal(ids, np.arange(r0.j))
    g = growref.grow(og8, alg, n + m, xg, r2, sp, sc, spar, samples[n:])
    assert g.status == st1
    _same_tree(g, r1, r1.j + r1.found)
    assert np.array_equal(g.nearest_log, r1.nearest_log[n:]) and np.array_equal(g.accept_log, r1.accept_log[n:]) and np.array_equal(g.jlog, r1.jlog[n:])
    assert g.rows == r1.rows and g.j > r0.j


@pytest.mark.parametrize("grid,alg,n,m,seed", GROW_CASES[:3])
def test_nothing_cut_two_grows_are_one_plan(grid, alg, n, m, seed):
    og8, xs, xg, samples, r2 = grow_setup(grid, alg, n, m, seed)
    N, m1 = n + m, m // 3
    st0, r0 = oracle.plan(og8, n, alg, xs, xg, samples[:n], r2_rewire=r2)
    st1, r1 = oracle.plan(og8, N, alg, xs, xg, samples, r2_rewire=r2)
    _, sp, sc, spar = growref.seed(r0.pts, r0.parent, r0.vcost, r0.j)
    g1 = growref.grow(og8, alg, N, xg, r2, sp, sc, spar, samples[n:n + m1])
    _, sp, sc, spar = growref.seed(g1.pts, g1.parent, g1.vcost, g1.j)  # (the goal row of the first grow is not a tree vertex)
    g2 = growref.grow(og8, alg, N, xg, r2, sp, sc, spar, samples[n + m1:])
    _same_tree(g2, r1, r1.j + r1.found)
    assert np.array_equal(np.concatenate([g1.accept_log, g2.accept_log]), r1.accept_log[n:])


# ------------------------------------------------------------------------------------------------ seed rules, hand-written trees
def test_a_cut_vertex_leaves_sampled_and_its_cell_is_accepted_again():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    og[2, 13] = 1  # cuts the edge 1 -> 3, and 4 with it
    ids, sp, sc, spar = growref.seed(pts, parent, vcost, 6, og8_view=og)
    assert ids.tolist() == [0, 1, 2, 5] and spar.tolist() == [-1, 0, 0, 2] and sc.tolist() == [0.0, 8.0, 8.0, 16.0]
    assert growref.sampled_of(sp) == {(2, 10), (10, 2), (2, 2)}  # (8, 16) and (2, 16) are gone
    g = growref.grow(og, 1, 10, (19, 19), hostprep.radius_threshold(30), sp, sc, spar, [(8, 16), (2, 10), (8, 16)])
    assert g.accept_log.tolist() == [1, 0, 0] and g.j == 5 and np.array_equal(g.pts[4], (8, 16))
    assert g.jlog.tolist() == [4, 5, 5]


def test_the_roots_cell_is_sampled_only_through_another_vertex():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    _, sp, sc, spar = growref.seed(pts, parent, vcost, 6)
    assert (2, 2) in growref.sampled_of(sp)  # through vertex 5
    _, sp5, sc5, spar5 = growref.seed(pts, parent, vcost, 5)  # the tree without vertex 5
    assert (2, 2) not in growref.sampled_of(sp5)
    g = growref.grow(og, 0, 8, (19, 19), 0, sp5, sc5, spar5, [(2, 2), (2, 2)])
    assert g.accept_log.tolist() == [1, 0] and g.parent[5] == 0 and g.vcost[5] == 0.0  # xstart drawn once is a vertex (rrt.py:425)
    og2 = og.copy()
    og2[6, 2] = 1  # cuts 0 -> 2 and 5 with it: the root's cell leaves the set again
    _, sp2, _, _ = growref.seed(pts, parent, vcost, 6, og8_view=og2)
    assert (2, 2) not in growref.sampled_of(sp2)


def test_a_blocked_root_has_no_seed():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    og[2, 2] = 1
    ids, sp, sc, spar = growref.seed(pts, parent, vcost, 6, og8_view=og)
    assert len(ids) == 0
    with pytest.raises(AssertionError):
        growref.grow(og, 0, 8, (19, 19), 0, sp, sc, spar, [(3, 3)])


def test_go2goal_fallbacks_follow_the_querys_own_n():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    og[17:20, 17:20] = 1  # the goal sits on an obstacle: no vertex sees it
    _, sp, sc, spar = growref.seed(pts, parent, vcost, 6)
    g = growref.grow(og, 0, 8, (18, 18), 0, sp, sc, spar, [(5, 5)])
    assert g.j == 7 and not g.found and g.status == growref.ST_UNREACHABLE and g.rows == 8  # j < n: rrt.py:318 faults
    g = growref.grow(og, 0, 7, (18, 18), 0, sp, sc, spar, [(5, 5)])
    assert g.j == 7 and not g.found and g.status == growref.ST_OK and g.vgoal == 0  # j == n: rrt.py:330-331


# ------------------------------------------------------------------------------------------------ binding and arguments, no device
def test_the_binding_declares_the_grow_calls():
    for s in ("rrt_batch_grow", "rrt_batch_grow_ms", "rrt_plan_grow", "rrt_plan_grow_ms"):
        assert s in _ffi.SYMBOLS
    L = _ffi.lib()
    assert L.rrt_batch_grow.argtypes[1] is ctypes.c_int32 and len(L.rrt_batch_grow.argtypes) == 7 and len(L.rrt_plan_grow.argtypes) == 6
    # NULL handles are refused before anything touches a device
    j0 = ctypes.c_int32(0)
    assert L.rrt_batch_grow(None, 0, None, 0, ctypes.byref(j0), None, ctypes.byref(j0)) == _ffi.RRT_E_ARG
    assert L.rrt_batch_grow_ms(None, None, 3) == _ffi.RRT_E_ARG
    assert L.rrt_plan_grow(None, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_grow_ms(None, None, 3) == _ffi.RRT_E_ARG


def test_grow_samples_are_unpacked():
    s = _ffi._grow_samples(np.array([3 | (7 << 16), 200 | (150 << 16)], dtype=np.uint32))
    assert s.dtype == np.int32 and s.tolist() == [[3, 7], [200, 150]] and s.flags["C_CONTIGUOUS"]
    assert _ffi._grow_samples(np.zeros((0, 2), dtype=np.int64)).shape == (0, 2)


def test_the_classes_that_do_not_grow_say_so_before_any_device_call():
    og = np.zeros((32, 32), dtype=np.int64)
    for p in (amd.RRTStarInformed(og, 50, 8, 4, pbar=False), RRTStarDubins(og, 50, 8, 4.0, pbar=False), amd.RRTStar(og, 50, 8, pbar=False, rewire="correct"),
              amd.RRTStar(og, 50, 8, pbar=False, costfn=lambda vcosts, points, v, x: vcosts[v] + 1.0),
              amd.RRTStandard(np.zeros((2100, 8), dtype=np.int64), 50, pbar=False)):
        with pytest.raises(ValueError, match="grow"):
            p.grow(5)
        assert p._ctx is None  # nothing was created on the way
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 8, pbar=False)):
        with pytest.raises(RuntimeError, match="grow: no tree on the device"):
            p.grow(5)
        assert p._ctx is None
