"""CPU: the host restatement of reroot (tests/rerootref.py) pinned against the oracle, its rules on hand-written trees, the inputs
the GPU tests rely on, and the binding and argument checks of RRT.reroot / _ffi that need no device.

Re-rooting the tree of oracle.plan at vertex 0 reverses nothing: it must give the same tree, renumbered by depth, with the same costs
bit for bit -- the oracle's costs are cost[parent] + sqrt(float64(d2)), the sum the restatement accumulates.

The blocked-edge inputs.  An edge that is free parent -> child and blocked child -> parent is an accident of the line walk; the maps
of tests/golden/plans_A.npz hold five (one on the maze, four on the noise map).  Re-rooting behind such an edge leaves the subtree
behind it and cuts the rest.  On the maze that is 75 of 77 vertices; on the noise map the largest such subtree has 8 of 1363
vertices, so no root of that input cuts less than 99.4 %: the 1 % .. 99 % condition is asserted on the maze input and on the
hand-written tree, and the noise input serves the conditions `d >= 8` and `more than one vertex cut` and the properties below."""
import ctypes

import numpy as np
import pytest

import growref
import keepref
import oracle
import rerootref
from plannedcases import GROW_CASES, MAZE, NOISE, grow_setup, hand_tree, one_way_edges, oracle_planned, roots_behind
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

CLEAN = [("noise200", 0, 300, 11), ("noise200", 1, 300, 12), ("square100", 0, 200, 14), ("square100", 1, 200, 15)]


def walked_cost(pts, new_parent, r, k):
    """the left-to-right f64 sum of the legs r -> ... -> k, from the path itself"""
    way = [k]
    while way[-1] != r:
        way.append(int(new_parent[way[-1]]))
    way.reverse()
    total = np.float64(0.0)
    for a, b in zip(way, way[1:]):
        dx, dy = int(pts[a][0]) - int(pts[b][0]), int(pts[a][1]) - int(pts[b][1])
        total = total + np.sqrt(np.float64(dx * dx + dy * dy))
    return total


def check_properties(c, R, r):
    """the independent form of the costs and the edge set, for any re-root of c's tree"""
    ro = c["ro"]
    for k in range(len(R.ids)):
        want = walked_cost(ro.pts, R.new_parent, r, int(R.ids[k]))
        assert R.vcost[k].view(np.int64) == want.view(np.int64), (r, k)
    alive = set(R.ids.tolist())
    before = {frozenset((k, int(ro.parent[k]))) for k in range(1, ro.j) if k in alive and int(ro.parent[k]) in alive}
    after = {frozenset((int(R.ids[k]), int(R.ids[R.parent[k]]))) for k in range(1, len(R.ids))}
    assert before == after and len(after) == len(R.ids) - 1
    assert np.all(np.diff(R.depth) >= 0) and R.depth[0] == 0 and np.all(R.depth[1:] == R.depth[R.parent[1:]] + 1)
    same = np.flatnonzero(np.diff(R.depth) == 0)
    assert np.all(R.ids[same] < R.ids[same + 1])  # inside a level the previous numbers ascend


# ------------------------------------------------------------------------------------------------ pinned on the oracle
@pytest.mark.parametrize("grid,alg,n,m,seed", GROW_CASES)
def test_reroot_at_zero_is_the_same_tree_renumbered(grid, alg, n, m, seed):
    og8, xs, xg, samples, r2 = grow_setup(grid, alg, n, m, seed)
    st, ro = oracle.plan(og8, n, alg, xs, xg, samples[:n], r2_rewire=r2)
    R = rerootref.reroot(og8, ro.pts, ro.parent, ro.j, 0)
    assert R.d == 0 and not R.reversed_ok and sorted(R.ids.tolist()) == list(range(ro.j)) and R.ids[0] == 0
    assert np.array_equal(R.pts, np.asarray(ro.pts[:ro.j])[R.ids])
    assert np.array_equal(R.ids[R.parent[1:]], np.asarray(ro.parent[:ro.j])[R.ids[1:]]) and R.parent[0] == -1
    assert np.array_equal(R.vcost.view(np.int64), np.asarray(ro.vcost[:ro.j])[R.ids].view(np.int64))  # bit for bit
    assert np.array_equal(R.depth, keepref.depth(ro.parent, ro.j)[R.ids])
    assert not np.array_equal(R.ids, np.arange(ro.j))  # no special case for vertex 0: the tree is renumbered by depth


# ------------------------------------------------------------------------------------------------ hand-written trees
def test_hand_tree_rerooted_at_a_leaf():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    R = rerootref.reroot(og, pts, parent, 6, 4)
    assert R.d == 3 and R.path == [4, 3, 1, 0] and R.ids.tolist() == [4, 3, 1, 0, 2, 5] and R.parent.tolist() == [-1, 0, 1, 2, 3, 4]
    assert R.vcost.tolist() == [0.0, 6.0, 12.0, 20.0, 28.0, 36.0] and np.array_equal(R.pts, pts[[4, 3, 1, 0, 2, 5]])
    # without vertex 5 nothing else sits on the old root's cell: it is in `sampled` as the cell of an ordinary vertex; the new root's is not
    R5 = rerootref.reroot(og, pts, parent, 5, 4)
    assert (2, 2) in growref.sampled_of(R5.pts) and (8, 16) not in growref.sampled_of(R5.pts)
    g = growref.grow(og, 0, 8, (19, 19), 0, R5.pts, R5.vcost, R5.parent, [(2, 2), (8, 16), (8, 16)])
    assert g.accept_log.tolist() == [0, 1, 0] and g.parent[5] == 0 and g.vcost[5] == 0.0  # the new start drawn once is a vertex


def test_hand_tree_rerooted_at_an_inner_vertex():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    R = rerootref.reroot(og, pts, parent, 6, 1)
    assert R.d == 1 and R.ids.tolist() == [1, 0, 3, 2, 4, 5] and R.parent.tolist() == [-1, 0, 0, 1, 2, 3]
    assert R.vcost.tolist() == [0.0, 8.0, 6.0, 16.0, 12.0, 24.0]
    assert growref.sampled_of(R.pts) == {(2, 2), (2, 16), (10, 2), (8, 16)}  # (2, 10), the new root's cell, is out


def test_a_blocked_cell_on_a_reversed_edge_cuts_exactly_the_far_side():
    pts, parent, vcost = hand_tree()
    og = np.zeros((20, 20), dtype=np.uint8)
    og[2, 13] = 1  # on the edge 1 - 3
    R = rerootref.reroot(og, pts, parent, 6, 4)
    assert R.reversed_ok == {3: True, 1: False, 0: True} and R.ids.tolist() == [4, 3] and R.parent.tolist() == [-1, 0] and R.vcost.tolist() == [0.0, 6.0]
    assert 0.01 <= 1 - len(R.ids) / 6 <= 0.99
    R = rerootref.reroot(og, pts, parent, 6, 2)  # the blocked cell lies on no reversed edge of this root: nothing is tested, nothing cut
    assert R.reversed_ok == {0: True} and len(R.ids) == 6
    # with a view the input is what keep_tree left: on this map 3 and 4 are gone before the re-root
    Rv = rerootref.reroot(og, pts, parent, 6, 5, og8_view=og)
    assert Rv.ids.tolist() == [5, 2, 0, 1] and Rv.parent.tolist() == [-1, 0, 1, 2] and Rv.vcost.tolist() == [0.0, 8.0, 16.0, 24.0]
    with pytest.raises(AssertionError):
        rerootref.reroot(og, pts, parent, 6, 4, og8_view=og)  # not alive in the view


# ------------------------------------------------------------------------------------------------ the inputs and their conditions
def test_the_maze_input_has_one_one_way_edge():
    c = oracle_planned(*MAZE)
    ro = c["ro"]
    assert ro.j == 77 and keepref.depth(ro.parent, ro.j).max() == 9
    assert one_way_edges(c) == [21] and len(roots_behind(c, [21])) == 2
    for r in roots_behind(c, [21]):
        R = rerootref.reroot(c["og8"], ro.pts, ro.parent, ro.j, r)
        cut = ro.j - len(R.ids)
        assert not R.reversed_ok[int(ro.parent[21])] and cut > 1 and 0.01 <= cut / ro.j <= 0.99, (r, cut)
        assert set(R.ids.tolist()) == set(roots_behind(c, [21]))  # what is left is the subtree behind the edge
        check_properties(c, R, r)


def test_the_noise_input_has_four_one_way_edges():
    c = oracle_planned(*NOISE)
    ro = c["ro"]
    assert ro.j == 1363 and keepref.depth(ro.parent, ro.j).max() == 16
    edges = one_way_edges(c)
    assert edges == [618, 1024, 1051, 1123] and len(roots_behind(c, edges)) == 14
    deep = [r for r in roots_behind(c, edges) if len(rerootref.path_to_root(ro.parent, ro.j, r)) - 1 >= 8]
    assert deep  # d >= 8
    for r in (deep[0], roots_behind(c, [618])[-1]):
        R = rerootref.reroot(c["og8"], ro.pts, ro.parent, ro.j, r)
        assert not all(R.reversed_ok.values()) and ro.j - len(R.ids) > 1 and len(R.ids) >= 1
        check_properties(c, R, r)


@pytest.mark.parametrize("grid,alg,n,seed", CLEAN)
def test_the_clean_inputs_have_none_and_round_trip(grid, alg, n, seed):
    c = oracle_planned(grid, alg, n, seed)
    ro, og8 = c["ro"], c["og8"]
    assert one_way_edges(c) == []
    dep = keepref.depth(ro.parent, ro.j)
    leaf = int(np.argmax(dep))
    mid = rerootref.path_to_root(ro.parent, ro.j, leaf)[int(dep[leaf]) // 2]
    for r in (leaf, mid):
        R = rerootref.reroot(og8, ro.pts, ro.parent, ro.j, r)
        assert all(R.reversed_ok.values()) and len(R.ids) == ro.j and R.d == dep[r]
        check_properties(c, R, r)
        # round trip: at the vertex the old root became
        back = int(np.flatnonzero(R.ids == 0)[0])
        R2 = rerootref.reroot(og8, R.pts, R.parent, len(R.ids), back)
        assert all(R2.reversed_ok.values())
        orig = R.ids[R2.ids]  # the original number of every vertex of the second tree
        assert orig[0] == 0 and sorted(orig.tolist()) == list(range(ro.j))
        assert np.array_equal(orig[R2.parent[1:]], np.asarray(ro.parent[:ro.j])[orig[1:]])
        assert np.array_equal(R2.vcost.view(np.int64), np.asarray(ro.vcost[:ro.j])[orig].view(np.int64))


def test_reroot_then_grow_feeds_the_loop_like_a_seed():
    c = oracle_planned("noise200", 1, 300, 12)
    ro = c["ro"]
    r = int(np.argmax(keepref.depth(ro.parent, ro.j)))
    R = rerootref.reroot(c["og8"], ro.pts, ro.parent, ro.j, r)
    m = c["n"] - ro.j
    more = hostprep.draw_free_samples(np.random.default_rng(5), np.argwhere(c["og8"] == 0), m)
    g = growref.grow(c["og8"], 1, c["n"], c["xg"], c["r2"], R.pts, R.vcost, R.parent, more)
    assert g.j0 == ro.j and g.j > g.j0 and np.array_equal(g.pts[0], ro.pts[r]) and g.vcost[0] == 0.0


# ------------------------------------------------------------------------------------------------ binding and arguments, no device
def test_the_binding_declares_the_reroot_calls():
    for s in ("rrt_batch_reroot", "rrt_batch_reroot_ms", "rrt_plan_reroot", "rrt_plan_reroot_ms"):
        assert s in _ffi.SYMBOLS
    L = _ffi.lib()
    assert L.rrt_batch_reroot.argtypes[2] is ctypes.c_int32 and len(L.rrt_batch_reroot.argtypes) == 8 and len(L.rrt_plan_reroot.argtypes) == 7
    j0 = ctypes.c_int32(0)
    assert L.rrt_batch_reroot(None, 0, 0, None, 0, ctypes.byref(j0), None, ctypes.byref(j0)) == _ffi.RRT_E_ARG
    assert L.rrt_batch_reroot_ms(None, None, 8) == _ffi.RRT_E_ARG
    assert L.rrt_plan_reroot(None, 0, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_reroot_ms(None, None, 8) == _ffi.RRT_E_ARG


def test_the_classes_that_do_not_reroot_say_so_before_any_device_call():
    og = np.zeros((32, 32), dtype=np.int64)
    for p, why in ((amd.RRTStarInformed(og, 50, 8, 4, pbar=False), "RRTStandard and RRTStar only"),
                   (RRTStarDubins(og, 50, 8, 4.0, pbar=False), "a Dubins word is not reversible"),
                   (RRTDubins(og, 50, 4.0, pbar=False), "a Dubins word is not reversible"),
                   (amd.RRTStar(og, 50, 8, pbar=False, rewire="correct"), "child lists"),
                   (amd.RRTStar(og, 50, 8, pbar=False, costfn=lambda vcosts, points, v, x: vcosts[v] + 1.0), "custom cost function"),
                   (amd.RRTStandard(np.zeros((2100, 8), dtype=np.int64), 50, pbar=False), "large-grid")):
        with pytest.raises(ValueError, match="reroot: .*" + why):
            p.reroot(3)
        assert p._ctx is None  # nothing was created on the way
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 8, pbar=False)):
        with pytest.raises(RuntimeError, match="reroot: no tree on the device"):
            p.reroot(3)
        assert p._ctx is None


def test_m_and_room_are_checked_before_any_device_call():
    p = amd.RRTStar(np.zeros((32, 32), dtype=np.int64), 50, 8, pbar=False)
    p._tree_resident, p._grow_j0 = "device", 40  # as a plan() that left 40 vertices
    state = p.rand_gen.bit_generator.state
    with pytest.raises(ValueError, match="reroot: m=-1"):
        p.reroot(3, -1)
    with pytest.raises(ValueError, match="reroot: the tree holds 40 vertices and n=50: room for 10 more samples, not 11"):
        p.reroot(3, 11)
    with pytest.raises(ValueError, match="reroot: vertex=-2"):
        p.reroot(-2)
    p._grow_j0 = 0
    with pytest.raises(ValueError, match="reroot: no vertex of the tree is alive"):
        p.reroot(0)
    assert p._ctx is None and p.rand_gen.bit_generator.state == state and p._tree_resident == "device"
