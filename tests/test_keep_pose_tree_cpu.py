"""CPU: the host side of keep_pose_tree -- the restatement the GPU tests compare with (posekeepref.py) held to what it is for, the
conditions under which the changed maps, the chain and the stride trees of test_keep_pose_tree_gpu.py are worth running, and the
planners' guards.  Everything is asserted without a GPU."""
import numpy as np
import pytest

import poseref
import posekeepref
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

WORKLOADS = ["A", "B", "D", "E"]
INF = np.inf


def _all_alive_on_its_own_map(w):
    k = posekeepref.kept(w, w.og8)
    assert k.ok.all() and k.alive.all() and len(k.alive) == w.j, (w.name, np.flatnonzero(~k.ok)[:8])
    assert np.array_equal(k.vertex, w.vertex) and np.array_equal(k.cost, w.cost)  # the view of everything answers as the tree


# ------------------------------------------------------------------------------------------------ an unchanged map
@pytest.mark.parametrize("name", WORKLOADS)
def test_an_unchanged_map_keeps_every_vertex_of_a_workload(name):
    """the edge definition is plan()'s own: the oracle accepted every edge by this sweep of this word"""
    _all_alive_on_its_own_map(poseref.workload(name))


@pytest.mark.parametrize("place", list(poseref.TIE_PLACES))
def test_an_unchanged_map_keeps_every_vertex_of_the_duplicate_trees(place):
    for rho, nh in poseref.TIE_PAIRS:
        for star in (0, 1):
            w = poseref.tie_duplicate(rho, nh, star, place)
            _all_alive_on_its_own_map(w)
            assert w.ro.vcost[w.dup] == 0.0  # the zero-length edge among them


@pytest.mark.parametrize("j", posekeepref.STRIDE_KEEP_J)
def test_an_unchanged_map_keeps_every_vertex_of_the_stride_trees(j):
    for star in (0, 1):
        _all_alive_on_its_own_map(poseref.stride_tree(j, star))


# ------------------------------------------------------------------------------------------------ the changed map
def test_the_blocks_are_the_stated_draw():
    w = poseref.workload("E")
    W, H = w.og8.shape
    og2 = posekeepref.blocks_map(w.og8, w.xs)
    rng = np.random.default_rng(7)
    want, placed = w.og8.copy(), 0
    while placed < 6:
        x = int(rng.integers(0, W - 8))
        y = int(rng.integers(0, H - 8))
        if abs(x + 4 - w.xs[0]) <= 16 and abs(y + 4 - w.xs[1]) <= 16:
            continue
        want[x:x + 8, y:y + 8] = 1
        placed += 1
    assert np.array_equal(og2, want) and og2[w.xs[0], w.xs[1]] == 0 and (og2 >= w.og8).all() and (og2 != w.og8).any()


@pytest.mark.parametrize("name", WORKLOADS)
def test_the_changed_map_cuts_some_and_not_all_and_the_view_matters(name):
    k = posekeepref.changed(name)
    w = k.w
    n_alive = int(k.alive.sum())
    free_but_dead = int((k.ok & ~k.alive).sum())
    v_whole, c_whole = posekeepref.whole_tree_on(k)
    differing = int(((v_whole != k.vertex) | (c_whole != k.cost)).sum())
    print(name, "alive", n_alive, "of", w.j, "own edge free but dead", free_but_dead, "goals differing", differing, "connected", int((k.vertex >= 0).sum()))
    assert 0.05 * w.j <= n_alive <= 0.95 * w.j
    assert free_but_dead >= 1  # a vertex that dies through an ancestor: the pointer jumping decides it, not its own edge
    assert differing >= 1      # answering from the whole tree on the new map would show
    assert k.alive[0] and not k.alive[~k.ok].any()
    assert k.alive[k.vertex[k.vertex >= 0]].all()
    # every ancestor of an alive vertex is alive: the parent walks of paths_to_poses stay inside the view
    par = np.asarray(w.ro.parent[:w.j])
    assert k.alive[par[np.flatnonzero(k.alive)[1:]]].all()
    assert (n_alive, free_but_dead, differing) == {"E": (123, 9, 4), "D": (148, 8, 1), "A": (328, 33, 1), "B": (706, 54, 2)}[name]


# ------------------------------------------------------------------------------------------------ the chain
def test_the_cut_chain_needs_every_jump_round():
    k = posekeepref.chain_cut()
    w = k.w
    j = w.j
    assert j == 1100 and np.all(w.ro.parent[1:j] == np.arange(j - 1))
    cut = np.flatnonzero(~k.ok)
    assert 1 <= len(cut) <= 3 and cut.max() - cut.min() == len(cut) - 1, cut  # the edges over the cell, next to each other
    first = int(cut.min())
    assert k.alive[:first].all() and not k.alive[first:].any() and 380 <= j - first <= 420, (first, j)
    # ceil(log2 j) = 11 rounds of pointer jumping; one fewer covers 1024 vertices towards the root and keeps vertices that are not alive
    rounds = 1
    while (1 << rounds) < j:
        rounds += 1
    assert rounds == 11

    def jumped(ok, r):
        """rrt_keep_jump_kernel r times, then rrt_keep_compact_kernel's alive (rrt_keep.h), restated"""
        ok, anc = ok.copy(), np.concatenate([[0], np.asarray(w.ro.parent[1:j], dtype=np.int64)])
        for _ in range(r):
            ok, anc = ok & ok[anc], anc[anc]
        return ok & (anc == 0)

    whole = posekeepref.kept(w, w.og8)
    assert whole.alive.all()
    assert np.array_equal(jumped(k.ok, 11), k.alive) and np.array_equal(jumped(whole.ok, 11), whole.alive)
    # a round fewer reaches 1024 vertices towards the root: a vertex deeper than that is then wrong in one of the two states -- on the
    # whole chain it has not arrived at the root, and a walk that is not at the root counts as cut.  The workloads are at most 10 deep.
    assert not jumped(whole.ok, 10)[1025:].any() and jumped(whole.ok, 10)[:1025].all()
    # the goals behind the cut connect from in front of it or not at all
    assert k.alive[k.vertex[k.vertex >= 0]].all()


# ------------------------------------------------------------------------------------------------ the stride trees, cut
@pytest.mark.parametrize("j", posekeepref.STRIDE_KEEP_J)
def test_the_stamped_block_lies_in_the_trees_half(j):
    cut_any = False
    for star in (0, 1):
        k = posekeepref.stride_cut(j, star)
        assert k.alive[0] and len(k.alive) == j
        cut_any |= not k.alive.all()
        if j >= 63:
            assert 0 < (~k.alive).sum() < j, (j, star, int(k.alive.sum()))
    assert cut_any or j < 63


# ------------------------------------------------------------------------------------------------ the root blocked
@pytest.mark.parametrize("name", ["E", "D"])
def test_a_blocked_root_leaves_nothing(name):
    k = posekeepref.root_blocked(poseref.workload(name))
    assert not k.alive.any() and np.all(k.vertex == -1) and np.all(k.cost == INF)


# ------------------------------------------------------------------------------------------------ the planners' guards
class _HostDevice:
    """stands in for the device context: answers keep_pose_tree and connect_poses from the restatement"""

    def __init__(self, w, planner):
        self.w, self.p, self.alive = w, planner, None

    def keep_pose_tree(self):
        w = self.w
        self.alive = posekeepref.alive(np.ascontiguousarray(np.asarray(self.p.og) != 0, dtype=np.uint8), w.ro.pts, w.ro.head, w.ro.parent, w.j, w.rho, w.nh)
        return self.alive


def _dubins(cls, og, n=100):
    args = (og, n) + ((10,) if cls is RRTStarDubins else ()) + (3.0,)
    return cls(*args, n_headings=16, pbar=False)


@pytest.mark.parametrize("cls", [RRTDubins, RRTStarDubins])
def test_the_planner_guards(cls):
    og = np.zeros((40, 30), dtype=int)
    p = _dubins(cls, og)
    with pytest.raises(RuntimeError, match="plan"):
        p.keep_pose_tree(og)
    p._tree_resident = "device"  # as after a plan()
    with pytest.raises(ValueError, match="planned on"):
        p.keep_pose_tree(np.zeros((40, 31), dtype=int))
    assert p._tree_resident == "device"  # (the refusal changed nothing)
    p.set_og(og.copy())
    with pytest.raises(RuntimeError, match="plan"):  # set_og still drops the tree
        p.keep_pose_tree(og)
    # the straight-line calls stay refused for a Dubins planner, as before
    for call in (lambda: p.keep_tree(og), lambda: p.keep_tree_resident(None), lambda: p.connect_goals([(5, 5)]), lambda: p.routes_to([(5, 5)])):
        with pytest.raises(ValueError, match="Dubins"):
            call()
    with pytest.raises(ValueError, match="RRTStandard and RRTStar only"):
        p.grow(10)


def test_the_planner_takes_the_new_map_as_keep_tree_does():
    w = poseref.workload("E")
    k = posekeepref.changed("E")
    p = RRTStarDubins(w.og, w.n, 12, w.rho, n_headings=w.nh, pbar=False)
    dev = _HostDevice(w, p)
    p._device = lambda: dev
    p._tree_resident = "device"
    p._grid_dirty = False
    og2 = k.og8.astype(np.int64)
    alive = p.keep_pose_tree(og2)
    assert np.array_equal(alive, k.alive) and alive.dtype == bool
    assert p.og is og2 and np.array_equal(p.free, np.argwhere(og2 == 0)) and p._grid_dirty and p._tree_resident == "device"

    def failing():
        raise RuntimeError("device")

    dev.keep_pose_tree = failing
    with pytest.raises(RuntimeError, match="device"):
        p.keep_pose_tree(w.og)
    assert p._tree_resident is None  # a failure leaves no tree for this grid


def test_the_straight_line_planners_name_keep_tree():
    og = np.zeros((40, 30), dtype=int)
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 10, pbar=False), amd.RRTStarInformed(og, 50, 10, 5, pbar=False)):
        with pytest.raises(ValueError, match="use keep_tree"):
            p.keep_pose_tree(og)
        with pytest.raises(ValueError, match="use keep_tree"):
            p.keep_pose_tree_resident(None, 0)
