"""CPU: the host restatement of keep_tree (keepref.py) on hand-built trees and on the reference's goldens, and what RRT.keep_tree /
RRT.keep_tree_resident do to the planner without the device.  The device side is tests/test_keep_tree_gpu.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import goalref
import keepref
import oracle
import orchelp
import routeref
from plannedcases import WALL64_XG, WALL64_XS, pinned_goal_cases, wall64_og, wall64_planned
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

INF = np.inf


def _chain(k):
    """a tree that is one chain along y = 10: vertex i at (5 + 4 i, 10), costs 4 i"""
    pts = np.array([(5 + 4 * i, 10) for i in range(k)], dtype=np.int64)
    return pts, np.arange(-1, k - 1), 4.0 * np.arange(k)


def test_a_chain_cut_in_the_middle():
    pts, parent, vcost = _chain(10)
    og8 = np.zeros((64, 32), dtype=np.uint8)
    assert keepref.alive(og8, pts, parent, 10).all()
    og8[5 + 4 * 5 + 2, 10] = 1  # on the edge 5 -> 6, on no vertex
    assert keepref.edge_ok(og8, pts, parent, 10).tolist() == [True] * 6 + [False] + [True] * 3
    assert keepref.alive(og8, pts, parent, 10).tolist() == [True] * 6 + [False] * 4
    goals = [(41, 20), (9, 20)]  # in the open: a straight chain gains nothing, the root is as cheap as anything, before and after
    a, v, c = keepref.connect(og8, pts, parent, vcost, 10, goals)
    v0, c0, _ = goalref.connect(og8, pts, vcost, 10, goals)
    assert v0.tolist() == [0, 0] and v.tolist() == [0, 0]
    a, got = keepref.routes(og8, pts, parent, vcost, 10, [(41, 10)])
    assert got[0].tolist() == [-1] and got[2].tolist() == [INF] and got[3].tolist() == [0, 0]  # the goal on the chain, behind the cut
    og8[:, 12] = 1  # a wall under the chain, open only at x >= 38: only the vertices 9 and 8 see the goal below it ...
    og8[38:, 12] = 0
    og8[27, 10] = 0
    v0, c0, _ = goalref.connect(og8, pts, vcost, 10, [(41, 20)])
    assert v0[0] in (8, 9)
    og8[27, 10] = 1  # ... and with the cut back none of them is alive
    a, v, c = keepref.connect(og8, pts, parent, vcost, 10, [(41, 20)])
    assert a.sum() == 6 and v.tolist() == [-1] and c.tolist() == [INF]


def test_a_blocked_root():
    pts, parent, vcost = _chain(6)
    og8 = np.zeros((64, 32), dtype=np.uint8)
    og8[5, 10] = 1
    assert keepref.edge_ok(og8, pts, parent, 6).tolist() == [False, False] + [True] * 4  # (the walk of edge 0 -> 1 starts on the root)
    a, got = keepref.routes(og8, pts, parent, vcost, 6, [(20, 20), (5, 10)], cut=True)
    assert not a.any()
    vertex, cost, length, offsets, xy, ids = got
    assert vertex.tolist() == [-1, -1] and np.all(cost == INF) and np.all(length == INF) and offsets.tolist() == [0, 0, 0] and len(xy) == len(ids) == 0
    a, v, c = keepref.connect(og8, pts, parent, vcost, 6, [(20, 20)])
    assert v.tolist() == [-1] and v.dtype == np.int32 and c.tolist() == [INF]


def test_a_parent_with_a_higher_index_than_its_child():
    # 0 -> 3 -> 1 -> 2 and 0 -> 4: the parent of vertex 1 is vertex 3
    pts = np.array([(5, 5), (25, 5), (35, 5), (15, 5), (5, 20)], dtype=np.int64)
    parent = np.array([-1, 3, 1, 0, 0])
    vcost = np.array([0.0, 20.0, 30.0, 10.0, 15.0])
    og8 = np.zeros((48, 32), dtype=np.uint8)
    assert keepref.depth(parent, 5).tolist() == [0, 2, 3, 1, 1]
    og8[10, 5] = 1  # the edge 0 -> 3: the cut vertex has the highest index of its branch
    a, ids, p, c, par = keepref.view(og8, pts, parent, vcost, 5)
    assert a.tolist() == [True, False, False, False, True] and ids.tolist() == [0, 4] and par.tolist() == [-1, 0]
    og8[10, 5] = 0
    og8[30, 5] = 1  # the edge 1 -> 2
    a, ids, p, c, par = keepref.view(og8, pts, parent, vcost, 5)
    assert a.tolist() == [True, True, False, True, True] and ids.tolist() == [0, 1, 3, 4] and par.tolist() == [-1, 2, 0, 0]
    assert c.tolist() == [0.0, 20.0, 10.0, 15.0]  # the costs go with their vertices, unchanged
    og8[6:23, 8] = 1  # a wall under the branch with a gap under vertex 1 = (25, 5): only that vertex sees the goal below the gap
    og8[28:, 8] = 1
    a, got = keepref.routes(og8, pts, parent, vcost, 5, [(25, 12)])
    assert a.tolist() == [True, True, False, True, True]
    vertex, cost, length, offsets, xy, ids = got
    assert vertex.tolist() == [1] and ids.tolist() == [0, 3, 1, -1]  # original numbers, through the higher-numbered parent
    assert xy.tolist() == [[5, 5], [15, 5], [25, 5], [25, 12]] and cost.tolist() == [27.0] and length.tolist() == [27.0]


def test_a_freed_cell_newly_connects_a_goal():
    pts, parent, vcost = _chain(4)
    og8 = np.zeros((64, 32), dtype=np.uint8)
    og8[:, 15] = 1  # a closed wall between the chain and the goal
    goal = [(17, 25)]
    v0, c0, _ = goalref.connect(og8, pts, vcost, 4, goal)
    assert v0.tolist() == [-1]
    og8[17, 15] = 0  # one cell freed, straight under vertex 3 = (17, 10)
    a, v, c = keepref.connect(og8, pts, parent, vcost, 4, goal)
    assert a.all() and v.tolist() == [3] and c.tolist() == [12.0 + 15.0]
    a, got = keepref.routes(og8, pts, parent, vcost, 4, goal, cut=True)
    assert got[5].tolist() == [0, 3, -1] and got[2].tolist() == [27.0]


@pytest.mark.parametrize("cid", pinned_goal_cases())
def test_an_unchanged_map_keeps_every_vertex_of_a_golden_tree(cid):
    """the reference tested every edge of its trees from the parent to the child: the same walk on the same map is free again, and
    the answers over the view are goalref's / routeref's over the tree"""
    G = orchelp.golden("plans_A.npz")
    m = G.by_id[cid]
    og8 = oracle.og_u8(G.grid(m["grid"]))
    j = m["vgoal"]
    pts, vcost, parent = G.arr(cid, "pts"), G.arr(cid, "vcost"), G.arr(cid, "parent")
    free = np.argwhere(og8 == 0)
    goals = np.concatenate([[m["xgoal"]], free[np.random.default_rng(5).integers(0, len(free), size=12)], np.argwhere(og8 != 0)[:1]])
    a, v, c = keepref.connect(og8, pts, parent, vcost, j, goals)
    assert a.all() and len(a) == j
    v0, c0, _ = goalref.connect(og8, pts, vcost, j, goals)
    assert np.array_equal(v, v0) and np.array_equal(c, c0) and (v[0], c[0]) == (parent[j], vcost[j])
    for cut in (False, True):
        a, got = keepref.routes(og8, pts, parent, vcost, j, goals, cut=cut)
        for g, w in zip(got, routeref.routes(og8, pts, vcost, parent, j, goals, cut=cut)):
            assert g.dtype == w.dtype and np.array_equal(g, w)


# ------------------------------------------------------------------------------------------------ the planner's state rules
def _with_keep(p, seen):
    """the oracle stand-in has no keep_tree: one that records the grid it would have run on"""
    dev = p._device

    def device():
        ctx = dev()
        ctx.keep_tree = lambda: seen.append(ctx.og8.copy()) or np.ones(3, dtype=bool)
        return ctx

    p._device = device
    return p


def test_keep_tree_does_what_set_og_does_and_keeps_the_tree():
    p, T, gv = wall64_planned()
    seen = []
    _with_keep(p, seen)
    og2 = wall64_og()
    og2[10:12, 20:30] = 1
    alive = p.keep_tree(og2)
    assert alive.tolist() == [True] * 3 and p._tree_resident == "device" and p.og is og2 and not p._grid_dirty
    assert np.array_equal(seen[0], oracle.og_u8(og2)) and np.array_equal(p.free, np.argwhere(og2 == 0))
    T2, gv2 = p.plan(WALL64_XS, WALL64_XG)  # a later plan() plans on the new map
    assert p.og is og2 and p._tree_resident == "device" and len(seen) == 1
    for pt in T2.__dict__["_lazy"][1][:p.last_stats["j"]]:
        assert og2[pt[0], pt[1]] == 0


def test_keep_tree_refuses_what_connect_goals_refuses_and_another_shape():
    og2 = wall64_og()
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        amd.RRTStar(wall64_og(), 300, 12, pbar=False).keep_tree(og2)
    for setter in (lambda p: p.set_og(wall64_og()), lambda p: p.set_n(300)):
        p, T, gv = wall64_planned()
        setter(p)
        with pytest.raises(RuntimeError, match="plan\\(\\) first"):
            p.keep_tree(og2)
    p, T, gv = wall64_planned()
    _with_keep(p, [])
    with pytest.raises(ValueError, match="planned on"):
        p.keep_tree(np.zeros((64, 47), dtype=np.int64))
    assert p._tree_resident == "device" and p.og.shape == (64, 48)  # nothing happened
    p.keep_tree(og2)

    def costfn(vcosts, points, v, x):
        return vcosts[v] + 2.0 * amd.r2norm(points[v] - x)

    h = amd.RRTStar(wall64_og(), 120, 12, costfn=costfn, pbar=False, seed=0)
    h._costfn_provider = orchelp.NumpyProvider(oracle.og_u8(wall64_og()))
    h.plan(WALL64_XS, WALL64_XG)
    with pytest.raises(ValueError, match="host route"):
        h.keep_tree(og2)
    # a keep that fails on the device leaves no tree for the grid that is now uploaded
    p, T, gv = wall64_planned()

    def boom():
        raise RuntimeError("device")

    p._device = lambda: SimpleNamespace(keep_tree=boom)
    with pytest.raises(RuntimeError, match="device"):
        p.keep_tree(og2)
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.connect_goals([(5, 5)])


def test_keep_tree_resident_selects_the_frame_and_keeps_the_tree():
    p, T, gv = wall64_planned()
    picked = []
    p._ctx = SimpleNamespace(keep_tree=lambda: np.ones(2, dtype=bool))
    frames = [wall64_og(), wall64_og()]
    frames[1][40:42, 10:20] = 1
    grids = SimpleNamespace(ctx=p._ctx, host=frames, select=picked.append)
    alive = p.keep_tree_resident(grids, 1)
    assert picked == [1] and alive.tolist() == [True, True] and p._tree_resident == "device" and p.og is frames[1] and not p._grid_dirty
    assert np.array_equal(p.free, np.argwhere(frames[1] == 0))
    with pytest.raises(ValueError, match="different device context"):
        p.keep_tree_resident(SimpleNamespace(ctx=object(), host=frames, select=picked.append), 0)
    with pytest.raises(ValueError, match="planned on"):
        p.keep_tree_resident(SimpleNamespace(ctx=p._ctx, host=[np.zeros((8, 8))], select=picked.append), 0)
    assert picked == [1] and p._tree_resident == "device"

    # frames that are gone: select raises before anything changed on the device, so the tree stays, on the grid it has
    def gone(k=0):
        raise RuntimeError("the device frames of this DeviceGrids are gone")

    with pytest.raises(RuntimeError, match="gone"):
        p.keep_tree_resident(SimpleNamespace(ctx=p._ctx, host=[wall64_og(), wall64_og()], select=gone), 0)
    assert p._tree_resident == "device" and p.og is frames[1]
    # a keep that fails on the device after the frame was selected leaves no tree for that frame
    boom = SimpleNamespace(keep_tree=gone)
    p._ctx = boom
    with pytest.raises(RuntimeError, match="gone"):
        p.keep_tree_resident(SimpleNamespace(ctx=boom, host=frames, select=picked.append), 0)
    assert picked == [1, 0] and p._tree_resident is None
    p._ctx = grids.ctx
    p._tree_resident = "device"
    p.set_og_resident(grids, 0)  # still drops the tree
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.keep_tree_resident(grids, 1)


@pytest.mark.parametrize("cls", [RRTDubins, RRTStarDubins])
def test_the_dubins_planners_refuse(cls):
    kw = dict(r_rewire=10) if cls is RRTStarDubins else {}
    p = cls(wall64_og(), 100, rho=3.0, pbar=False, **kw)
    with pytest.raises(ValueError, match="Dubins"):
        p.keep_tree(wall64_og())
    with pytest.raises(ValueError, match="Dubins"):
        p.keep_tree_resident(None, 0)
