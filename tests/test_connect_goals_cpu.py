"""CPU: what RRT.connect_goals / RRT.paths_to decide without the device, and the host check of the GPU tests (goalref.py)
pinned by the reference's goldens.  The device side is tests/test_connect_goals_gpu.py."""
import numpy as np
import pytest

import goalref
import oracle
import orchelp
from plannedcases import WALL64_XG, WALL64_XS, pinned_goal_cases, wall64_og, wall64_planned
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins


def test_no_tree_before_plan_and_after_the_setters():
    p = amd.RRTStar(wall64_og(), 300, 12, pbar=False)
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.connect_goals([(5, 5)])
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.paths_to(None, [(5, 5)])
    for setter in (lambda p: p.set_og(wall64_og()), lambda p: p.set_n(300)):
        p, T, gv = wall64_planned()
        assert p._tree_resident == "device"
        setter(p)
        with pytest.raises(RuntimeError, match="plan\\(\\) first"):
            p.connect_goals([(5, 5)])
        p.plan(WALL64_XS, WALL64_XG)
        assert p._tree_resident == "device"


def test_no_tree_after_set_og_resident():
    from types import SimpleNamespace

    p, T, gv = wall64_planned()
    p._ctx = object()  # (the stand-in planner has no device context of its own; set_og_resident only compares identities)
    grids = SimpleNamespace(ctx=p._ctx, host=[wall64_og(), wall64_og()], select=lambda k: None)
    assert p._tree_resident == "device"
    p.set_og_resident(grids, 1)
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.connect_goals([(5, 5)])
    p.plan(WALL64_XS, WALL64_XG)
    assert p._tree_resident == "device"


def test_a_host_plan_that_raised_leaves_no_tree():
    p = amd.RRTStar(wall64_og(), 50, 12, costfn=lambda vc, pts, v, x: vc[v] + 1.0, pbar=False, rewire="correct")
    with pytest.raises(ValueError, match="rewire"):
        p.plan(WALL64_XS, WALL64_XG)
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.connect_goals([(5, 5)])


def test_the_host_route_has_no_resident_tree():
    og = wall64_og()

    def costfn(vcosts, points, v, x):
        return vcosts[v] + 2.0 * amd.r2norm(points[v] - x)

    p = amd.RRTStar(og, 120, 12, costfn=costfn, pbar=False, seed=0)
    p._costfn_provider = orchelp.NumpyProvider(oracle.og_u8(og))
    p.plan(WALL64_XS, WALL64_XG)
    assert p.last_route == "host"
    with pytest.raises(ValueError, match="host route.*cost function"):
        p.connect_goals([(5, 5)])
    with pytest.raises(ValueError, match="not resident"):
        p.paths_to(None, [(5, 5)])


@pytest.mark.parametrize("cls", [RRTDubins, RRTStarDubins])
def test_the_dubins_planners_refuse(cls):
    kw = dict(r_rewire=10) if cls is RRTStarDubins else {}
    p = cls(wall64_og(), 100, rho=3.0, pbar=False, **kw)
    with pytest.raises(ValueError, match="Dubins"):
        p.connect_goals([(5, 5)])
    with pytest.raises(ValueError, match="Dubins"):
        p.paths_to(None, [(5, 5)])


@pytest.mark.parametrize("bad", [[1, 2, 3], [[1, 2, 3]], [[[1, 2]]], 5, [[1.5, 2.0]], [[np.nan, 2.0]], [[64, 0]], [[0, 48]], [[-1, 0]], [(5, 5), (5, 99)]])
def test_malformed_goals(bad):
    p, T, gv = wall64_planned(50)
    with pytest.raises(ValueError, match="goal"):
        p.connect_goals(bad)
    with pytest.raises(ValueError, match="goal"):
        amd.RRTStar(wall64_og(), 50, 12, pbar=False).connect_goals(bad)  # (the argument is looked at first)


def test_goal_arrays_that_are_taken():
    p, T, gv = wall64_planned(50)
    seen = []
    p._device = lambda: type("Ctx", (), {"connect_goals": staticmethod(lambda g: seen.append(g) or (np.zeros(len(g), np.int32), np.zeros(len(g))))})
    for goals, m in (((5, 5), 1), ([[5.0, 6.0]], 1), (np.zeros((0, 2), dtype=int), 0), (np.array([[63, 47], [0, 0]], dtype=np.uint16), 2)):
        v, c = p.connect_goals(goals)
        assert seen[-1].shape == (m, 2) and seen[-1].dtype == np.int64 and len(v) == m
    assert seen[1].tolist() == [[5, 6]]


def test_paths_to_walks_the_parents_of_a_golden_tree(monkeypatch):
    G = orchelp.golden("plans_A.npz")
    m = next(m for m in G.manifest if m["alg"] == 1 and m["n"] >= 400 and m.get("rows") == m["n"] + 1 and m["grid"] != "empty43x100")
    og = G.grid(m["grid"])
    p = orchelp.use_oracle(orchelp.make_planner(amd, m, og))
    T, gv = p.plan(np.array(m["xstart"]), np.array(m["xgoal"]))
    assert gv == m["vgoal"]
    parent, pts = G.arr(m["id"], "parent"), G.arr(m["id"], "pts")
    goals = np.array([m["xgoal"], [0, 0], m["xstart"], [1, 2]])
    vertex = np.array([parent[gv], -1, 0, gv - 1], dtype=np.int32)
    calls = []

    def fake(g):
        calls.append(np.array(g))
        return vertex, np.zeros(len(vertex))

    for lazy in (True, False):
        if not lazy:
            T.adj  # noqa: B018  (materialises the graph: the parent walk goes through networkx's dictionaries)
        monkeypatch.setattr(p, "connect_goals", fake)
        paths = p.paths_to(T, goals)
        assert len(calls) == (1 if lazy else 2) and np.array_equal(calls[-1], goals)  # one device call for all goals
        assert paths[1] is None and len(paths) == 4
        assert np.array_equal(paths[0], pts[G.arr(m["id"], "path")])  # the reference's own route to its goal
        assert paths[2].tolist() == [m["xstart"], m["xstart"]]
        want, v = [[1, 2]], gv - 1
        while v != -1:
            want.append(pts[v].tolist())
            v = parent[v]
        assert paths[3].tolist() == want[::-1] and paths[3].dtype == np.int64


@pytest.mark.parametrize("cid", pinned_goal_cases())
def test_the_host_check_reproduces_the_references_goal_row(cid):
    """goalref.connect_one on the golden tree before its goal row gives the row the reference appended: (parent, cost)"""
    G = orchelp.golden("plans_A.npz")
    m = G.by_id[cid]
    og8 = oracle.og_u8(G.grid(m["grid"]))
    j = m["vgoal"]
    pts, vcost, parent = G.arr(cid, "pts"), G.arr(cid, "vcost"), G.arr(cid, "parent")
    v, c, tried = goalref.connect_one(og8, pts, vcost, j, m["xgoal"])
    assert (v, c) == (parent[j], vcost[j]) and 1 <= tried <= j
    rv, rc, rt = goalref.connect(og8, pts, vcost, j, [m["xgoal"], m["xgoal"]])
    assert rv.tolist() == [v, v] and rc.tolist() == [c, c] and rv.dtype == np.int32
    wall = np.argwhere(og8 != 0)
    if len(wall):
        assert goalref.connect_one(og8, pts, vcost, j, wall[0]) == (-1, np.inf, j)


def test_pinned_cases_exist():
    assert len(pinned_goal_cases()) == 3
