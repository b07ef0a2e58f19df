"""CPU: the host side of connect_poses -- the restatement the GPU tests compare with (poseref.py) against the oracle's own goal
decision, the lower bound the kernel sorts and prunes by, the planners' validation and the any-heading reduction; and the
conditions under which the GPU tests' made-up trees (exact ties, trees of exactly j vertices, the fuzz) and the independent audit of
oracle/dubins_ref.c are worth something."""
import numpy as np
import pytest

import oracle
import poseref
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

NAMES = sorted(poseref.SPECS)


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_gives_the_oracles_own_goal_and_the_workload_is_worth_running(name):
    w = poseref.workload(name)
    poseref.check_conditions(w)
    if name == "C":
        assert w.j > 2 * 1024 and w.rank.max() > 1024  # a winner beyond the first round of one vertex per lane
    if name.startswith("G"):
        # a goal that IS a tree pose (vertex j // 2, the start): the word to itself has length zero, or -- where the reduction of
        # a zero angle lands just below 2 pi -- is a full turn; both are exercised as they come
        v, turn = w.j // 2, poseref.TWOPI * w.rho
        for g, k in ((0, v), (2, 0)):
            extra = w.c[g, k] - w.ro.vcost[k]
            assert extra == 0.0 or abs(extra - turn) < 1e-9, (g, k, extra)


def _chord_lower_bound_f32(V, d2):
    """chord_lower_bound of rrt_cell_stream.h, operation by operation in float32 (numpy's root is the correctly rounded one, the
    hardware's is within an ulp: the bound's margins cover that, see there)"""
    f = np.float32
    s = (V.astype(f) + np.sqrt(d2.astype(f))) * (f(1.0) - f(1.0e-6)) - f(4.0e-3)
    assert s.dtype == f
    return np.maximum(s, f(0.0))


@pytest.mark.parametrize("name", NAMES)
def test_the_chord_bound_is_below_every_cost(name):
    """what the kernel's walk may end on: bound <= c[k] for every (vertex, goal) pair; equality only at cost 0"""
    w = poseref.workload(name)
    pts = w.ro.pts[:w.j].astype(np.int64)
    worst = np.inf
    for g, goal in enumerate(w.goals):
        d = pts - goal[:2]
        lb = _chord_lower_bound_f32(w.ro.vcost[:w.j], d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64)
        bad = np.flatnonzero(lb > w.c[g])
        assert bad.size == 0, (name, g, bad[:5], lb[bad[:5]], w.c[g][bad[:5]])
        eq = lb == w.c[g]
        assert np.all(w.c[g][eq] == 0.0)
        worst = min(worst, float((w.c[g] - lb).min()))
    assert worst >= 0.0


def test_poses_are_validated_on_the_host():
    p = RRTStarDubins(np.zeros((40, 30), dtype=int), 100, 10, 3.0, n_headings=16, pbar=False)
    ok = p._pose_array([(0, 0, 0), (39, 29, 15), (5, 5, -1)])
    assert ok.dtype == np.int64 and ok.shape == (3, 3)
    assert p._pose_array((3, 4, 5)).tolist() == [[3, 4, 5]] and p._pose_array(np.array([[3.0, 4.0, 5.0]])).tolist() == [[3, 4, 5]]
    assert p._pose_array(np.zeros((0, 3), dtype=int)).shape == (0, 3)
    for bad, word in (([(1, 2)], "shape"), ([[(1, 2, 3)]], "shape"), ([(1.5, 2, 3)], "integer"), ([(1, 2, np.nan)], "integer"),
                      ([(40, 0, 0)], "outside"), ([(0, 30, 0)], "outside"), ([(-1, 0, 0)], "outside"), ([(0, 0, 16)], "heading"),
                      ([(0, 0, -2)], "heading"), ([(0, 0, 0), (1, 1, 99)], "pose 1")):
        with pytest.raises(ValueError, match=word):
            p.connect_poses(bad)  # (before any device call: there is no tree and no device here)


@pytest.mark.parametrize("cls", [RRTDubins, RRTStarDubins])
def test_no_tree_before_plan(cls):
    args = (np.zeros((40, 30), dtype=int), 100) + ((10,) if cls is RRTStarDubins else ()) + (3.0,)
    p = cls(*args, pbar=False)
    with pytest.raises(RuntimeError, match="plan"):
        p.connect_poses([(5, 5, 0)])
    with pytest.raises(RuntimeError, match="plan"):
        p.paths_to_poses(None, [(5, 5, -1)])
    # the straight-line calls stay refused for a Dubins planner, as before
    with pytest.raises(ValueError, match="Dubins"):
        p.connect_goals([(5, 5)])
    with pytest.raises(ValueError, match="Dubins"):
        p.keep_tree(np.zeros((40, 30), dtype=int))


def test_the_straight_line_planners_name_connect_goals():
    og = np.zeros((40, 30), dtype=int)
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 10, pbar=False), amd.RRTStarInformed(og, 50, 10, 5, pbar=False)):
        with pytest.raises(ValueError, match="connect_goals"):
            p.connect_poses([(5, 5, 0)])


class _HostDevice:
    """stands in for the device context: answers connect_poses from the restatement"""

    def __init__(self, w):
        self.w, self.calls = w, []

    def connect_poses(self, poses):
        w = self.w
        self.calls.append(np.array(poses))
        v, c, _ = poseref.connect(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, poses, w.rho, w.nh)
        return v, c


def test_any_heading_is_the_cost_heading_smallest_connected_pose():
    w = poseref.workload("G256")  # 256 headings: the widest expansion
    p = RRTStarDubins(w.og, w.n, 12, w.rho, n_headings=w.nh, pbar=False)
    dev = _HostDevice(w)
    p._device = lambda: dev
    p._tree_resident = "device"
    ob = np.argwhere(w.og8 != 0)[0]
    cells = [w.goals[5, :2], w.goals[6, :2], ob]
    poses = [(cells[0][0], cells[0][1], -1), tuple(w.goals[7]), (cells[1][0], cells[1][1], -1), (ob[0], ob[1], -1)]
    vertex, cost, heading = p.connect_poses(poses)
    assert len(dev.calls) == 1 and dev.calls[0].shape == (3 * w.nh + 1, 3) and dev.calls[0][:, 2].min() == 0  # concrete headings only, one call
    assert vertex.dtype == np.int32 and cost.dtype == np.float64 and heading.dtype == np.int64
    for k, cell in ((0, cells[0]), (2, cells[1]), (3, ob)):
        assert (vertex[k], cost[k], heading[k]) == poseref.any_heading(w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, cell, w.rho, w.nh), k
    assert (vertex[1], cost[1], heading[1]) == (w.vertex[7], w.cost[7], w.goals[7, 2])
    assert vertex[0] >= 0 and vertex[2] >= 0 and (vertex[3], cost[3], heading[3]) == (-1, np.inf, -1)
    # a concrete pose that does not connect keeps its heading; the answer -1 / inf
    v1, c1, h1 = p.connect_poses((ob[0], ob[1], 3))
    assert (v1[0], c1[0], h1[0]) == (-1, np.inf, 3)


# ------------------------------------------------------------------------------------------------ exact ties
def _own_goal_agrees_with_the_oracle(w):
    found, vgoal, parent, cost = poseref.own_goal_row(w)
    assert tuple(w.goals[-1]) == w.xg or tuple(w.goals[0]) == w.xg
    g = len(w.goals) - 1 if tuple(w.goals[-1]) == w.xg else 0
    assert (w.vertex[g], w.cost[g]) == (parent, cost) and found == (w.vertex[g] >= 0)


@pytest.mark.parametrize("place", list(poseref.TIE_PLACES))
@pytest.mark.parametrize("star", [0, 1])
@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_a_duplicate_of_the_start_pose_ties_with_it_for_every_goal(rho, nh, star, place):
    """c[0] == c[dup] bit for bit whatever the goal, the duplicate where the GPU test wants it, and the restatement never answers it"""
    w = poseref.tie_duplicate(rho, nh, star, place)
    poseref.check_tie_duplicate(w, place)
    _own_goal_agrees_with_the_oracle(w)
    assert len(w.goals) >= 12 and len({(g[0], g[1]) for g in w.goals[:nh].tolist()}) == 1 and sorted(w.goals[:nh, 2].tolist()) == list(range(nh))


@pytest.mark.parametrize("fillers", [0, 100])
@pytest.mark.parametrize("star", [0, 1])
@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_collinear_and_mirrored_poses_tie_exactly(rho, nh, star, fillers):
    a, b, iL, iR = poseref.tie_collinear(rho, nh, star, fillers)
    poseref.check_tie_collinear(a, b, iL, iR)
    assert iL == 2 and iR == fillers + 3
    _own_goal_agrees_with_the_oracle(a)
    _own_goal_agrees_with_the_oracle(b)


def test_a_chain_of_collinear_poses_ties_in_every_comparison():
    w = poseref.tie_chain()
    poseref.check_tie_chain(w)
    _own_goal_agrees_with_the_oracle(w)
    pts = w.ro.pts[:w.j].astype(np.int64)
    d = pts - w.goals[0, :2]
    lb = _chord_lower_bound_f32(w.ro.vcost[:w.j], d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    assert np.all(lb == lb[0])  # one bucket: integers that single precision holds exactly


# ------------------------------------------------------------------------------------------------ trees around the strides
@pytest.mark.parametrize("star", [0, 1])
@pytest.mark.parametrize("j", poseref.STRIDE_J)
def test_the_stride_trees_have_exactly_j_vertices_and_goals_of_every_kind(j, star):
    w = poseref.stride_tree(j, star)
    poseref.check_stride_tree(w, j)
    assert w.n >= j and 8 <= len(w.goals) <= 13
    W, H = w.og8.shape
    assert w.og8[tuple(w.goals[poseref.I_WALL, :2])] == 1 and {(0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0)} <= {(g[0], g[1]) for g in w.goals.tolist()}
    for g in poseref.I_BEHIND:
        assert w.vertex[g] == -1 and w.og8[tuple(w.goals[g, :2])] == 0
    # the same poses for every size
    assert np.array_equal(w.goals, np.array(poseref.STRIDE_GOALS))


# ------------------------------------------------------------------------------------------------ the fuzz
def test_the_fuzz_does_not_pass_on_nothing():
    cases = poseref.fuzz_cases()
    goals, connected, past_blocked = poseref.fuzz_coverage(cases)
    assert len(cases) >= 100 and goals == len(cases) * poseref.FUZZ_M == len(cases) * 8
    assert 4 * connected >= goals, (connected, goals)        # at least 25 % of the goals connect
    assert 20 * past_blocked >= goals, (past_blocked, goals)  # at least 5 % past a blocked first candidate
    for w in cases:
        _own_goal_agrees_with_the_oracle(w)
    # the draw reaches the corners it is there for
    assert {w.n for w in cases} == {1, 2, 17, 64, 100, 300, 800} and {w.nh for w in cases} == {1, 8, 64, 256}
    assert {w.rho for w in cases} == {0.5, 1.5, 4.0, 12.0} and {w.star for w in cases} == {0, 1}
    assert any(min(w.og8.shape) < 2 * w.rho and w.j > 1 for w in cases)  # a grid smaller than a turning circle, with a tree on it
    assert sum(int((w.og8[w.goals[:, 0], w.goals[:, 1]] != 0).sum()) for w in cases) >= 20  # goals on obstacle cells


# ------------------------------------------------------------------------------------------------ the independent audit
AUDITED = ["A", "B", "C", "D", "E", "G1", "G256"]


@pytest.mark.parametrize("name", AUDITED)
def test_the_independent_audit_is_clean_on_the_restatements_answers(name):
    """poseref prices and sweeps with include/rrt_dubins.h, the header the kernel compiles; oracle/dubins_ref.c does not include it.
    Its audit works through every vertex for every goal with libm's arithmetic."""
    w = poseref.workload(name)
    a = poseref.goals_audit(w, w.vertex, w.cost)
    assert a["words"] == a["sweeps"] == w.j * int((w.og8[w.goals[:, 0], w.goals[:, 1]] == 0).sum())
    poseref.assert_goals_audit_clean(a, w.vertex)


def _errors(a):
    return {k: a[k] for k in ("answer_wrong", "answer_blocked", "cost_mismatch", "missed", "phantom")}


def test_the_independent_audit_is_not_blind():
    w = poseref.workload("A")
    none = dict(answer_wrong=0, answer_blocked=0, cost_mismatch=0, missed=0, phantom=0)
    assert _errors(poseref.goals_audit(w, w.vertex, w.cost)) == none
    g = int(np.flatnonzero(w.vertex >= 0)[0])
    goal = tuple(w.goals[g])
    # one answer moved to another visible vertex that is more expensive
    order = np.argsort(w.c[g], kind="stable").tolist()
    k = next(k for k in order[w.rank[g] + 1:] if w.c[g, k] > w.cost[g] + 1e-3 and
             poseref.sweep_free(w.og8, w.ro.pts[k], w.ro.head[k], goal, w.rho, w.nh, w.c[g, k] - w.ro.vcost[k]))
    vertex, cost = w.vertex.copy(), w.cost.copy()
    vertex[g], cost[g] = k, w.c[g, k]
    a = poseref.goals_audit(w, vertex, cost)
    assert _errors(a) == dict(none, answer_wrong=1) and a["first_bad_goal"] == g, a
    # one cost raised by 1e-6
    cost = w.cost.copy()
    cost[g] += 1e-6
    a = poseref.goals_audit(w, w.vertex, cost)
    assert _errors(a) == dict(none, cost_mismatch=1) and a["first_bad_goal"] == g and 0.9e-6 < a["max_cost_err"] < 1.1e-6, a
    # one connected goal declared unreachable
    vertex, cost = w.vertex.copy(), w.cost.copy()
    vertex[g], cost[g] = -1, np.inf
    a = poseref.goals_audit(w, vertex, cost)
    assert _errors(a) == dict(none, missed=1) and a["first_bad_goal"] == g and a["n_connected"] == int((w.vertex >= 0).sum()) - 1, a
    # one obstacle goal given a vertex
    vertex, cost = w.vertex.copy(), w.cost.copy()
    vertex[w.i_obstacle], cost[w.i_obstacle] = 0, w.c[w.i_obstacle, 0]
    a = poseref.goals_audit(w, vertex, cost)
    assert _errors(a) == dict(none, phantom=1) and a["first_bad_goal"] == w.i_obstacle, a
    # one answer moved to a vertex behind a wall: the root of the stride tree, for the goal it can reach only through the wall
    s = poseref.stride_tree(1025, 1)
    g = len(s.goals) - 1
    assert s.vertex[g] > 0 and np.isfinite(s.c[g, 0]) and s.og8[70:73, :80].all()
    cells = oracle.dub_sweep_cells(*s.ro.pts[0], poseref.theta(s.ro.head[0], s.nh), s.goals[g, 0], s.goals[g, 1], poseref.theta(s.goals[g, 2], s.nh), s.rho)
    assert np.any((cells[:, 0] >= 70) & (cells[:, 0] < 73) & (cells[:, 1] < 80))  # the root's word runs into the wall
    vertex, cost = s.vertex.copy(), s.cost.copy()
    vertex[g], cost[g] = 0, s.c[g, 0]
    a = poseref.goals_audit(s, vertex, cost)
    assert _errors(a) == dict(none, answer_blocked=1, answer_wrong=1) and a["first_bad_goal"] == g, a  # (blocked, hence not the first minimum either)
    with pytest.raises(ValueError):
        oracle.dubins_goals_audit(s.og8, s.ro.pts, s.ro.head, s.ro.vcost, s.j, s.goals, np.full(len(s.goals), s.j), s.cost, rho=s.rho, nh=s.nh)
