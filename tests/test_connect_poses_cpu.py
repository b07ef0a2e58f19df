"""CPU: the host side of connect_poses -- the restatement the GPU tests compare with (poseref.py) against the oracle's own goal
decision, the lower bound the kernel sorts and prunes by, the planners' validation and the any-heading reduction."""
import numpy as np
import pytest

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
