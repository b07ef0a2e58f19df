"""CPU: the host restatement of relax_poses (tests/poserelaxref.py) pinned -- its two forms against each other, its certificate against
planted errors --, the inputs of tests/poserelaxcases.py held to what each is for, and the binding, the argument checks and the refusal
texts of RRTDubins / RRTStarDubins .relax_poses and _ffi that need no device (tests/golden/pose_relax_refusals.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import poserelaxcases as pc
import poserelaxref
import poseref
from rrtplanner_amd import _ffi
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "pose_relax_refusals.json")) as f:
    GOLDEN = json.load(f)

ALL = list(pc.WORKLOADS) + list(pc.FIXTURES) + [f"sized{j}" for j in pc.SIZES]
# measured: vertices cheaper of j, summed cost after / before
FALLS = {"A": (343, 402, 0.71), "C": (2022, 2176, 0.78), "D": (166, 176, 0.64), "E": (139, 175, 0.87)}


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ALL)
def test_dijkstra_and_jacobi_agree_and_the_certificate_is_clean(name):
    w, r, X = pc.fixture(name)
    G = X.G
    cj, rounds = poserelaxref.jacobi(G, X.in_cost)
    assert np.array_equal(_bits(cj), _bits(X.cstar)) and 0 <= rounds < max(G.j, 2)
    # the tree's own costs are a valid start: c[parent] + word == c[v], bit for bit, on every edge
    assert np.array_equal(_bits(X.in_cost[1:]), _bits(X.in_cost[X.in_parent[1:]] + G.plen[1:]))
    assert X.cstar[0] == 0.0 and np.all(X.cstar <= X.in_cost) and sorted(X.ids.tolist()) == list(range(w.j))
    assert X.sweeps <= X.words <= X.pairs
    assert pc.certified(w, r, X) == []
    print(name, dict(j=w.j, fell=X.fell, rounds=rounds, ties=X.ties, words=X.words, sweeps=X.sweeps, pairs=X.pairs))


@pytest.mark.parametrize("name", list(FALLS))
def test_the_costs_fall_as_measured(name):
    w, r, X = pc.fixture(name)
    fell, j, ratio = FALLS[name]
    assert w.j == j and X.fell == fell and 2 * X.fell > j
    got = X.cstar.sum() / X.in_cost.sum()
    assert got < 0.95 and abs(got - ratio) < 0.005, got
    assert int((X.parent > np.arange(len(X.parent))).sum()) == 0  # (after the renumbering; before it, many parents have the higher number)
    assert int((X.new_parent[1:] > np.arange(1, w.j)).sum()) >= j // 8


def test_the_certificate_flags_each_planted_error():
    w, r, X = pc.fixture("blocked70")
    R, old = pc.R_of(r), poserelaxref.old_edges_of(X.in_parent, X.order)
    j = len(X.pts)

    def kinds(pts, head, parent, cost, prev=X.order):
        return {what for what, _ in poserelaxref.certify(w.og8, pts, head, parent, cost, R, w.rho, w.nh, old, prev=prev)}

    assert kinds(X.pts, X.head, X.parent, X.vcost) == set()
    # a cost one ulp off
    cost = X.vcost.copy()
    cost[j // 2] = np.nextafter(cost[j // 2], np.inf)
    assert "cost is not parent + edge" in kinds(X.pts, X.head, X.parent, cost)
    # a blocked parent edge: a vertex behind the wall hung on a vertex of the cluster, its cost made to fit
    behind = int(np.flatnonzero(X.pts[:, 0] >= 33)[-1])
    front = next(k for k in np.flatnonzero((X.pts[:, 0] >= 16) & (X.pts[:, 0] <= 22) & (X.pts[:, 1] >= 26)).tolist()
                 if k < behind and (k, behind) not in old and not poserelaxref.swept_free(w.og8, X.pts, X.head, k, behind, w.rho, w.nh))
    parent, cost = X.parent.copy(), X.vcost.copy()
    parent[behind] = front
    cost[behind] = cost[front] + poserelaxref.word(X.pts, X.head, front, behind, w.rho, w.nh)
    got = kinds(X.pts, X.head, parent, cost)
    assert "parent edge outside E" in got and "cost is not parent + edge" not in got
    # a missed improvement: a leaf whose cost fell, put back on its old parent at the cost that edge gives
    inner = set(X.parent.tolist())
    k = next(k for k in range(1, j) if k not in inner and X.cstar[X.order[k]] < X.in_cost[X.order[k]])
    new = np.full(j, -1, dtype=np.int64)
    new[X.order] = np.arange(j)
    op = int(new[X.in_parent[X.order[k]]])
    parent, cost = X.parent.copy(), X.vcost.copy()
    parent[k], cost[k] = op, cost[op] + poserelaxref.word(X.pts, X.head, op, k, w.rho, w.nh)
    assert cost[k] > X.vcost[k]
    assert kinds(X.pts, X.head, parent, cost) - {"parent above child"} == {"an edge of E improves"}
    # a wrong parent on a tie: the vertex of `ties8` that two parents give the same cost, hung on the one the rule does not choose
    w2, r2, Y = pc.fixture("ties8")
    v = int(np.flatnonzero(Y.order == 3)[0])
    loser = int(np.flatnonzero(Y.order == 1)[0])
    parent = Y.parent.copy()
    assert parent[v] == int(np.flatnonzero(Y.order == 2)[0]) and loser < v
    parent[v] = loser
    bad = poserelaxref.certify(w2.og8, Y.pts, Y.head, parent, Y.vcost, pc.R_of(r2), w2.rho, w2.nh, poserelaxref.old_edges_of(Y.in_parent, Y.order), prev=Y.order)
    assert {what for what, _ in bad} == {"parent is not the smallest (cost, previous number)"}


@pytest.mark.parametrize("name", ["E", "duplicate", "blocked144"])
def test_relaxing_twice_lowers_nothing(name):
    w, r, X = pc.fixture(name)
    Y = poserelaxref.relax(w.og8, X.pts, X.head, X.parent, X.vcost, len(X.pts), pc.R_of(r), w.rho, w.nh)
    assert Y.fell == 0 and np.array_equal(_bits(Y.cstar), _bits(X.vcost))
    assert poserelaxref.certify(w.og8, Y.pts, Y.head, Y.parent, Y.vcost, pc.R_of(r), w.rho, w.nh, poserelaxref.old_edges_of(Y.in_parent, Y.order), prev=Y.order) == []


# ------------------------------------------------------------------------------------------------ what each input is for
def test_an_exact_tie_goes_to_the_cheaper_parent_not_to_the_lower_number():
    w, r, X = pc.fixture("ties8")
    assert np.array_equal(X.in_pts, [(10, 10), (15, 10), (13, 10), (20, 10)]) and np.array_equal(X.in_parent, [-1, 0, 1, 1]) and np.all(X.in_head == 0)
    assert X.cstar.tolist() == [0.0, 5.0, 3.0, 10.0] and X.in_cost[2] > 10.0
    G = X.G
    ok = [int(u) for u, ln in zip(G.into[3].tolist(), G.into_len[3].tolist()) if X.cstar[u] + ln == X.cstar[3] and G.edge(u, 3)]
    assert ok == [1, 2] and X.new_parent[3] == 2  # costs 5 and 3: the cost-3 parent wins, which has the higher number


def test_a_vertex_that_repeats_the_start_pose_is_a_zero_length_edge():
    w, r, X = pc.fixture("duplicate")
    poseref.check_tie_duplicate(w, "first")
    k = w.dup
    assert X.G.plen[k] == 0.0 and X.cstar[k] == 0.0 and X.new_parent[k] == 0
    assert not np.any(X.new_parent == k)  # every word from the duplicate is the root's: the root has the smaller (cost, number)
    assert X.fell > 0


def test_an_old_parent_edge_longer_than_r_carries_a_cheaper_path_to_its_subtree():
    w, r, X = pc.fixture("long_edge")
    G, R = X.G, pc.R_of(r)
    assert not w.star  # an RRTDubins tree: the parent is the nearest vertex, however far
    through = [v for v in range(1, G.j) if G.D2[G.parent[v], v] >= R and X.new_parent[v] == G.parent[v] and X.cstar[v] < X.in_cost[v]]
    assert through, "no vertex gets cheaper through an old edge that is longer than r"
    assert int((G.D2[G.parent[1:], np.arange(1, G.j)] >= R).sum()) >= 10


@pytest.mark.parametrize("name,least", [("blocked70", 65), ("blocked144", 129)])
def test_blocked_cheaper_candidates_past_one_and_two_wavefronts(name, least):
    w, r, X = pc.fixture(name)
    G = X.G
    assert int((w.og8[30:32, :] == 0).sum()) == 10 and np.all(w.og8[30:32, 2:7] == 0)  # a wall with one gap
    most, free_after = 0, 0
    for v in range(1, G.j):
        cheaper = [(X.cstar[u] + ln, u) for u, ln in zip(G.into[v].tolist(), G.into_len[v].tolist()) if X.cstar[u] + ln < X.cstar[v] and u != G.parent[v]]
        assert not any(G.free(u, v) for _, u in cheaper)  # (the fixpoint: every cheaper candidate is blocked)
        if len(cheaper) > most:
            most, free_after = len(cheaper), int(X.new_parent[v] != G.parent[v])
    assert most >= least, most


def test_a_box_with_more_surviving_candidates_than_the_lds_list_holds():
    w, r, X = pc.fixture("crowd")
    G = X.G
    cap = pc.list_cap()
    assert cap >= 64
    most = 0
    for v in range(1, G.j):  # the survivors of the first round's screen against the starting costs (the device's float bound lets no fewer through)
        us = G.into[v]
        bound = min(X.in_cost[v], X.in_cost[G.parent[v]] + G.plen[v])
        most = max(most, int((X.in_cost[us] + np.sqrt(G.D2[us, v].astype(np.float64)) < bound).sum()))
    assert most > cap, (most, cap)


def test_a_chain_that_takes_at_least_100_jacobi_rounds():
    w, r, X = pc.fixture("chain")
    assert w.j == 260 and np.array_equal(w.ro.parent[1:w.j], np.arange(w.j - 1))
    assert poserelaxref.jacobi(X.G, X.in_cost)[1] >= 100 and X.fell >= 250


@pytest.mark.parametrize("j", pc.SIZES)
def test_trees_of_exactly_these_sizes(j):
    w, r, X = pc.fixture(f"sized{j}")
    assert w.j == j == len(X.ids)
    if j >= 63:  # (not an input the call leaves as it is)
        assert X.fell >= 8 and X.sweeps >= 8


# ------------------------------------------------------------------------------------------------ binding and arguments, no device
NAMES = ("rrt_batch_relax_poses", "rrt_batch_relax_poses_ms", "rrt_batch_relax_poses_stats", "rrt_plan_relax_poses", "rrt_plan_relax_poses_ms",
         "rrt_plan_relax_poses_stats")


def test_the_header_and_the_binding_carry_the_six_symbols():
    hdr = open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    for s in NAMES:
        assert s in _ffi.SYMBOLS and f"int {s}(" in hdr
    L = _ffi.lib()
    assert L.rrt_batch_relax_poses.argtypes[2] is ctypes.c_int64 and len(L.rrt_batch_relax_poses.argtypes) == 8 and len(L.rrt_plan_relax_poses.argtypes) == 7
    j0 = ctypes.c_int32(0)
    assert L.rrt_batch_relax_poses(None, 0, 576, None, 0, ctypes.byref(j0), None, ctypes.byref(j0)) == _ffi.RRT_E_ARG
    assert L.rrt_batch_relax_poses_ms(None, None, 9) == _ffi.RRT_E_ARG and L.rrt_batch_relax_poses_stats(None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_relax_poses(None, 576, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_relax_poses_ms(None, None, 9) == _ffi.RRT_E_ARG and L.rrt_plan_relax_poses_stats(None, None) == _ffi.RRT_E_ARG


def _refused(key, fn, *args, **fmt):
    code, text = GOLDEN[key]
    assert code == "ValueError"
    with pytest.raises(ValueError) as e:
        fn(*args)
    assert str(e.value) == text.format(**fmt), str(e.value)


def test_the_classes_refuse_with_the_golden_texts_before_any_device_call():
    og = np.zeros((32, 32), dtype=np.int64)
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 8, pbar=False), amd.RRTStarInformed(og, 50, 8, 4, pbar=False)):
        _refused("straight_line_planner", p.relax_poses, 8)
        assert p._ctx is None
    for p in (RRTDubins(og, 50, 4.0, pbar=False), RRTStarDubins(og, 50, 8, 4.0, pbar=False)):
        _refused("dubins_planner_relax", p.relax, 8)  # relax keeps refusing a Dubins planner, with the text it had
        _refused("radius_not_positive", p.relax_poses, 0)
        with pytest.raises(RuntimeError, match="relax_poses: no tree on the device"):
            p.relax_poses(8)
        assert p._ctx is None and p.last_relax is None
    _refused("no_radius", RRTDubins(og, 50, 4.0, pbar=False).relax_poses)
    p = RRTStarDubins(og, 50, 8, 4.0, pbar=False)
    with pytest.raises(RuntimeError, match="relax_poses: no tree on the device"):
        p.relax_poses()  # r defaults to r_rewire


def test_the_device_refusals_are_in_the_golden_file():
    for key in ("non_dubins_batch", "dubins_batch_relax", "q_out_of_range", "unfinished_query", "no_plan", "grid_not_kept", "m_negative", "root_blocked",
                "room", "r2_not_positive", "heading_out_of_range", "cell_outside", "ms_none", "stats_none", "plan_ms_none", "null", "grid_shape"):
        code, text = GOLDEN[key]
        assert code in (_ffi.RRT_E_ARG, _ffi.RRT_E_UNSUPPORTED) and text
    src = open(os.path.join(ROOT, "rrtplanner_amd", "csrc", "rrt_tree_calls.hip")).read()
    assert "r2=%lld: the threshold of the squared distance has to be positive" in src and '"rrt_batch_relax_poses"' in src
