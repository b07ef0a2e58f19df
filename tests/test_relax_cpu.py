"""CPU: the host restatement of relax (tests/relaxref.py) pinned -- its two forms against each other, its certificate against planted
errors, its limits against rerootref --, the inputs of tests/relaxcases.py held to what each is for, and the binding and argument
checks of RRT.relax / _ffi that need no device.

Relaxing twice: the second call starts from the first one's result, renumbered.  Its costs are the same bit for bit; its parents may
differ where a vertex has more than one qualifying parent with the same cost, because the rule breaks that tie by the vertex number
and the numbers changed.  So the test asserts only the costs and the certificate."""
import ctypes
import os

import numpy as np
import pytest

import keepref
import oracle
import relaxcases as rc
import relaxref
import rerootref
import treecalls as tc
from rrtplanner_amd import _ffi
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

ALL = list(rc.FIXTURES) + ["base0", "base1"]


def _get(name):
    if name.startswith("base"):
        c = rc.base(int(name[4]))
        return c, tc.RR, rc.relaxed(c, tc.RR)
    return rc.fixture(name)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _certified(c, r, X):
    return relaxref.certify(c["og8"], X.pts, X.parent, X.vcost, rc.R_of(r), relaxref.old_edges_of(X.in_parent, X.order))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", ALL)
def test_dijkstra_and_jacobi_agree_and_the_certificate_is_clean(name):
    c, r, X = _get(name)
    cj, rounds = relaxref.jacobi(X.E, X.D2, X.in_cost)
    assert np.array_equal(_bits(cj), _bits(X.cstar)) and 0 <= rounds < len(X.E)
    assert np.array_equal(_bits(X.in_cost[1:]), _bits(X.in_cost[X.in_parent[1:]] + np.sqrt(X.D2[X.in_parent[1:], np.arange(1, len(X.E))].astype(np.float64))))
    assert X.cstar[0] == 0.0 and np.all(X.cstar <= X.in_cost) and sorted(X.ids.tolist()) == list(range(c["ro"].j))
    assert _certified(c, r, X) == []


def test_the_certificate_flags_each_planted_error():
    c, r, X = _get("blocked70")
    R, old = rc.R_of(r), relaxref.old_edges_of(X.in_parent, X.order)
    og8, j = c["og8"], len(X.pts)

    def kinds(pts, parent, cost):
        return {what for what, _ in relaxref.certify(og8, pts, parent, cost, R, old)}

    assert kinds(X.pts, X.parent, X.vcost) == set()
    # one cost off by an ulp
    cost = X.vcost.copy()
    cost[j // 2] = np.nextafter(cost[j // 2], np.inf)
    assert "cost is not parent + edge" in kinds(X.pts, X.parent, cost)
    # a parent outside E: a vertex behind the wall hung on a vertex of the cluster, its cost made to fit
    behind = int(np.flatnonzero(X.pts[:, 0] >= 33)[-1])
    front = int(np.flatnonzero((X.pts[:, 0] >= 16) & (X.pts[:, 0] <= 22) & (X.pts[:, 1] >= 26))[0])
    assert front < behind and not oracle.collisionfree(og8, X.pts[front], X.pts[behind])[0] and (front, behind) not in old
    parent, cost = X.parent.copy(), X.vcost.copy()
    parent[behind] = front
    d = X.pts[front] - X.pts[behind]
    cost[behind] = cost[front] + np.sqrt(np.float64(int(d @ d)))
    got = kinds(X.pts, parent, cost)
    assert "parent edge outside E" in got and "cost is not parent + edge" not in got
    # a missed improving edge: a leaf whose cost fell, put back on its old parent at the cost that edge gives
    leaves = [k for k in range(1, j) if k not in set(X.parent.tolist()) and X.cstar[X.order[k]] < X.in_cost[X.order[k]]]
    k = leaves[0]
    new = np.full(j, -1, dtype=np.int64)
    new[X.order] = np.arange(j)
    op = int(new[X.in_parent[X.order[k]]])
    parent, cost = X.parent.copy(), X.vcost.copy()
    d = X.pts[op] - X.pts[k]
    parent[k], cost[k] = op, cost[op] + np.sqrt(np.float64(int(d @ d)))
    assert cost[k] > X.vcost[k]
    assert kinds(X.pts, parent, cost) - {"parent above child"} == {"an edge of E improves"}
    # a parent above its child: a vertex and its parent change numbers
    k = next(k for k in range(2, j) if X.parent[k] > 0)
    p = int(X.parent[k])
    perm = np.arange(j)
    perm[[p, k]] = [k, p]
    parent = np.where(X.parent >= 0, perm[np.maximum(X.parent, 0)], -1)[perm]
    assert kinds(X.pts[perm], parent, X.vcost[perm]) >= {"parent above child"}


@pytest.mark.parametrize("name", ["blocked70", "near1025", "ties8"])
def test_a_radius_below_every_distance_gives_the_input_tree_renumbered(name):
    c, _, _ = _get(name)
    pts, parent, cost, j = rc.tree(c)
    D2 = relaxref.d2_matrix(pts)
    R = int(D2[D2 > 0].min())
    assert R >= 1 and (D2 + np.eye(j, dtype=np.int64) * R >= R).all()  # no pair is near
    X = relaxref.relax(c["og8"], pts, parent, cost, j, R)
    Z = rerootref.reroot(c["og8"], pts, parent, j, 0)
    assert X.fell == 0 and np.array_equal(X.ids, Z.ids) and np.array_equal(X.parent, Z.parent) and np.array_equal(X.pts, Z.pts)
    assert np.array_equal(_bits(X.vcost), _bits(Z.vcost)) and np.array_equal(_bits(X.vcost), _bits(cost[X.ids]))


@pytest.mark.parametrize("name", ["long_edge", "blocked144", "base1"])
def test_relaxing_twice_leaves_the_costs(name):
    c, r, X = _get(name)
    Y = relaxref.relax(c["og8"], X.pts, X.parent, X.vcost, len(X.pts), rc.R_of(r))
    assert Y.fell == 0 and np.array_equal(_bits(Y.cstar), _bits(X.vcost))
    back = X.ids[Y.ids]  # the first input's number of every vertex of the second result
    assert np.array_equal(_bits(Y.vcost), _bits(X.cstar[X.order][Y.ids])) and sorted(back.tolist()) == list(range(len(X.pts)))
    old = relaxref.old_edges_of(Y.in_parent, Y.order)
    assert relaxref.certify(c["og8"], Y.pts, Y.parent, Y.vcost, rc.R_of(r), old) == []


def test_relax_shortens_a_rerooted_tree():
    c = rc.base(1)
    pts, parent, cost, j = rc.tree(c)
    Z = rerootref.reroot(c["og8"], pts, parent, j, j // 2)
    X = relaxref.relax(c["og8"], Z.pts, Z.parent, Z.vcost, len(Z.ids), tc.R2)
    assert len(X.ids) == len(Z.ids) and X.vcost.mean() < Z.vcost.mean() and X.fell > len(Z.ids) // 2
    print("mean cost after / before:", X.vcost.mean() / Z.vcost.mean())


def test_the_direction_of_the_walk_decides():
    c, r, X = _get("base1")
    one_way = 0
    for v in range(1, len(X.E)):
        for u in np.flatnonzero(X.D2[:, v] < tc.R2).tolist():
            if u != v and u != X.in_parent[v]:
                one_way += (u in X.E[v]) != bool(oracle.collisionfree(c["og8"], X.in_pts[v], X.in_pts[u])[0])
    Eb, _ = relaxref.candidate_edges(c["og8"], X.in_pts, X.in_parent, tc.R2, backwards=True)
    cb = relaxref.dijkstra(Eb, X.D2)
    assert one_way >= 1 and int((_bits(cb) != _bits(X.cstar)).sum()) >= 1
    print("near pairs free one way only:", one_way, "vertices with another cost:", int((_bits(cb) != _bits(X.cstar)).sum()))


# ------------------------------------------------------------------------------------------------ what each input is for
def test_ties_go_to_the_cheaper_parent_not_to_the_lower_number():
    c, r, X = _get("ties8")
    assert np.array_equal(X.in_pts, [(10, 10), (15, 10), (13, 10), (20, 10)]) and np.array_equal(X.in_parent, [-1, 0, 1, 1])
    assert X.cstar.tolist() == [0.0, 5.0, 3.0, 10.0]
    ok = [u for u in X.E[3] if X.cstar[u] + relaxref.leg(X.D2, u, 3) == X.cstar[3]]
    assert ok == [1, 2] and X.new_parent[3] == 2  # costs 5 and 3: the cost-3 parent wins, which has the higher number
    c, r, Y = _get("ties11")
    assert [u for u in Y.E[3] if Y.cstar[u] + relaxref.leg(Y.D2, u, 3) == Y.cstar[3]] == [0, 1, 2] and Y.new_parent[3] == 0


def test_the_roots_cell_sampled_again_and_an_old_edge_longer_than_r():
    c, r, X = _get("long_edge")
    assert np.array_equal(X.in_parent, [-1, 0, 1, 2, 3, 4, 4, 0])
    assert X.D2[0, 7] == 0 and X.cstar[7] == 0.0 and X.new_parent[7] == 0
    assert X.D2[3, 4] >= rc.R_of(r) and X.E[4] == [3, 5, 6] and X.new_parent[4] == 3  # the long edge is the only candidate from outside its subtree
    assert X.new_parent[3] == 0 and X.cstar[3] < X.in_cost[3]                   # the detour to its upper end is cut short ...
    assert all(X.cstar[k] < X.in_cost[k] for k in (4, 5, 6))                    # ... and the whole subtree behind it gets cheaper
    assert all(X.D2[u, k] >= rc.R_of(r) for u in (0, 1, 2, 3, 7) for k in (4, 5, 6))


@pytest.mark.parametrize("name,least", [("blocked70", 65), ("blocked144", 130)])
def test_blocked_cheaper_candidates_past_one_and_two_wavefronts(name, least):
    c, r, X = _get(name)
    R = rc.R_of(r)
    most = 0
    for v in range(1, len(X.E)):
        near = [u for u in np.flatnonzero(X.D2[:, v] < R).tolist() if u != v and u not in X.E[v]]  # (within R and blocked)
        most = max(most, sum(X.cstar[u] + relaxref.leg(X.D2, u, v) < X.cstar[v] for u in near))
    assert most >= least, most


def test_a_near_set_of_more_than_four_wavefronts():
    c, r, X = _get("near1025")
    assert c["ro"].j == 1025 and max(len(e) for e in X.E) >= 257


def test_a_chain_that_takes_hundreds_of_rounds():
    c, r, X = _get("zigzag")
    ro = c["ro"]
    assert ro.j == 1100 and np.array_equal(ro.parent[1:1100], np.arange(1099))
    d = np.diff(ro.pts[:1100], axis=0)
    assert np.all((d * d).sum(axis=1) == 10) and 6.0 < 2 * np.sqrt(10.0)
    assert relaxref.jacobi_rounds(c["og8"], *rc.tree(c), rc.R_of(r)) >= 256 and X.fell >= 1000


def test_base_has_real_ties():
    c, r, X = _get("base1")
    assert X.ties >= 1 and X.fell >= c["ro"].j // 2


# ------------------------------------------------------------------------------------------------ binding and arguments, no device
def test_the_binding_declares_the_relax_calls():
    names = ("rrt_batch_relax", "rrt_batch_relax_ms", "rrt_batch_relax_stats", "rrt_plan_relax", "rrt_plan_relax_ms", "rrt_plan_relax_stats")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rrt_hip.h")).read()
    for s in names:
        assert s in _ffi.SYMBOLS and f"int {s}(" in hdr
    L = _ffi.lib()
    assert L.rrt_batch_relax.argtypes[2] is ctypes.c_int64 and len(L.rrt_batch_relax.argtypes) == 8 and len(L.rrt_plan_relax.argtypes) == 7
    j0 = ctypes.c_int32(0)
    assert L.rrt_batch_relax(None, 0, 576, None, 0, ctypes.byref(j0), None, ctypes.byref(j0)) == _ffi.RRT_E_ARG
    assert L.rrt_batch_relax_ms(None, None, 9) == _ffi.RRT_E_ARG and L.rrt_batch_relax_stats(None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_relax(None, 576, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_relax_ms(None, None, 9) == _ffi.RRT_E_ARG and L.rrt_plan_relax_stats(None, None) == _ffi.RRT_E_ARG
    assert _ffi.RRT_E_INTERNAL == -7 and "#define RRT_E_INTERNAL (-7)" in hdr


def test_the_classes_that_do_not_relax_say_so_before_any_device_call():
    og = np.zeros((32, 32), dtype=np.int64)
    for p, why in ((amd.RRTStarInformed(og, 50, 8, 4, pbar=False), "RRTStandard and RRTStar only"),
                   (RRTStarDubins(og, 50, 8, 4.0, pbar=False), "depends on the headings"),
                   (RRTDubins(og, 50, 4.0, pbar=False), "depends on the headings"),
                   (amd.RRTStar(og, 50, 8, pbar=False, rewire="correct"), "child lists"),
                   (amd.RRTStar(og, 50, 8, pbar=False, costfn=lambda vcosts, points, v, x: vcosts[v] + 1.0), "custom cost function"),
                   (amd.RRTStandard(np.zeros((2100, 8), dtype=np.int64), 50, pbar=False), "large-grid")):
        with pytest.raises(ValueError, match="relax: .*" + why):
            p.relax(8)
        assert p._ctx is None  # nothing was created on the way
    p = amd.RRTStandard(og, 50, pbar=False)
    with pytest.raises(ValueError, match="relax: .*pass r"):
        p.relax()
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 8, pbar=False)):
        with pytest.raises(RuntimeError, match="relax: no tree on the device"):
            p.relax(8)
        assert p._ctx is None and p.last_relax is None


def test_r_m_and_room_are_checked_before_any_device_call():
    p = amd.RRTStar(np.zeros((32, 32), dtype=np.int64), 50, 8, pbar=False)
    p._tree_resident, p._grow_j0 = "device", 40  # as a plan() that left 40 vertices
    state = p.rand_gen.bit_generator.state
    with pytest.raises(ValueError, match="relax: r=0"):
        p.relax(0)
    with pytest.raises(ValueError, match="relax: m=-1"):
        p.relax(m=-1)
    with pytest.raises(ValueError, match="relax: the tree holds 40 vertices and n=50: room for 10 more samples, not 11"):
        p.relax(m=11)
    assert p._ctx is None and p.rand_gen.bit_generator.state == state and p._tree_resident == "device"
