"""CPU: the host restatement of reroot_poses (tests/poserootref.py) pinned -- against poserelaxref where the root stays, against a plain
parent walk where only old edges count, its two forms against each other, the certificate and an independent reachability --, the cases
held to what each is for, and the binding, the argument checks and the refusal texts that need no device
(tests/golden/pose_reroot_refusals.json)."""
import ctypes
import json
import os

import numpy as np
import pytest

import posekeepref
import poserelaxcases as pc
import poserelaxref
import poseref
import poserootcases as rc
import poserootref
from rrtplanner_amd import _ffi, moving
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "pose_reroot_refusals.json")) as f:
    GOLDEN = json.load(f)


def _bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def _reachable(X):
    """breadth-first reachability from vertex 0 over the edge set of the dense input, computed here: the old parent edges and the near
    pairs whose word is finite and sweeps free"""
    G = X.G
    j = G.j
    seen = np.zeros(j, dtype=bool)
    seen[0] = True
    todo = [0]
    while todo:
        u = todo.pop()
        heads = [v for v in range(1, j) if not seen[v] and (int(X.f_parent[v]) == u or (
            G.D2[u, v] < G.R and np.isfinite(poserelaxref.word(G.pts, G.head, u, v, G.rho, G.nh)) and poserelaxref.swept_free(G.og8, G.pts, G.head, u, v, G.rho, G.nh)))]
        for v in heads:
            seen[v] = True
            todo.append(v)
    return seen


def _held(w, r, X, og8=None):
    """what every result must satisfy: the two forms agree, the start is what the issue requires, the certificate is clean, the reached
    set is the reachable one"""
    G = X.G
    cj, rounds = poserootref.jacobi(G, X.start)
    assert np.array_equal(_bits(cj), _bits(X.cstar)) and 0 <= rounds < max(G.j, 2)
    assert X.start[0] == 0.0 and np.all(X.cstar <= X.start)
    assert rc.certified(w, r, X, og8) == []
    assert np.array_equal(np.isfinite(X.cstar), _reachable(X))
    assert X.reached + X.cut == G.j and X.reached == len(X.ids) == len(set(X.ids.tolist())) and X.sweeps <= X.words <= X.pairs
    return rounds


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(pc.WORKLOADS))
def test_root_0_gives_relax_poses_exactly(name):
    w, r = rc.workload(name)
    X, Y = rc.rerooted(w, 0, r), pc.relaxed(w, r)
    for a in ("ids", "pts", "head", "parent", "order", "new_parent"):
        assert np.array_equal(getattr(X, a), getattr(Y, a)), a
    assert np.array_equal(_bits(X.vcost), _bits(Y.vcost)) and np.array_equal(_bits(X.cstar), _bits(Y.cstar))
    assert (X.words, X.sweeps, X.pairs, X.cut) == (Y.words, Y.sweeps, Y.pairs, 0)
    # the start is the tree's own costs: every vertex hangs below vertex 0
    assert np.array_equal(_bits(X.start), _bits(Y.in_cost))


@pytest.mark.parametrize("name", ["E", "D", "A"])
def test_r2_0_gives_exactly_the_descendants_of_the_root(name):
    w, r = rc.workload(name)
    pts, head, parent, cost, j = pc.tree(w)
    for root in rc.roots_of(w):
        X = rc.rerooted(w, root, 0)
        below = []
        for k in range(j):  # a plain parent walk
            u = k
            while u != root and u != 0:
                u = int(parent[u])
            if u == root:
                below.append(k)
        depth = {root: 0}
        for k in below:  # (ascending: a parent comes before its child)
            if k != root:
                depth[k] = depth[int(parent[k])] + 1
        want = sorted(below, key=lambda k: (depth[k], 0 if k == root else 1, k))
        assert X.ids.tolist() == want and X.words == 0 and X.sweeps == 0
        vcost = np.zeros(len(want))
        new = {k: n for n, k in enumerate(want)}
        for n, k in enumerate(want[1:], 1):
            assert X.parent[n] == new[int(parent[k])]
            vcost[n] = vcost[X.parent[n]] + poserelaxref.word(pts, head, int(parent[k]), k, w.rho, w.nh)
        assert np.array_equal(_bits(X.vcost), _bits(vcost)) and np.array_equal(_bits(X.start[np.isfinite(X.start)]), _bits(X.cstar[np.isfinite(X.cstar)]))
        _held(w, 0, X)
    assert len(rc.rerooted(w, rc.midway(w), 0).ids) > 1  # (a root with something below it)


@pytest.mark.parametrize("name", ["E", "D", "A", "ties8", "duplicate", "long_edge", "blocked70", "chain", "sized1", "sized2", "sized63", "sized65"])
def test_dijkstra_and_jacobi_agree_the_certificate_is_clean_and_reached_is_reachable(name):
    w, r = rc.workload(name)
    for root in rc.roots_of(w):
        X = rc.rerooted(w, root, r)
        rounds = _held(w, r, X)
        print(name, dict(j=w.j, root=root, reached=X.reached, cut=X.cut, rounds=rounds, words=X.words, sweeps=X.sweeps, pairs=X.pairs))


# ------------------------------------------------------------------------------------------------ what each case is for
def test_a_radius_that_cuts_between_5_and_95_percent():
    w, r = rc.workload("D")
    X = rc.rerooted(w, w.j - 1, r)
    assert r > 0 and 0.05 * w.j < X.cut < 0.95 * w.j, (X.cut, w.j)
    old_root = int(np.flatnonzero(X.f_ids == 0)[0])
    assert not np.isfinite(X.cstar[old_root])  # (an RRTDubins tree heads away from its start: nothing leads back)


def test_a_case_that_cuts_none_and_reattaches_the_old_root_by_a_swept_word():
    w, r = rc.workload("E")
    X = rc.rerooted(w, w.j - 1, r)
    assert X.cut == 0 and X.reached == w.j
    old_root = int(np.flatnonzero(X.f_ids == 0)[0])
    assert old_root == 1 and X.f_parent[old_root] == -1 and np.isfinite(X.cstar[old_root])  # no old edge leads into it
    p = int(X.new_parent[old_root])
    assert p >= 0 and X.G.D2[p, old_root] < X.G.R and X.G.free(p, old_root)


def test_a_reached_vertex_keeps_an_old_parent_edge_longer_than_r():
    w, r = rc.workload("E")
    X = rc.rerooted(w, w.j - 1, r)
    G = X.G
    kept = [v for v in X.order.tolist() if X.f_parent[v] >= 0 and X.new_parent[v] == X.f_parent[v] and G.D2[X.f_parent[v], v] >= G.R]
    assert kept, "no reached vertex hangs on an old parent edge that is longer than r"


def test_a_duplicate_of_the_roots_pose_at_a_smaller_previous_number():
    w, r = rc.workload("duplicate")
    poseref.check_tie_duplicate(w, "first")
    X = rc.rerooted(w, w.dup, r)
    # the old root repeats the new root's pose and had the smaller number: in the dense input it is vertex 1, behind the root
    assert X.f_ids[0] == w.dup and X.f_ids[1] == 0 and tuple(X.f_pts[1]) == tuple(X.f_pts[0]) and X.f_head[1] == X.f_head[0]
    assert X.cstar[1] == 0.0 and X.new_parent[1] == 0 and X.G.into_len[1][0] == 0.0
    # every word from the duplicate is the root's, and the root has the smaller (cost, number): the duplicate is a parent only over an
    # old edge longer than the radius, where the root's equal word is no candidate
    on_dup = np.flatnonzero(X.new_parent == 1)
    assert np.all(X.G.D2[0, on_dup] >= X.G.R) and np.all(X.f_parent[on_dup] == 1)
    near = [v for v in range(2, X.G.j) if X.G.D2[0, v] < X.G.R and X.G.edge(0, v) and X.cstar[v] == X.G.into_len[v][0]]
    assert near and all(X.new_parent[v] == 0 for v in near)
    _held(w, r, X)


def test_a_root_inside_a_kept_view_and_one_that_is_not_alive_in_it():
    k = posekeepref.changed("A")
    w, r = k.w, pc.WORKLOADS["A"]
    alive = np.flatnonzero(k.alive)
    dead = np.flatnonzero(~k.alive)
    assert len(dead) and len(alive) > 2
    root = int(alive[-1])
    X = rc.rerooted(w, root, r, k.og8, True)
    assert X.ids[0] == root and set(X.ids.tolist()) <= set(alive.tolist()) and X.G.j == len(alive)
    _held(w, r, X, k.og8)
    with pytest.raises(ValueError, match="not alive"):
        rc.rerooted(w, int(dead[0]), r, k.og8, True)
    with pytest.raises(ValueError, match="outside"):
        poserootref.reroot(w.og8, *pc.tree(w), w.j, pc.R_of(r), w.rho, w.nh)


# ------------------------------------------------------------------------------------------------ binding and arguments, no device
NAMES = ("rrt_batch_reroot_poses", "rrt_batch_reroot_poses_ms", "rrt_batch_reroot_poses_stats", "rrt_plan_reroot_poses", "rrt_plan_reroot_poses_ms",
         "rrt_plan_reroot_poses_stats")


def test_the_header_declares_the_six_symbols_and_the_module_binds_them():
    hdr = open(os.path.join(ROOT, "include", "rrt_hip_moving.h")).read()
    assert '#include "rrt_hip_moving.h"' in open(os.path.join(ROOT, "include", "rrt_hip.h")).read()
    for s in NAMES:
        assert f"int {s}(" in hdr and s not in _ffi.SYMBOLS and s in moving._PROTOTYPES
    L = moving._lib()
    assert L is _ffi.lib()
    assert L.rrt_batch_reroot_poses.argtypes[2] is ctypes.c_int32 and L.rrt_batch_reroot_poses.argtypes[3] is ctypes.c_int64
    assert len(L.rrt_batch_reroot_poses.argtypes) == 9 and len(L.rrt_plan_reroot_poses.argtypes) == 8
    j0 = ctypes.c_int32(0)
    assert L.rrt_batch_reroot_poses(None, 0, 0, 576, None, 0, ctypes.byref(j0), None, ctypes.byref(j0)) == _ffi.RRT_E_ARG
    assert L.rrt_batch_reroot_poses_ms(None, None, 10) == _ffi.RRT_E_ARG and L.rrt_batch_reroot_poses_stats(None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_reroot_poses(None, 0, 576, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    assert L.rrt_plan_reroot_poses_ms(None, None, 10) == _ffi.RRT_E_ARG and L.rrt_plan_reroot_poses_stats(None, None) == _ffi.RRT_E_ARG


def _refused(key, fn, *args, **fmt):
    code, text = GOLDEN[key]
    assert code == "ValueError"
    with pytest.raises(ValueError) as e:
        fn(*args)
    assert str(e.value) == text.format(**fmt), str(e.value)


def test_the_module_refuses_with_the_golden_texts_before_any_device_call():
    og = np.zeros((32, 32), dtype=np.int64)
    for p in (amd.RRTStandard(og, 50, pbar=False), amd.RRTStar(og, 50, 8, pbar=False), amd.RRTStarInformed(og, 50, 8, 4, pbar=False)):
        _refused("straight_line_planner", moving.reroot_poses, p, 3, 8)
        assert p._ctx is None
    for p in (RRTDubins(og, 50, 4.0, pbar=False), RRTStarDubins(og, 50, 8, 4.0, pbar=False)):
        _refused("dubins_planner_reroot", p.reroot, 3)  # reroot keeps refusing a Dubins planner, with the text it had
        _refused("radius_negative", moving.reroot_poses, p, 3, -1)
        with pytest.raises(RuntimeError, match="reroot_poses: no tree on the device"):
            moving.reroot_poses(p, 3, 8)
        with pytest.raises(RuntimeError, match="reroot_poses: no tree on the device"):
            moving.reroot_poses(p, 3, 0)  # r = 0 is allowed
        assert p._ctx is None and p.last_relax is None
    _refused("no_radius", moving.reroot_poses, RRTDubins(og, 50, 4.0, pbar=False), 3)
    p = RRTStarDubins(og, 50, 8, 4.0, pbar=False)
    with pytest.raises(RuntimeError, match="reroot_poses: no tree on the device"):
        moving.reroot_poses(p, 3)  # r defaults to r_rewire
