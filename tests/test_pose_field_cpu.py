"""CPU: the host restatement of the pose cost field (posefieldref.py) and the cases of the GPU tests (posefieldcases.py), held to what
they are for.  The device is compared with them in test_pose_field_gpu.py; here the restatement is checked against poseref cell by
cell, the header, the binding and the library are shown to agree, the windows are shown to get the runs they are meant to get, and every
case is shown to ask what it is meant to ask: obstacles, cells nothing reaches, several winners and headings, winners past cheaper
blocked candidates, exact ties between vertices and between headings, a view that lost vertices."""
import json
import os

import numpy as np
import pytest

import posefieldcases as pfc
import posefieldref
import poseref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rrtplanner_amd", "csrc")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_poseref_cell_by_cell():
    w, window, f = pfc.workload("E")
    x0, y0, ww, hh = window
    assert f.vertex.shape == f.cost.shape == f.rank.shape == (ww, hh, w.nh) and f.vertex.dtype == np.int32 and f.cost.dtype == np.float64
    anyv, anyc, anyh = posefieldref.any_heading(f)
    tree = (w.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j)
    free = np.argwhere(f.free)
    for cx, cy in free[np.random.default_rng(1).permutation(len(free))[:5]].tolist():
        cell = (x0 + cx, y0 + cy)
        v, c, h = poseref.any_heading(*tree, cell, w.rho, w.nh)
        assert (anyv[cx, cy], anyh[cx, cy]) == (v, h) and _bits(anyc[cx, cy]) == _bits(c)
        for H in pfc.headings_of(w.nh)[1:]:
            (v1,), (c1,), (r1,) = poseref.connect(*tree, [(cell[0], cell[1], H)], w.rho, w.nh)
            fv, fc, fh = posefieldref.fixed(f, H)
            assert (fv[cx, cy], f.rank[cx, cy, H]) == (v1, r1) and _bits(fc[cx, cy]) == _bits(c1) and fh[cx, cy] == (H if v1 >= 0 else -1)
    # a blocked cell: poseref itself answers -1 / inf, at every heading
    bx, by = np.argwhere(~f.free)[0].tolist()
    assert np.all(f.vertex[bx, by] == -1) and np.all(np.isinf(f.cost[bx, by])) and (anyv[bx, by], anyh[bx, by]) == (-1, -1)
    v, c, _ = poseref.connect(*tree, [(x0 + bx, y0 + by, 0)], w.rho, w.nh)
    assert (v[0], c[0]) == (-1, np.inf)
    # a window is the slice of the whole
    inner = (x0 + 2, y0 + 1, 3, 2)
    part = posefieldref.field(*tree, w.rho, w.nh, inner)
    for H in pfc.headings_of(w.nh):
        posefieldref.same(posefieldref.answer(part, H), posefieldref.cut(posefieldref.answer(f, H), window, inner))


# ------------------------------------------------------------------------------------------------ header, binding, library
def test_the_header_the_binding_and_the_library_agree():
    """include/rrt_hip_pose_field.h declares what rrtplanner_amd.posefield binds, and librrt_hip.so exports it (no call is made)"""
    import ctypes
    import re

    from rrtplanner_amd import _ffi, field, posefield

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rrt_hip_pose_field.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(posefield._PROTOTYPES) and len(declared) == 6
    assert not set(declared) & set(_ffi.SYMBOLS) and not set(declared) & set(field._PROTOTYPES)  # the recorded surfaces stay as they are
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert posefield._lib() is _ffi.lib()
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_field_refusals.json")))
    assert all(len(v) == 2 and (v[0] in (-1, -5, "ValueError")) and v[1].split(":")[0] in declared + ["pose_field"] for v in golden.values())


def test_the_planner_form_refuses_on_the_host():
    from rrtplanner_amd import posefield
    from rrtplanner_amd import rrt as amd
    from rrtplanner_amd.dubins import RRTStarDubins

    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_field_refusals.json")))
    og = np.zeros((32, 40), dtype=int)
    with pytest.raises(ValueError) as e:
        posefield.pose_field(amd.RRTStar(og, 50, 8, pbar=False))
    assert str(e.value) == golden["straight_class"][1] and "field.cost_field" in str(e.value)
    p = RRTStarDubins(og, 50, 8, 2.0, n_headings=16, pbar=False)
    for bad in ((0, 0, 33, 1), (0, 0, 0, 1), (-1, 0, 2, 2), (0, 39, 1, 2)):
        with pytest.raises(ValueError, match="inside"):
            posefield.pose_field(p, bad)
    with pytest.raises(ValueError, match="window"):
        posefield.pose_field(p, (0, 0, 1))
    for bad in (16, -2, 1.5, "north"):
        with pytest.raises(ValueError, match="heading"):
            posefield.pose_field(p, (0, 0, 2, 2), bad)
    with pytest.raises(RuntimeError, match="plan"):  # a good call before any plan(): the planner's own guard
        posefield.pose_field(p, (0, 0, 2, 2), 3)


# ------------------------------------------------------------------------------------------------ the runs of a window
def test_which_windows_get_runs_of_more_than_one_cell():
    """The host gives a wavefront clamp(cells / 4096, 1, 16) consecutive cells of a column.  Only from the second cell of a run on does a
    cell start from the winner before it and scan the buckets from that bound, so the GPU file needs windows on both sides: every small
    case runs with one cell a wavefront, the whole 96 x 100 grid with two, and the windows of the 256 x 256 map with 6, 15 and 16, with
    a last run of a column that is cut short in two of them."""
    text = open(os.path.join(CSRC, "rrt_tree_calls.hip")).read()
    assert "pv.run = (int32_t)std::clamp<int64_t>(m / POSE_FIELD_WAVES, 1, POSE_FIELD_RUN);" in text
    small = list(pfc.WINDOWS.values()) + pfc.edge_windows() + list(pfc.SIZED_WINDOWS) + [pfc.TIE_WINDOW, pfc.MIRROR_WINDOW, (0, 0, 24, 24), (0, 0, 64, 64)]
    assert all(pfc.run_of(win) == 1 for win in small)
    assert pfc.run_of((0, 0, 96, 100)) == 2 and [pfc.run_of(win) for win in pfc.WIDE_WINDOWS] == [16, 6, 15]
    assert pfc.run_of((0, 0, 4096, 4096)) == 16 and pfc.run_of((0, 0, 128, 64)) == 2 and pfc.run_of((0, 0, 127, 64)) == 1
    assert [win[3] % pfc.run_of(win) for win in pfc.WIDE_WINDOWS] == [0, 2, 10]
    w = pfc.wide()
    assert w.og8.shape == (256, 256) and w.j >= 200 and w.nh == 8
    og2, alive = pfc.wide_kept()
    assert 50 < alive.sum() < w.j - 50 and alive[0]
    for win in pfc.WIDE_WINDOWS:
        for tile in pfc.tiles(win):
            assert pfc.run_of(tile) == 1 and win[0] <= tile[0] and tile[0] + tile[2] <= win[0] + win[2] and win[1] <= tile[1] and tile[1] + tile[3] <= win[1] + win[3]
        assert sum(t[2] * t[3] for t in pfc.tiles(win)) == win[2] * win[3]
        for probe in pfc.wide_probes(w):
            assert win[0] <= probe[0] and probe[0] + probe[2] <= win[0] + win[2] and win[1] <= probe[1] and probe[1] + probe[3] <= win[1] + win[3]
    connected, differ = 0, 0
    for probe in pfc.wide_probes(w):
        f, g = pfc.reference("wide", w, probe), pfc.reference("wide kept", w, probe, alive=alive, og8=og2)
        connected += int((posefieldref.any_heading(f)[0] >= 0).sum())
        differ += int((f.vertex != g.vertex).sum())
        assert np.all(alive[g.vertex[g.vertex >= 0]])
    assert connected >= 100 and differ >= 1  # the tree answers on the probes, and its view answers otherwise on some of them


# ------------------------------------------------------------------------------------------------ the cases, held to their purpose
@pytest.mark.parametrize("name", pfc.CLUTTERED)
def test_a_cluttered_window_is_cluttered(name):
    w, window, f = pfc.workload(name)
    anyv, anyc, anyh = posefieldref.any_heading(f)
    connected = f.vertex >= 0
    assert (~f.free).sum() > 0                                    # blocked cells
    assert (f.free & (anyv < 0)).sum() > 0                        # free cells that nothing reaches, at any heading
    assert len(np.unique(anyv[anyv >= 0])) >= 4                   # distinct winning vertices
    assert len(np.unique(anyh[anyh >= 0])) >= 3                   # distinct winning headings
    assert 4 * (f.rank[connected] > 0).sum() >= connected.sum() > 0  # answers found past a cheaper blocked candidate
    assert np.hypot(window[0] + window[2] / 2 - w.xs[0], window[1] + window[3] / 2 - w.xs[1]) > 12  # away from the root
    assert f.free.sum() * w.nh * w.j <= 1_500_000


def test_every_workload_window_asks_something():
    for name in pfc.WINDOWS:
        w, window, f = pfc.workload(name)
        assert w.nh == {"A": 16, "B": 8, "E": 64, "G1": 1, "G256": 256}[name] and 100 <= w.j <= 820
        assert window[2] * window[3] <= 100 and f.free.sum() * w.nh * w.j <= 1_500_000
        anyv = posefieldref.any_heading(f)[0]
        assert (anyv >= 0).sum() >= 10 and (~f.free).sum() > 0, name
        for H in pfc.headings_of(w.nh)[1:]:
            assert (posefieldref.fixed(f, H)[0] >= 0).sum() >= 5, (name, H)


def test_the_small_map_and_the_edge_windows():
    w, window, f = pfc.small_map()
    anyv = posefieldref.any_heading(f)[0]
    assert w.og8.shape == (24, 24) and w.j >= 20 and (anyv >= 0).sum() > 200 and len(np.unique(anyv[anyv >= 0])) >= 4 and (~f.free).sum() > 30
    W, H = poseref.workload("B").og8.shape
    shapes = [win[2:] for win in pfc.edge_windows()]
    assert shapes == [(1, 1), (W, 1), (1, H), (1, H), (1, 1), (1, 1), (1, 1), (1, 1)] and pfc.edge_windows()[3][0] == W - 1
    for x0, y0, ww, hh in pfc.edge_windows():
        assert 0 <= x0 and 0 <= y0 and x0 + ww <= W and y0 + hh <= H


@pytest.mark.parametrize("j", pfc.SIZES)
def test_the_sized_trees_have_their_size(j):
    for k in (0, 1, 2):
        w, window, f = pfc.sized(j, k)
        assert w.j == j and f.free.all() and f.free.sum() * w.nh * w.j <= 1_500_000
        anyv, anyc, anyh = posefieldref.any_heading(f)
        if k == 0 and j >= 63:  # behind the screen the root's words are blocked: other vertices answer
            assert (anyv > 0).all() and (f.rank > 0).any()
        if k == 2:  # the root's own pose: cost 0.0, by a word of no length
            assert (anyv[0, 1], anyc[0, 1], anyh[0, 1]) == (0, 0.0, poseref.STRIDE_START[2]) and (anyv >= 0).all()
    assert pfc.SIZED_WINDOWS[0][0] + 3 <= 70 and pfc.SIZED_WINDOWS[1][0] >= 73  # on either side of the wall x in [70, 73)


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_the_duplicate_ties_with_the_root_and_never_wins(rho, nh):
    for star in (0, 1):
        w, window, f = pfc.tie_duplicate(rho, nh, star)
        poseref.check_tie_duplicate(w, "first")
        assert window[0] <= 44 < window[0] + window[2] and window[1] <= 47 < window[1] + window[3]
        assert not np.any(f.vertex == w.dup) and (f.vertex == 0).sum() >= 8
        assert np.all(f.rank[f.vertex == 0] == 0)  # the tie is the winning key: the duplicate is the very next candidate


@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_the_mirror_tie_goes_to_the_lower_index(rho, nh):
    for star in (0, 1):
        b, iL, iR, window, f = pfc.tie_mirror(rho, nh, star)
        poseref.check_tie_collinear(poseref.tie_collinear(rho, nh, star, 0)[0], b, iL, iR)
        gx, gy = 90 - window[0], 50 - window[1]
        assert f.vertex[gx, gy, 0] == iL < iR and f.rank[gx, gy, 0] >= 1 and _bits(f.cost[gx, gy, 0]) == _bits(b.c[0, iR])


def test_the_heading_tie_is_a_tie_bit_for_bit():
    """the search of posefieldcases.heading_tie finds a cell -- (19, 50), right behind the start, at rho 4 and 16 headings: headings 1
    and 15, mirror images of each other --; its two cheapest headings have equal bits and the any-heading answer is the smaller one"""
    found = pfc.heading_tie()
    assert found is not None
    w, window, f, (h0, h1) = found
    c = f.cost[0, 0]
    assert h0 < h1 and np.isfinite(c[h0]) and _bits(c[h0]) == _bits(c[h1]) and np.all(c >= c[h0])
    anyv, anyc, anyh = posefieldref.any_heading(f)
    assert anyh[0, 0] == h0 and anyv[0, 0] == f.vertex[0, 0, h0] and window[1] == poseref.TIE_START[1] and window[0] < poseref.TIE_START[0]


# ------------------------------------------------------------------------------------------------ a kept view
def test_the_kept_view_lost_vertices_and_keeps_its_numbers():
    k, window, f = pfc.kept()
    alive = k.alive
    anyv = posefieldref.any_heading(f)[0]
    winners = anyv[anyv >= 0]
    assert 0 < (~alive).sum() and alive[0] and len(winners) >= 10 and np.all(alive[f.vertex[f.vertex >= 0]])
    assert np.any((np.cumsum(alive) - 1)[winners] != winners)  # the caller's numbers, not the view's
    before = pfc.workload(pfc.KEPT)[2]
    assert not np.array_equal(before.vertex, f.vertex)  # the new map and the lost vertices change the field of this window
