"""CPU: the host restatement of the cost-to-come field (fieldref.py) and the cases of the GPU tests (fieldcases.py), held to what they
are for.  The device is compared with them in test_cost_field_gpu.py; here the restatement is checked against goalref cell by cell,
and every case is shown to ask what it is meant to ask: cells past a blocked first candidate, cells no vertex sees, deep candidates
with few distinct winners, an exact tie."""
import numpy as np
import pytest

import fieldcases
import fieldref
import goalref
import oracle


def _free(c, window):
    x0, y0, w, h = window
    return c["og8"][x0:x0 + w, y0:y0 + h] == 0


def test_the_restatement_is_goalref_cell_by_cell():
    c, window, (vertex, cost, tried) = fieldcases.planned("maze")
    assert vertex.shape == cost.shape == tried.shape == c["og8"].shape and vertex.dtype == np.int32 and cost.dtype == np.float64
    rng = np.random.default_rng(1)
    for x, y in np.argwhere(c["og8"] == 0)[rng.integers(0, int((c["og8"] == 0).sum()), size=40)].tolist():
        k, ck, t = goalref.connect_one(c["og8"], *fieldcases.tree(c), (x, y))
        assert (vertex[x, y], tried[x, y]) == (k, t) and np.float64(cost[x, y]).view(np.int64) == np.float64(ck).view(np.int64)
    # a window is the slice of the whole
    inner = (20, 31, 17, 40)
    part = fieldref.field(c["og8"], *fieldcases.tree(c), inner)
    for a, b in zip(part, fieldref.cut((vertex, cost, tried), window, inner)):
        assert np.array_equal(a, b)


def test_blocked_cells_answer_minus_one_and_inf():
    c, window, (vertex, cost, tried) = fieldcases.planned("maze")
    blocked = np.argwhere(c["og8"] != 0)
    assert len(blocked) > 100
    assert np.all(vertex[c["og8"] != 0] == -1) and np.all(np.isinf(cost[c["og8"] != 0])) and np.all(tried[c["og8"] != 0] == 0)
    for x, y in blocked[:: len(blocked) // 6][:6].tolist():  # goalref itself: every line ends on the cell
        k, ck, t = goalref.connect_one(c["og8"], *fieldcases.tree(c), (x, y))
        assert (k, ck, t) == (-1, np.inf, c["ro"].j)


def test_the_maze_has_unconnected_cells_and_blocked_first_candidates():
    c, window, (vertex, cost, tried) = fieldcases.planned("maze")
    free = _free(c, window)
    unconnected = free & (vertex < 0)
    assert c["ro"].j == 77
    assert unconnected.sum() >= 1000 and np.all(tried[unconnected] == c["ro"].j) and np.all(np.isinf(cost[unconnected]))
    assert (tried[free] > 1).sum() * 2 >= free.sum()


def test_the_square_connects_every_free_cell():
    c, window, (vertex, cost, tried) = fieldcases.planned("square")
    free = _free(c, window)
    assert np.all(vertex[free] >= 0) and np.all(np.isfinite(cost[free]))
    assert (tried[free] > 1).sum() * 4 >= free.sum()


def test_the_noise_window_is_deep_and_coherent():
    c, window, (vertex, cost, tried) = fieldcases.planned("noise")
    free = _free(c, window)
    assert window == fieldcases.NOISE_WINDOW and free.sum() > 2000
    assert np.all(tried[free] > 8) and tried[free].max() > 256
    assert len(np.unique(vertex[free & (vertex >= 0)])) < 100  # the coherence a kernel may exploit


@pytest.mark.parametrize("swapped", [False, True])
def test_the_tie_is_a_tie_bit_for_bit(swapped):
    c = fieldcases.tie(swapped)
    og8, (pts, vcost, j) = c["og8"], fieldcases.tree(c)
    g = np.array(fieldcases.TIE_CELL)
    assert not oracle.collisionfree(og8, pts[0], g)[0] and oracle.collisionfree(og8, pts[1], g)[0] and oracle.collisionfree(og8, pts[2], g)[0]
    key = [np.float64(vcost[k]) + np.sqrt(np.float64(((pts[k].astype(np.int64) - g) ** 2).sum())) for k in (1, 2)]
    assert key[0].view(np.int64) == key[1].view(np.int64) and key[0] < np.float64(vcost[0]) + 1000
    assert abs(int(pts[1][0]) - int(pts[2][0])) == 64  # (in different buckets for every edge up to 64 cells)
    k, ck, t = goalref.connect_one(og8, pts, vcost, j, g)
    assert (k, t) == (1, 2) and ck == key[0]  # the start is tried first and blocked; the lower index of the two wins


@pytest.mark.parametrize("k", fieldcases.SIZES)
def test_the_sized_trees_have_their_size_and_hidden_cells(k):
    c = fieldcases.sized(k)
    assert c["ro"].j == k and c["og8"].shape == fieldcases.SIZED_SHAPE
    W, H = fieldcases.SIZED_SHAPE
    for x0, y0, w, h in fieldcases.sized_windows():
        assert 0 <= x0 and 0 <= y0 and x0 + w <= W and y0 + h <= H
    if k >= 63:  # behind the wall the start sees little: other vertices answer there
        vertex, cost, tried = fieldcases.reference(("sized", k), c, (65, 0, 1, H))
        assert (vertex > 0).sum() >= 10 and (tried > 1).sum() >= 10


def test_the_header_the_binding_and_the_library_agree():
    """include/rrt_hip_field.h declares what rrtplanner_amd.field binds, and librrt_hip.so exports it (no call is made: no GPU here)"""
    import ctypes
    import os
    import re

    from rrtplanner_amd import _ffi, field

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "rrt_hip_field.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(rrt_[a-z0-9_]+)\s*\(", hdr)))
    assert declared == sorted(field._PROTOTYPES) and len(declared) == 6
    assert not set(declared) & set(_ffi.SYMBOLS)  # the recorded surface of _ffi stays as it is
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    assert field._lib() is _ffi.lib()
