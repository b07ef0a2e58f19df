"""Host restatement of the cost-to-come field (rrt_batch_cost_field, rrtplanner_amd.field.cost_field): the check of the cost_field tests.

The field of a window is goalref.connect over the free cells of the window, cell by cell, and -1 / inf for the blocked ones, written
into (w, h) arrays.  Nothing is shortened and nothing is shared between cells: no buckets, no bounds, no neighbour's winner."""
import numpy as np

import goalref
import keepref


def whole(og8):
    return (0, 0) + tuple(np.asarray(og8).shape)


def field(og8, pts, vcost, j, window=None):
    """(vertex int32 (w, h), cost float64 (w, h), tried int64 (w, h)) over window = (x0, y0, w, h), by default the whole grid; tried is
    goalref's count of lines walked for a free cell (j where no vertex sees it) and 0 for a blocked one"""
    og8 = np.asarray(og8)
    x0, y0, w, h = whole(og8) if window is None else window
    vertex = np.full((w, h), -1, dtype=np.int32)
    cost = np.full((w, h), np.inf, dtype=np.float64)
    tried = np.zeros((w, h), dtype=np.int64)
    free = np.argwhere(og8[x0:x0 + w, y0:y0 + h] == 0)
    if len(free):
        v, c, t = goalref.connect(og8, pts, vcost, j, free + np.array((x0, y0)))
        vertex[free[:, 0], free[:, 1]] = v
        cost[free[:, 0], free[:, 1]] = c
        tried[free[:, 0], free[:, 1]] = t
    return vertex, cost, tried


def kept_field(og8_new, pts, parent, vcost, j, window=None):
    """(alive, vertex, cost, tried) as keep_tree on og8_new and then cost_field return them: the field over keepref's view of the alive
    vertices, in the numbers of the tree the caller holds"""
    a, ids, p, c, _ = keepref.view(og8_new, pts, parent, vcost, j)
    v, cost, tried = field(og8_new, p, c, len(ids), window)
    if len(ids):
        v = np.where(v < 0, -1, ids[np.maximum(v, 0)]).astype(np.int32)
    return a, v, cost, tried


def same(got, want):
    """the device's (vertex, cost) against the restatement's: shapes, types, vertices, and the costs as raw bits"""
    (gv, gc), (wv, wc) = got, want[:2]
    assert gv.dtype == np.int32 and gc.dtype == np.float64 and gv.shape == gc.shape == wv.shape, (gv.dtype, gc.dtype, gv.shape, gc.shape, wv.shape)
    assert np.array_equal(gv, wv), ("vertex", np.argwhere(gv != wv)[:8].tolist())
    assert np.array_equal(gc.view(np.int64), wc.view(np.int64)), ("cost", np.argwhere(gc.view(np.int64) != wc.view(np.int64))[:8].tolist())


def cut(want, window, inner):
    """the part `inner` = (x0, y0, w, h) of a field `want` that was taken over `window`"""
    ax, ay = inner[0] - window[0], inner[1] - window[1]
    return tuple(a[ax:ax + inner[2], ay:ay + inner[3]] for a in want)
