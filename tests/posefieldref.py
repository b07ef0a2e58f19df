"""Host restatement of the pose cost field (rrt_batch_pose_field, rrtplanner_amd.posefield): the check of the pose_field tests.

The literal form: for every free cell (x, y) of the window and every heading h in [0, nh), poseref.connect([(x, y, h)]) -- the oracle's
word and sweep over all j vertices in stable (cost, index) order.  Nothing is shared between cells or headings: no bound, no
neighbour, no bucket.  A blocked cell answers -1 / inf at every heading without a word.

  fixed heading H   the answers at H; the heading array holds H where a vertex connects and -1 where none does
  any heading       poseref.any_heading's rule over the nh answers of the cell: e = argmin(cost), the first among equals (the smallest
                    heading); (vertex[e], cost[e], e) if that one connects, else (-1, inf, -1)
  a kept view       posekeepref.connect_alive in place of poseref.connect: the alive vertices alone, on the new map, in the numbers of
                    the whole tree

A reference costs j * nh words per free cell, some 7 us each: posefieldcases.py keeps every one below about 1.5 million."""
import numpy as np

import posekeepref
import poseref


class Field:
    """vertex int32 (w, h, nh), cost float64 (w, h, nh), rank int64 (w, h, nh) (-1 where nothing connects, and for a kept view), free bool (w, h)"""


def field(og8, pts, head, vcost, j, rho, nh, window, alive=None):
    x0, y0, w, h = window
    f = Field()
    f.window, f.nh, f.j = tuple(window), nh, int(j if alive is None else np.count_nonzero(alive))
    f.vertex = np.full((w, h, nh), -1, dtype=np.int32)
    f.cost = np.full((w, h, nh), np.inf, dtype=np.float64)
    f.rank = np.full((w, h, nh), -1, dtype=np.int64)
    f.free = og8[x0:x0 + w, y0:y0 + h] == 0
    for cx in range(w):
        for cy in range(h):
            if not f.free[cx, cy]:
                continue
            goals = [(x0 + cx, y0 + cy, a) for a in range(nh)]
            if alive is None:
                f.vertex[cx, cy], f.cost[cx, cy], f.rank[cx, cy] = poseref.connect(og8, pts, head, vcost, j, goals, rho, nh)
            else:
                f.vertex[cx, cy], f.cost[cx, cy] = posekeepref.connect_alive(og8, alive, pts, head, vcost, goals, rho, nh)
    return f


def fixed(f, H):
    """(vertex int32 (w, h), cost float64 (w, h), heading int32 (w, h)) of the field at arrival heading H"""
    v = f.vertex[:, :, H].copy()
    return v, f.cost[:, :, H].copy(), np.where(v >= 0, H, -1).astype(np.int32)


def any_heading(f):
    """... at any arrival heading"""
    e = np.argmin(f.cost, axis=2)  # (the first among equal costs: the smallest heading)
    v = np.take_along_axis(f.vertex, e[:, :, None], axis=2)[:, :, 0]
    c = np.take_along_axis(f.cost, e[:, :, None], axis=2)[:, :, 0]
    return v.copy(), np.where(v >= 0, c, np.inf), np.where(v >= 0, e, -1).astype(np.int32)


def answer(f, heading):
    return any_heading(f) if heading < 0 else fixed(f, heading)


def cut(ans, window, inner):
    """the answer over `inner`, a window inside `window`, as the slice of the one over `window`"""
    ox, oy = inner[0] - window[0], inner[1] - window[1]
    return tuple(a[ox:ox + inner[2], oy:oy + inner[3]] for a in ans)


def same(got, want):
    """three arrays, equal entry for entry; costs as raw bits"""
    (gv, gc, gh), (wv, wc, wh) = got, want
    assert gv.dtype == np.int32 and gc.dtype == np.float64 and gh.dtype == np.int32 and gv.shape == gc.shape == gh.shape == wv.shape
    assert np.array_equal(gv, wv), np.argwhere(gv != wv)[:8]
    assert np.array_equal(gc.view(np.int64), np.ascontiguousarray(wc).view(np.int64)), np.argwhere(gc != wc)[:8]
    assert np.array_equal(gh, wh), np.argwhere(gh != wh)[:8]
