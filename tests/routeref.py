"""Host restatement of the routes calls (rrt_batch_routes, RRT.routes_to): the check of the routes tests.

Per goal: goalref's decision (vertex, cost); the raw route root = 0, ..., vertex along the parent pointers, then the goal, as rows
(x, y, id) with id = -1 for the goal; with `shortcut` the greedy line-of-sight pass; the length as the f64 sum, left to right, of
np.sqrt(float64(d2)) over the emitted legs (d2 an integer below 2^25: numpy's root is the correctly rounded one, as the device's is).

Nothing here is shortened: from every anchor EVERY later row is tested with the oracle's literal line walk, from the anchor to the
row (the walk is not symmetric), and the largest free one -- or a + 1, which is taken untested -- is the next row."""
import numpy as np

import goalref
import oracle


def raw_route(pts, parent, vertex, goal):
    """(rows (k, 2) int64, ids int64[k]) of the route root .. vertex, goal"""
    ids = [int(vertex)]
    while ids[-1] != 0:
        assert len(ids) <= len(parent), "the parent pointers do not lead to vertex 0"
        ids.append(int(parent[ids[-1]]))
    ids.reverse()
    rows = np.concatenate([np.asarray(pts, dtype=np.int64)[ids], np.asarray(goal, dtype=np.int64).reshape(1, 2)])
    return rows, np.array(ids + [-1], dtype=np.int64)


def shortcut(og8, rows):
    """(indices kept, lines tested): the rows of the polyline `rows` that greedy shortcutting emits"""
    k, a, keep, tested = len(rows), 0, [0], 0
    while a < k - 1:
        free = [b for b in range(a + 1, k) if b == a + 1 or oracle.collisionfree(og8, rows[a], rows[b])[0]]
        tested += k - 1 - (a + 1)
        a = max(free)
        keep.append(a)
    return keep, tested


def length(rows):
    total = np.float64(0.0)
    for p, q in zip(rows[:-1], rows[1:]):
        d = np.asarray(q, dtype=np.int64) - np.asarray(p, dtype=np.int64)
        total = total + np.sqrt(np.float64(d[0] * d[0] + d[1] * d[1]))
    return float(total)


def polyline(og8, rows, ids, cut):
    """(rows, ids, length) of one raw route, shortcut if `cut`"""
    rows, ids = np.asarray(rows, dtype=np.int64).reshape(-1, 2), np.asarray(ids, dtype=np.int64)
    if cut:
        keep, _ = shortcut(og8, rows)
        rows, ids = rows[keep], ids[keep]
    return rows, ids, length(rows)


def routes(og8, pts, vcost, parent, j, goals, cut=False):
    """(vertex int32[M], cost float64[M], length float64[M], offsets int64[M + 1], xy int32[(rows, 2)], ids int32[rows]) as
    _ffi.Batch.routes returns them"""
    goals = np.asarray(goals).reshape(-1, 2)
    vertex, cost, _ = goalref.connect(og8, pts, vcost, j, goals)
    xy, ids, lens, offsets = [np.zeros((0, 2), dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [], [0]
    for g, v in zip(goals, vertex.tolist()):
        if v < 0:
            lens.append(np.inf)
        else:
            r, i, ln = polyline(og8, *raw_route(pts, parent, v, g), cut)
            xy.append(r)
            ids.append(i)
            lens.append(ln)
        offsets.append(offsets[-1] + (0 if v < 0 else len(xy[-1])))
    return (vertex, cost, np.array(lens, dtype=np.float64), np.array(offsets, dtype=np.int64), np.concatenate(xy).astype(np.int32),
            np.concatenate(ids).astype(np.int32))
