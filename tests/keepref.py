"""Host restatement of keep_tree (rrt_batch_keep_tree, RRT.keep_tree): the check of the keep-tree tests.

Given the finished tree (pts, parent, vcost; vertices [0, j), root 0) and the new map og':
  edge_ok[0] = the root's cell is free;  edge_ok[k] = oracle.collisionfree(og', pts[parent[k]], pts[k]) for k > 0 -- the oracle's
  literal line walk, from the parent to the child;  alive[k] = every edge_ok on the walk from k to the root.
The answers of the goals and routes calls afterwards are goalref's / routeref's, run on the alive vertices alone (in their original
order, with their unchanged costs and their parents renumbered) against og', and mapped back to the original vertex numbers.

Nothing here is shortened: every vertex walks its own way to the root, and parent[k] < k is not assumed."""
import numpy as np

import goalref
import oracle
import routeref


def edge_ok(og8, pts, parent, j):
    ok = np.zeros(j, dtype=bool)
    for k in range(j):
        if k == 0:
            ok[0] = og8[int(pts[0][0]), int(pts[0][1])] == 0
        else:
            ok[k] = oracle.collisionfree(og8, pts[int(parent[k])], pts[k])[0]
    return ok


def alive(og8, pts, parent, j):
    """bool[j]"""
    ok = edge_ok(og8, pts, parent, j)
    out = np.zeros(j, dtype=bool)
    for k in range(j):
        u, steps, good = k, 0, bool(ok[k])
        while good and u != 0:
            u = int(parent[u])
            steps += 1
            assert 0 <= u < j and steps <= j, "the parent pointers do not lead to vertex 0"
            good = bool(ok[u])
        out[k] = good
    return out


def depth(parent, j):
    """int[j]: edges between a vertex and the root"""
    out = np.zeros(j, dtype=np.int64)
    for k in range(j):
        u = k
        while u != 0:
            u = int(parent[u])
            out[k] += 1
            assert out[k] <= j
    return out


def view(og8, pts, parent, vcost, j):
    """(alive bool[j], ids int64[n_alive], pts, vcost, parent of the alive vertices alone, the parents renumbered; the root's -1)"""
    a = alive(og8, pts, parent, j)
    ids = np.flatnonzero(a)
    new = np.full(j, -1, dtype=np.int64)
    new[ids] = np.arange(len(ids))
    par = np.array([-1 if k == 0 else new[int(parent[k])] for k in ids.tolist()], dtype=np.int64)
    assert np.all(par[1:] >= 0)  # every ancestor of an alive vertex is alive
    return a, ids, np.asarray(pts, dtype=np.int64)[ids].reshape(-1, 2), np.asarray(vcost, dtype=np.float64)[ids], par


def connect(og8, pts, parent, vcost, j, goals):
    """(alive, vertex int32[M], cost float64[M]) as keep_tree and then connect_goals return them"""
    a, ids, p, c, _ = view(og8, pts, parent, vcost, j)
    v, cost, _ = goalref.connect(og8, p, c, len(ids), goals)
    if len(ids) == 0:
        return a, v, cost  # (all -1 / inf)
    return a, np.where(v < 0, -1, ids[np.maximum(v, 0)]).astype(np.int32), cost


def routes(og8, pts, parent, vcost, j, goals, cut=False):
    """(alive, (vertex, cost, length, offsets, xy, ids)) as keep_tree and then _ffi.Batch.routes return them"""
    a, ids, p, c, par = view(og8, pts, parent, vcost, j)
    if len(ids) == 0:
        m = len(np.asarray(goals).reshape(-1, 2))
        return a, (np.full(m, -1, dtype=np.int32), np.full(m, np.inf), np.full(m, np.inf), np.zeros(m + 1, dtype=np.int64),
                   np.zeros((0, 2), dtype=np.int32), np.zeros(0, dtype=np.int32))
    v, cost, length, offsets, xy, rid = routeref.routes(og8, p, c, par, len(ids), goals, cut=cut)
    return a, (np.where(v < 0, -1, ids[np.maximum(v, 0)]).astype(np.int32), cost, length, offsets, xy,
               np.where(rid < 0, -1, ids[np.maximum(rid, 0)]).astype(np.int32))
