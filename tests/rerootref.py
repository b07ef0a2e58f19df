"""Host restatement of reroot (rrt_batch_reroot, RRT.reroot): the check of the reroot tests.

  input    the finished tree (pts, parent; vertices [0, j), root 0), or with og8_view its alive vertices as keepref sees them;
  path     p_0 = r, p_1 = parent[r], ..., p_d = 0;
  parents  new_parent[p_{i+1}] = p_i, new_parent[r] = -1, every other vertex keeps its parent;
  edges    each of the d reversed edges is walked by oracle.collisionfree(og8, pts[new parent], pts[new child]) -- the oracle's
           literal line walk, which is not symmetric; the edges that were not reversed are not tested again;
  alive    every edge on the vertex's own walk along new_parent to r holds (and the vertex was in the input);
  numbers  the alive vertices sorted by (edges between the vertex and r, previous number);
  costs    cost[0] = 0, cost[k] = cost[parent[k]] + sqrt(float64(d2)) for k = 1, 2, ... in the new numbering: every parent is below
           its child, so each cost is the left-to-right f64 sum along the path from r -- the arithmetic of growref.grow's `cost`.

The result feeds growref.grow as growref.seed's does.  Nothing here is shortened: every vertex walks its own way to r."""
import numpy as np

import keepref
import oracle


class Rerooted:
    pass


def path_to_root(parent, j, r):
    """[r, parent[r], ..., 0]"""
    p = [int(r)]
    while p[-1] != 0:
        p.append(int(parent[p[-1]]))
        assert 0 <= p[-1] < j and len(p) <= j, "the parent pointers do not lead to vertex 0"
    return p


def reroot(og8, pts, parent, j, r, og8_view=None):
    """The tree [0, j) re-rooted at its vertex r on the map og8 (og8_view: the map it was kept on, None = no view; r must be alive).
    Returns a Rerooted: ids int64[j0] (the previous number of each vertex), pts (j0, 2), vcost f64[j0], parent int64[j0], and for the
    tests d, path, new_parent (previous numbering), reversed_ok {child: bool}, depth int64[j0]."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    r = int(r)
    assert 0 <= r < j
    inp = np.ones(j, dtype=bool) if og8_view is None else keepref.alive(og8_view, pts, parent, j)
    assert inp[r], "the new root is not alive in the view"
    path = path_to_root(parent, j, r)
    d = len(path) - 1
    new_parent = np.array([int(parent[k]) for k in range(j)], dtype=np.int64)
    for i in range(d):
        new_parent[path[i + 1]] = path[i]
    new_parent[r] = -1
    reversed_ok = {path[i + 1]: bool(oracle.collisionfree(og8, pts[path[i]], pts[path[i + 1]])[0]) for i in range(d)}
    depth = np.full(j, -1, dtype=np.int64)
    for k in range(j):
        if not inp[k]:
            continue
        u, steps, good = k, 0, True
        while good and u != r:
            good = reversed_ok.get(u, True)
            u = int(new_parent[u])
            steps += 1
            assert (not good) or (0 <= u < j and steps <= j and inp[u]), "the new parent pointers do not lead to the new root"
        if good:
            depth[k] = steps
    ids = np.array(sorted((k for k in range(j) if depth[k] >= 0), key=lambda k: (int(depth[k]), k)), dtype=np.int64)
    new = np.full(j, -1, dtype=np.int64)
    new[ids] = np.arange(len(ids))
    out = Rerooted()
    out.ids, out.d, out.path, out.new_parent, out.reversed_ok = ids, d, path, new_parent, reversed_ok
    out.pts = pts[ids].copy()
    out.parent = np.array([-1 if k == r else new[int(new_parent[k])] for k in ids.tolist()], dtype=np.int64)
    out.depth = depth[ids]
    assert ids[0] == r and np.all(out.parent[1:] >= 0) and np.all(out.parent[1:] < np.arange(1, len(ids)))
    out.vcost = np.zeros(len(ids))
    for k in range(1, len(ids)):
        dx = out.pts[out.parent[k]] - out.pts[k]
        out.vcost[k] = out.vcost[out.parent[k]] + np.sqrt(np.float64(int(dx[0]) * int(dx[0]) + int(dx[1]) * int(dx[1])))
    return out
