"""Host restatement of grow (rrt_batch_grow, RRT.grow): the check of the grow tests.

  seed     the alive vertices of keepref.view on the new map, in their original order, parents renumbered -- or, without a view,
           the whole tree [0, j);
  sampled  the cells of seed vertices 1 .. j0-1 and nothing else (rrt.py:407-413 never puts xstart into the set);
  loop     m iterations of rrt.py:418-437 (alg 0) / :498-548 (alg 1, default cost, the reference's rewire, which changes nothing)
           over oracle.nearest, oracle.within, oracle.collisionfree and cost = vcost[v] + sqrt(float(d2)); the near set is walked in
           ascending index with strict <, as rrt.py:515-521 does; j starts at j0, the capacity rule is `j != n` with the query's n;
  goal     goalref's decision for xgoal; found: row j (and row n) is the goal; not found: j < n faults like rrt.py:318, else vgoal = 0.

Nothing here is shortened."""
import numpy as np

import goalref
import keepref
import oracle

ST_OK, ST_UNREACHABLE = 0, -2


class Grown:
    pass


def seed(pts, parent, vcost, j, og8_view=None):
    """(ids int64[j0], pts int64 (j0, 2), vcost f64[j0], parent int64[j0]); og8_view: the map the tree was kept on, None = no view"""
    if og8_view is None:
        par = np.asarray(parent[:j], dtype=np.int64).copy()
        par[0] = -1
        return np.arange(j, dtype=np.int64), np.asarray(pts[:j], dtype=np.int64).reshape(-1, 2).copy(), np.asarray(vcost[:j], dtype=np.float64).copy(), par
    _, ids, p, c, par = keepref.view(og8_view, pts, parent, vcost, j)
    return ids, p.copy(), c.copy(), par


def sampled_of(spts):
    """the `sampled` set after the seed: cells of vertices 1 .. j0-1"""
    return {(int(x), int(y)) for x, y in np.asarray(spts)[1:]}


def grow(og8, alg, n, xg, r2, spts, scost, spar, samples):
    """the m = len(samples) iterations and go2goal on the map og8, from the seed (spts, scost, spar) of a query of n samples"""
    j0, m = len(spts), len(samples)
    assert 1 <= j0 and j0 + m <= n
    g = Grown()
    g.n, g.j0 = n, j0
    g.pts = np.full((n + 1, 2), np.iinfo(np.int32).min, dtype=np.int64)
    g.vcost = np.full(n + 1, np.inf)
    g.parent = np.full(n + 1, -1, dtype=np.int64)
    g.pts[:j0], g.vcost[:j0], g.parent[:j0] = spts, scost, spar
    g.nearest_log = np.full(m, -1, dtype=np.int32)
    g.accept_log = np.zeros(m, dtype=np.uint8)
    g.jlog = np.zeros(m, dtype=np.int32)
    g.sum_j = g.sum_near = 0
    sampled = sampled_of(spts)
    j = j0
    for i in range(m):
        x = (int(samples[i][0]), int(samples[i][1]))
        g.jlog[i] = j
        g.sum_j += j
        vn = oracle.nearest(g.pts[:j], x)  # rrt.py:422
        g.nearest_log[i] = vn
        acc = oracle.collisionfree(og8, g.pts[vn], x)[0] and x not in sampled and j != n  # rrt.py:424-425
        g.accept_log[i] = acc
        if not acc:
            continue
        sampled.add(x)

        def cost(v):
            d = g.pts[v] - np.asarray(x, dtype=np.int64)
            return g.vcost[v] + np.sqrt(np.float64(int(d[0]) * int(d[0]) + int(d[1]) * int(d[1])))

        vbest, cbest = vn, cost(vn)
        if alg >= 1:
            near = oracle.within(g.pts[:j], x, r2)  # ascending index
            g.sum_near += len(near)
            for v in near.tolist():  # rrt.py:515-521
                cn = cost(v)
                if cn < cbest and oracle.collisionfree(og8, g.pts[v], x)[0]:
                    vbest, cbest = v, cn
        g.pts[j], g.vcost[j], g.parent[j] = x, cbest, vbest
        j += 1
    g.j = j
    v, c, _ = goalref.connect_one(og8, g.pts, g.vcost, j, xg)
    g.found, g.vgoal, g.status = int(v >= 0), 0, ST_OK
    if v >= 0:
        g.vgoal = j
        g.pts[j], g.vcost[j], g.parent[j] = xg, c, v
        g.pts[n], g.vcost[n] = xg, c
    elif j < n:
        g.status = ST_UNREACHABLE
    g.rows = n + 1 if g.found else n
    return g
