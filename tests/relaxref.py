"""Host restatement of relax (rrt_batch_relax, RRT.relax): the check of the relax tests.

  input    the finished tree (pts, parent, cost; vertices [0, j), root 0), or with og8_view its alive vertices as keepref sees them,
           renumbered; the map og8; the threshold R = hostprep.radius_threshold(r);
  edges    E(v), v != 0: every u != v with d2(u, v) < R and oracle.collisionfree(og8, pts[u], pts[v]) -- the oracle's literal line walk
           from u to v, which is not symmetric --, united with {parent[v]}: the old parent edge is not walked again and may be longer
           than the radius;
  costs    c[0] = 0, c[v] = min over u in E(v) of c[u] + sqrt(float64(d2(u, v))).  Two forms: a heap Dijkstra from the root, and a
           Jacobi iteration from the input costs to its fixpoint; tests/test_relax_cpu.py asserts they agree bit for bit;
  parents  over the final costs: the u in E(v) with c[u] + d == c[v] (f64 ==) and (c[u], u) < (c[v], v), the smallest (c[u], u);
  numbers  by (edges between the vertex and the root, previous number), as rerootref numbers a re-rooted tree;
  costs    again, summed from the root down in the new numbering: they must be the fixpoint's, bit for bit.

The result feeds growref.grow as growref.seed's does.  certify() checks result arrays by rules of their own."""
import heapq

import numpy as np

import keepref
import oracle


class Relaxed:
    pass


def d2_matrix(pts):
    p = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    dx = p[:, None, 0] - p[None, :, 0]
    dy = p[:, None, 1] - p[None, :, 1]
    return dx * dx + dy * dy


def leg(D2, u, v):
    return np.sqrt(np.float64(int(D2[u, v])))


def candidate_edges(og8, pts, parent, R, backwards=False):
    """E as a list per vertex (ascending u, the old parent among them), and the d2 matrix.  backwards: the walks taken v -> u, which is
    NOT the rule (tests/test_relax_cpu.py shows that it gives other costs)."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    j = len(pts)
    D2 = d2_matrix(pts)
    E = [[] for _ in range(j)]
    for v in range(1, j):
        near = np.flatnonzero(D2[:, v] < R)
        ev = set()
        for u in near.tolist():
            if u != v and oracle.collisionfree(og8, pts[v] if backwards else pts[u], pts[u] if backwards else pts[v])[0]:
                ev.add(u)
        ev.add(int(parent[v]))
        E[v] = sorted(ev)
    return E, D2


def dijkstra(E, D2):
    j = len(E)
    out = [[] for _ in range(j)]
    for v in range(1, j):
        for u in E[v]:
            out[u].append(v)
    c = np.full(j, np.inf)
    c[0] = 0.0
    done = np.zeros(j, dtype=bool)
    heap = [(0.0, 0)]
    while heap:
        cu, u = heapq.heappop(heap)
        if done[u]:
            continue
        done[u] = True
        for v in out[u]:
            if v == 0:
                continue
            cand = np.float64(cu) + leg(D2, u, v)
            if cand < c[v]:
                c[v] = cand
                heapq.heappush(heap, (float(cand), v))
    return c


def _flat(E, D2):
    us = np.array([u for v in range(len(E)) for u in E[v]], dtype=np.int64)
    vs = np.array([v for v in range(len(E)) for _ in E[v]], dtype=np.int64)
    return us, vs, np.sqrt(D2[us, vs].astype(np.float64))


def jacobi(E, D2, cost):
    """(fixpoint costs, rounds that lowered a cost): every round prices every edge with the costs of the round before"""
    us, vs, d = _flat(E, D2)
    c = np.array(cost, dtype=np.float64)
    c[0] = 0.0
    rounds = 0
    while True:
        new = c.copy()
        if len(us):
            np.minimum.at(new, vs, c[us] + d)
        if np.array_equal(new, c):
            return c, rounds
        c = new
        rounds += 1
        assert rounds <= len(E), "Bellman-Ford needs fewer rounds than vertices"


def jacobi_rounds(og8, pts, parent, cost, j, R):
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)[:j]
    E, D2 = candidate_edges(og8, pts, np.asarray(parent)[:j], R)
    return jacobi(E, D2, np.asarray(cost, dtype=np.float64)[:j])[1]


def choose_parents(E, D2, c):
    j = len(E)
    new_parent = np.full(j, -1, dtype=np.int64)
    ties = 0
    for v in range(1, j):
        ok = [(float(c[u]), u) for u in E[v] if c[u] + leg(D2, u, v) == c[v] and (float(c[u]), u) < (float(c[v]), v)]
        assert ok, ("no candidate gives the vertex its cost", v)
        ties += len(ok) > 1
        new_parent[v] = min(ok)[1]
    return new_parent, ties


def renumber(pts, new_parent, cstar):
    """(ids, pts, parent, vcost) by (depth, previous number), the costs summed from the root down"""
    j = len(pts)
    depth = keepref.depth(np.where(new_parent < 0, 0, new_parent), j)
    ids = np.array(sorted(range(j), key=lambda k: (int(depth[k]), k)), dtype=np.int64)
    new = np.full(j, -1, dtype=np.int64)
    new[ids] = np.arange(j)
    par = np.array([-1 if k == 0 else new[int(new_parent[k])] for k in ids.tolist()], dtype=np.int64)
    assert ids[0] == 0 and np.all(par[1:] >= 0) and np.all(par[1:] < np.arange(1, j))
    p = np.asarray(pts, dtype=np.int64)[ids]
    vcost = np.zeros(j)
    for k in range(1, j):
        dx = p[par[k]] - p[k]
        vcost[k] = vcost[par[k]] + np.sqrt(np.float64(int(dx[0]) * int(dx[0]) + int(dx[1]) * int(dx[1])))
    assert np.array_equal(vcost.view(np.int64), np.asarray(cstar)[ids].view(np.int64)), "the costs from the root down are not the fixpoint's"
    return ids, p.copy(), par, vcost


def relax(og8, pts, parent, cost, j, R, og8_view=None):
    """The tree [0, j) relaxed on the map og8 with the threshold R (og8_view: the map it was kept on, None = no view).  Returns a
    Relaxed: ids int64[j0] (the previous number of each vertex, in the caller's numbering), pts (j0, 2), parent int64[j0], vcost
    f64[j0]; and before the renumbering, in the numbering of the dense input: cstar, new_parent; in_ids (the caller's number of each
    input vertex), in_parent, in_cost, E, D2, fell (vertices whose cost fell), ties (vertices with more than one qualifying parent)."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    assert R > 0
    if og8_view is None:
        in_ids = np.arange(j, dtype=np.int64)
        ipts, icost = pts[:j].copy(), np.asarray(cost[:j], dtype=np.float64).copy()
        ipar = np.asarray(parent[:j], dtype=np.int64).copy()
        ipar[0] = -1
    else:
        _, in_ids, ipts, icost, ipar = keepref.view(og8_view, pts, parent, cost, j)
        assert len(in_ids) >= 1
    E, D2 = candidate_edges(og8, ipts, ipar, R)
    cstar = dijkstra(E, D2)
    new_parent, ties = choose_parents(E, D2, cstar)
    ids, opts, opar, ovcost = renumber(ipts, new_parent, cstar)
    out = Relaxed()
    out.ids, out.pts, out.parent, out.vcost = in_ids[ids], opts, opar, ovcost
    out.order = ids
    out.cstar, out.new_parent, out.in_ids, out.in_pts, out.in_parent, out.in_cost, out.E, out.D2 = cstar, new_parent, in_ids, ipts, ipar, icost, E, D2
    out.fell = int((cstar[1:] < icost[1:]).sum())
    out.ties = ties
    return out


def old_edges_of(in_parent, order):
    """the input's parent edges (parent, child) in the numbering of the result: order[k] = the input number of result vertex k"""
    new = np.full(len(order), -1, dtype=np.int64)
    new[np.asarray(order)] = np.arange(len(order))
    return {(int(new[int(in_parent[k])]), int(new[k])) for k in range(1, len(order))}


def certify(og8, pts, parent, cost, R, old_edges):
    """An independent certificate over result arrays (any numbering with the root at 0): a list of what is wrong, empty when the arrays
    are the shortest-path tree over the tested edges within R and the edges `old_edges` ((parent, child) pairs of these numbers)."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    parent = np.asarray(parent, dtype=np.int64)
    cost = np.asarray(cost, dtype=np.float64)
    j = len(pts)
    bad = []
    if cost[0] != 0.0:
        bad.append(("root cost", 0))

    def d2(u, v):
        dx, dy = int(pts[u][0]) - int(pts[v][0]), int(pts[u][1]) - int(pts[v][1])
        return dx * dx + dy * dy

    for k in range(1, j):
        p = int(parent[k])
        if not 0 <= p < j:
            bad.append(("parent outside the tree", k))
            continue
        if p >= k:
            bad.append(("parent above child", k))
        if (cost[p] + np.sqrt(np.float64(d2(p, k)))).view(np.int64) != cost[k].view(np.int64):
            bad.append(("cost is not parent + edge", k))
        if (p, k) not in old_edges and not (d2(p, k) < R and oracle.collisionfree(og8, pts[p], pts[k])[0]):
            bad.append(("parent edge outside E", k))
    D2 = d2_matrix(pts)
    better = cost[:, None] + np.sqrt(D2.astype(np.float64)) < cost[None, :]  # [u, v]: the edge u -> v would lower v
    np.fill_diagonal(better, False)
    better[:, 0] = False
    old = np.zeros((j, j), dtype=bool)
    for u, v in old_edges:
        old[u, v] = True
    better &= (D2 < R) | old
    for v in np.flatnonzero(better.any(axis=0)).tolist():
        for u in np.flatnonzero(better[:, v]).tolist():
            if (u, v) in old_edges or (D2[u, v] < R and oracle.collisionfree(og8, pts[u], pts[v])[0]):
                bad.append(("an edge of E improves", v))
                break
    return bad
