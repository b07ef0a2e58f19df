"""Host restatement of relax_poses (rrt_batch_relax_poses, RRTDubins / RRTStarDubins .relax_poses): the check of the pose relax tests,
in the manner of relaxref.py.

  input    the finished Dubins tree (pts, head, parent, cost; vertices [0, j), root 0), or with og8_view its alive vertices as
           posekeepref sees them, renumbered, with their heading bytes; the map og8; the threshold R = hostprep.radius_threshold(r);
  edges    E(v), v != 0: every u != v with d2(u, v) < R whose shortest word from pose u to pose v (oracle.dub_shortest: the arithmetic
           of include/rrt_dubins.h, the same on gcc and gfx950) is finite and sweeps free on og8 (poseref.sweep_free: every sample
           inside the grid and on a free cell, then v's cell), united with {parent[v]}: the old parent edge is not swept again and
           may be longer than the radius;
  costs    c[0] = 0, c[v] = min over u in E(v) of c[u] + len(u -> v) in f64.  Two forms: a heap Dijkstra from the root, and a Jacobi
           iteration from the tree's own costs (c[parent] + word == c[v] bit for bit on every edge, so they are a valid start);
           tests/test_pose_relax_cpu.py asserts they agree bit for bit.  Both sweep an edge only when it would lower a cost: the
           sweeps are cached per edge, and Dijkstra counts the words and the sweeps that no method can do without;
  parents  over the final costs: the u in E(v) with c[u] + len == c[v] (f64 ==) and (c[u], u) < (c[v], v), the smallest (c[u], u);
  numbers  by (edges between the vertex and the root, previous number);
  costs    again, summed from the root down in the new numbering as vcost[parent] + word: the fixpoint's, bit for bit.

The result feeds posegrowref.grow as posegrowref.seed's does.  certify() checks result arrays by rules of their own."""
import ctypes
import functools
import heapq

import numpy as np

import keepref
import oracle
import posegrowref
import posekeepref
import poseref
from relaxref import d2_matrix, old_edges_of  # noqa: F401  (old_edges_of: for the callers of certify)


class Relaxed:
    pass


@functools.lru_cache(maxsize=None)
def _word(x0, y0, h0, x1, y1, h1, rho, nh):
    return float(oracle.dub_shortest(float(x0), float(y0), poseref.theta(h0, nh), float(x1), float(y1), poseref.theta(h1, nh), rho)[3])


def words_into(pts, head, us, v, rho, nh):
    """the lengths of the words from the poses `us` to pose v, float64[len(us)]: oracle.dub_shortest without its per-call arrays"""
    call = oracle._dub_lib().orc_dub_shortest
    out = (ctypes.c_double * 5)()
    x1, y1, t1 = float(pts[v][0]), float(pts[v][1]), poseref.theta(int(head[v]), nh)
    ls = np.empty(len(us))
    for k, u in enumerate(us):
        call(float(pts[u][0]), float(pts[u][1]), poseref.theta(int(head[u]), nh), x1, y1, t1, float(rho), out)
        ls[k] = out[3]
    return ls


def word(pts, head, u, v, rho, nh):
    """length of the shortest word from pose u to pose v; inf: none"""
    return _word(int(pts[u][0]), int(pts[u][1]), int(head[u]), int(pts[v][0]), int(pts[v][1]), int(head[v]), float(rho), int(nh))


def swept_free(og8, pts, head, u, v, rho, nh):
    a, b = (int(pts[u][0]), int(pts[u][1])), (int(pts[v][0]), int(pts[v][1]), int(head[v]))
    return bool(poseref.sweep_free(og8, a, int(head[u]), b, rho, nh, word(pts, head, u, v, rho, nh)))


class Graph:
    """The near pairs of a dense input with their words, and the sweeps on demand.  into[v]: the u != v with d2(u, v) < R, ascending,
    and into_len[v] the words u -> v beside them; out[u] / out_len[u]: the same pairs by their tail; plen[v]: the old parent edge."""

    def __init__(self, og8, pts, head, parent, R, rho, nh):
        self.og8, self.R, self.rho, self.nh = og8, int(R), float(rho), int(nh)
        self.pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
        self.head, self.parent = np.asarray(head, dtype=np.int64), np.asarray(parent, dtype=np.int64)
        j = self.j = len(self.pts)
        self.D2 = d2_matrix(self.pts)
        self.into, self.into_len = [np.zeros(0, dtype=np.int64)] * j, [np.zeros(0)] * j
        out, out_len = [[] for _ in range(j)], [[] for _ in range(j)]
        for v in range(1, j):
            us = np.flatnonzero(self.D2[:, v] < self.R)
            us = us[us != v]
            ls = words_into(self.pts, self.head, us.tolist(), v, rho, nh)
            self.into[v], self.into_len[v] = us, ls
            for u, ln in zip(us.tolist(), ls.tolist()):
                out[u].append(v)
                out_len[u].append(ln)
        self.out = [np.array(o, dtype=np.int64) for o in out]
        self.out_len = [np.array(o, dtype=np.float64) for o in out_len]
        self.plen = np.zeros(j)
        self.kids = [[] for _ in range(j)]
        for v in range(1, j):
            self.plen[v] = word(self.pts, self.head, int(self.parent[v]), v, rho, nh)
            self.kids[int(self.parent[v])].append(v)
        self.pairs = int(sum(len(u) for u in self.into))
        self._free = {}

    def free(self, u, v):
        key = (int(u), int(v))
        if key not in self._free:
            self._free[key] = swept_free(self.og8, self.pts, self.head, key[0], key[1], self.rho, self.nh)
        return self._free[key]

    def edge(self, u, v):
        """u -> v is in E(v)"""
        return int(self.parent[v]) == int(u) or (u != v and self.D2[u, v] < self.R and self.free(u, v))


def dijkstra(G):
    """(costs, words, sweeps) by a heap Dijkstra from the root that puts off every evaluation until the heap asks for it.  A settled
    tail u enters its old children with their exact cost (no sweep) and its other near heads v with the chord c[u] + sqrt(d2), a hair
    below (no word is shorter than its chord; the hair covers the rounding of a straight word).  A chord that comes up while its head
    is unsettled has its word evaluated and goes back in with c[u] + len; a word that comes up while its head is unsettled is swept,
    and a free one settles the head.  So a word is evaluated only where the chord could not rule the pair out against the final cost,
    and an edge swept only where its word is below the final cost (or meets it first): no method that decides the same costs does with
    fewer, in whatever order it runs.  The tests hold the device's counters to at least these."""
    j = G.j
    c = np.full(j, np.inf)
    done = np.zeros(j, dtype=bool)
    heap = []
    words = sweeps = 0
    OLD, WORD, CHORD = 0, 1, 2

    def settle(u, cu):
        c[u], done[u] = cu, True
        for v in G.kids[u]:
            heapq.heappush(heap, (float(np.float64(cu) + G.plen[v]), OLD, u, v))
        vs = G.out[u]
        if len(vs):
            keys = (np.float64(cu) + np.sqrt(G.D2[u, vs].astype(np.float64))) * (1.0 - 1e-12)
            for i in np.flatnonzero(~done[vs] & (G.parent[vs] != u)).tolist():
                heapq.heappush(heap, (float(keys[i]), CHORD, u, i))

    settle(0, 0.0)
    while heap:
        key, kind, u, x = heapq.heappop(heap)
        v = int(G.out[u][x]) if kind != OLD else x
        if done[v]:
            continue
        if kind == OLD:
            settle(v, key)
        elif kind == CHORD:
            words += 1
            cand = np.float64(c[u]) + G.out_len[u][x]
            if np.isfinite(cand):
                heapq.heappush(heap, (float(cand), WORD, u, x))
        else:
            sweeps += 1
            if G.free(u, v):
                settle(v, key)
    assert done.all()
    return c, words, sweeps


def jacobi(G, cost):
    """(fixpoint costs, rounds that lowered a cost): every round prices every vertex with the costs of the round before"""
    j = G.j
    c = np.array(cost, dtype=np.float64)
    c[0] = 0.0
    rounds = 0
    while True:
        new = c.copy()
        for v in range(1, j):
            b = min(c[v], c[int(G.parent[v])] + G.plen[v])
            us = G.into[v]
            if len(us):
                cand = c[us] + G.into_len[v]
                idx = np.flatnonzero(cand < b)
                for i in idx[np.argsort(cand[idx], kind="stable")].tolist():
                    if G.free(int(us[i]), v):
                        b = cand[i]
                        break
            new[v] = b
        if np.array_equal(new, c):
            return c, rounds
        c = new
        rounds += 1
        assert rounds <= j, "Bellman-Ford needs fewer rounds than vertices"


def choose_parents(G, c):
    j = G.j
    new_parent = np.full(j, -1, dtype=np.int64)
    ties = 0
    for v in range(1, j):
        us, ls = G.into[v], G.into_len[v]
        p = int(G.parent[v])
        ok = [(float(c[u]), int(u)) for u, ln in zip(us.tolist(), ls.tolist())
              if c[u] + ln == c[v] and (float(c[u]), int(u)) < (float(c[v]), v) and (u == p or G.free(u, v))]
        if c[p] + G.plen[v] == c[v] and (float(c[p]), p) < (float(c[v]), v):
            ok.append((float(c[p]), p))
        ok = sorted(set(ok))
        assert ok, ("no candidate gives the vertex its cost", v)
        ties += len(ok) > 1
        new_parent[v] = ok[0][1]
    return new_parent, ties


def renumber(pts, head, new_parent, cstar, rho, nh):
    """(ids, pts, head, parent, vcost) by (depth, previous number), the costs summed from the root down"""
    j = len(pts)
    depth = keepref.depth(np.where(new_parent < 0, 0, new_parent), j)
    ids = np.array(sorted(range(j), key=lambda k: (int(depth[k]), k)), dtype=np.int64)
    new = np.full(j, -1, dtype=np.int64)
    new[ids] = np.arange(j)
    par = np.array([-1 if k == 0 else new[int(new_parent[k])] for k in ids.tolist()], dtype=np.int64)
    assert ids[0] == 0 and np.all(par[1:] >= 0) and np.all(par[1:] < np.arange(1, j))
    p, h = np.asarray(pts, dtype=np.int64)[ids], np.asarray(head, dtype=np.int64)[ids]
    vcost = np.zeros(j)
    for k in range(1, j):
        vcost[k] = vcost[par[k]] + word(p, h, int(par[k]), k, rho, nh)
    assert np.array_equal(vcost.view(np.int64), np.asarray(cstar)[ids].view(np.int64)), "the costs from the root down are not the fixpoint's"
    return ids, p.copy(), h.copy(), par, vcost


def relax(og8, pts, head, parent, cost, j, R, rho, nh, og8_view=None):
    """The Dubins tree [0, j) relaxed on the map og8 with the threshold R (og8_view: the map it was kept on, None = no view).  Returns
    a Relaxed: ids int64[j0] (the previous number of each vertex, in the caller's numbering), pts (j0, 2), head, parent, vcost; and
    before the renumbering, in the numbering of the dense input: cstar, new_parent, order; in_ids, in_pts, in_head, in_parent,
    in_cost, G (the Graph); fell, ties; words, sweeps (Dijkstra's counts), pairs (near pairs)."""
    assert R > 0
    alive = None if og8_view is None else posekeepref.alive(og8_view, pts, head, parent, j, rho, nh)
    in_ids, ipts, ihead, icost, ipar = posegrowref.seed(pts, head, parent, cost, j, alive)
    assert len(in_ids) >= 1
    G = Graph(og8, ipts, ihead, ipar, R, rho, nh)
    cstar, words, sweeps = dijkstra(G)
    new_parent, ties = choose_parents(G, cstar)
    ids, opts, ohead, opar, ovcost = renumber(ipts, ihead, new_parent, cstar, rho, nh)
    out = Relaxed()
    out.ids, out.pts, out.head, out.parent, out.vcost = in_ids[ids], opts, ohead, opar, ovcost
    out.order = ids
    out.cstar, out.new_parent, out.in_ids, out.in_pts, out.in_head, out.in_parent, out.in_cost, out.G = cstar, new_parent, in_ids, ipts, ihead, ipar, icost, G
    out.fell = int((cstar[1:] < icost[1:]).sum())
    out.ties, out.words, out.sweeps, out.pairs = ties, words, sweeps, G.pairs
    return out


def certify(og8, pts, head, parent, cost, R, rho, nh, old_edges, prev=None):
    """An independent certificate over result arrays (any numbering with the root at 0): a list of what is wrong, empty when the arrays
    are the shortest-path tree over the swept edges within R and the edges `old_edges` ((parent, child) pairs of these numbers).
    prev: the number each vertex had in the input; with it the parent rule is held too (the smallest (cost, previous number))."""
    pts = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    head = np.asarray(head, dtype=np.int64)
    parent = np.asarray(parent, dtype=np.int64)
    cost = np.asarray(cost, dtype=np.float64)
    j = len(pts)
    bad = []
    if cost[0] != 0.0:
        bad.append(("root cost", 0))
    D2 = d2_matrix(pts)
    swept = {}

    def in_e(u, v):
        if (u, v) in old_edges:
            return True
        if (u, v) not in swept:
            swept[(u, v)] = bool(D2[u, v] < R) and swept_free(og8, pts, head, u, v, rho, nh)
        return swept[(u, v)]

    for k in range(1, j):
        p = int(parent[k])
        if not 0 <= p < j:
            bad.append(("parent outside the tree", k))
            continue
        if p >= k:
            bad.append(("parent above child", k))
        if (cost[p] + word(pts, head, p, k, rho, nh)).view(np.int64) != cost[k].view(np.int64):
            bad.append(("cost is not parent + edge", k))
        if not in_e(p, k):
            bad.append(("parent edge outside E", k))
    old_into = {}
    for u, v in old_edges:
        old_into.setdefault(v, []).append(u)
    for v in range(1, j):
        us = set(np.flatnonzero(D2[:, v] < R).tolist()) | set(old_into.get(v, []))
        us.discard(v)
        us = sorted(us)
        p = int(parent[v])
        for u, ln in zip(us, words_into(pts, head, us, v, rho, nh).tolist()):
            cand = cost[u] + ln
            if cand < cost[v] and in_e(u, v):
                bad.append(("an edge of E improves", v))
                break
            if prev is not None and 0 <= p < j and u != p and cand == cost[v] and (cost[u], int(prev[u])) < (cost[p], int(prev[p])) and in_e(u, v):
                bad.append(("parent is not the smallest (cost, previous number)", v))
                break
    return bad
