"""Host restatement of reroot_poses (rrt_batch_reroot_poses, rrtplanner_amd.moving.reroot_poses): the check of the pose re-root tests,
in the manner of poserelaxref.py, whose edges, parent rule and numbering these are.

  input    the finished Dubins tree (pts, head, parent, cost; vertices [0, j), root 0), or with og8_view its alive vertices as
           posekeepref sees them, renumbered, with their heading bytes; a vertex `root` in the caller's numbers (with a view it must be
           alive: ValueError otherwise); the map og8; the threshold R >= 0;
  dense    the input with `root` moved to the front as number 0, the others in their order;
  edges    into v != 0: every u != v with d2(u, v) < R whose shortest word u -> v is finite and sweeps free on og8, united with the old
           parent edge, which is not swept again.  The new root has no edge into it, the old root no old parent edge (parent -1);
  start    0 for the root, the sums of the old edges' words from the root down for its descendants in the old tree, +inf elsewhere;
  costs    c[0] = 0, c[v] = min c[u] + len(u -> v) in f64, the least fixpoint.  Two forms: a heap Dijkstra from the root (its heap meets
           every start value again: the old edges are entered with exactly those sums) and a Jacobi iteration from the start;
           tests/test_pose_reroot_cpu.py asserts they agree bit for bit;
  cut      the vertices with c = +inf;
  parents  of the others by poserelaxref's rule over the final costs, the numbers by (depth, previous number), the costs summed again
           from the root down as vcost[parent] + word: the fixpoint's, bit for bit.

The result feeds posegrowref.grow as poserelaxref.relax's does."""
import heapq

import numpy as np

import keepref
import posegrowref
import posekeepref
import poserelaxref
from poserelaxref import word, words_into
from relaxref import d2_matrix


class Rerooted:
    pass


class Graph(poserelaxref.Graph):
    """poserelaxref.Graph over a dense input in which a vertex other than 0 may have no old parent (parent -1), and with R = 0"""

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
        self.plen = np.full(j, np.inf)
        self.plen[0] = 0.0
        self.kids = [[] for _ in range(j)]
        for v in range(1, j):
            p = int(self.parent[v])
            if p >= 0:
                self.plen[v] = word(self.pts, self.head, p, v, rho, nh)
                self.kids[p].append(v)
        self.pairs = int(sum(len(u) for u in self.into))
        self._free = {}


def front(in_ids, ipts, ihead, ipar, r):
    """the dense input with its vertex r moved to the front: (perm, ids, pts, head, parent); parent -1 for the new root and the old one"""
    j = len(in_ids)
    perm = np.array([r] + [k for k in range(j) if k != r], dtype=np.int64)
    new = np.full(j, -1, dtype=np.int64)
    new[perm] = np.arange(j)
    par = np.full(j, -1, dtype=np.int64)
    for n, k in enumerate(perm.tolist()):
        if k != r and k != 0:
            par[n] = new[int(ipar[k])]
    return perm, np.asarray(in_ids)[perm], np.asarray(ipts)[perm].copy(), np.asarray(ihead)[perm].copy(), par


def start_costs(G):
    """0 for the root, the sums of the old edges' words for what hangs below it, level by level, +inf elsewhere"""
    c = np.full(G.j, np.inf)
    c[0] = 0.0
    level = [0]
    while level:
        nxt = []
        for u in level:
            for v in G.kids[u]:
                c[v] = c[u] + G.plen[v]
                nxt.append(v)
        level = nxt
    return c


def dijkstra(G):
    """poserelaxref.dijkstra without its last line: a vertex that no edge reaches stays at +inf.  (costs, words, sweeps): every chord
    into an unreached head comes up, has its word evaluated, and every finite word into it is swept."""
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
    return c, words, sweeps


def jacobi(G, start):
    """(fixpoint costs, rounds that lowered a cost) from `start`: every round prices every vertex with the costs of the round before"""
    j = G.j
    c = np.array(start, dtype=np.float64)
    assert c[0] == 0.0
    rounds = 0
    while True:
        new = c.copy()
        for v in range(1, j):
            p = int(G.parent[v])
            b = c[v] if p < 0 else min(c[v], c[p] + G.plen[v])
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
    """poserelaxref.choose_parents over the reached vertices; -1 for the root and for what was not reached"""
    j = G.j
    new_parent = np.full(j, -1, dtype=np.int64)
    for v in range(1, j):
        if not np.isfinite(c[v]):
            continue
        p = int(G.parent[v])
        ok = [(float(c[u]), int(u)) for u, ln in zip(G.into[v].tolist(), G.into_len[v].tolist())
              if c[u] + ln == c[v] and (float(c[u]), int(u)) < (float(c[v]), v) and (u == p or G.free(u, v))]
        if p >= 0 and c[p] + G.plen[v] == c[v] and (float(c[p]), p) < (float(c[v]), v):
            ok.append((float(c[p]), p))
        assert ok, ("no candidate gives the vertex its cost", v)
        new_parent[v] = min(ok)[1]
    return new_parent


def renumber(pts, head, new_parent, cstar, rho, nh):
    """(order, pts, head, parent, vcost) of the reached vertices by (depth, previous number), the costs summed from the root down"""
    j = len(pts)
    reached = np.flatnonzero(np.isfinite(cstar))
    depth = keepref.depth(np.where(new_parent < 0, 0, new_parent), j)  # (what was not reached hangs on 0 here and is left out below)
    order = np.array(sorted(reached.tolist(), key=lambda k: (int(depth[k]), k)), dtype=np.int64)
    new = np.full(j, -1, dtype=np.int64)
    new[order] = np.arange(len(order))
    par = np.array([-1 if k == 0 else new[int(new_parent[k])] for k in order.tolist()], dtype=np.int64)
    assert order[0] == 0 and np.all(par[1:] >= 0) and np.all(par[1:] < np.arange(1, len(order)))
    p, h = np.asarray(pts, dtype=np.int64)[order], np.asarray(head, dtype=np.int64)[order]
    vcost = np.zeros(len(order))
    for k in range(1, len(order)):
        vcost[k] = vcost[par[k]] + word(p, h, int(par[k]), k, rho, nh)
    assert np.array_equal(vcost.view(np.int64), np.asarray(cstar)[order].view(np.int64)), "the costs from the root down are not the fixpoint's"
    return order, p.copy(), h.copy(), par, vcost


def reroot(og8, pts, head, parent, cost, j, root, R, rho, nh, og8_view=None):
    """The Dubins tree [0, j) re-rooted at its vertex `root` on the map og8 with the threshold R (og8_view: the map it was kept on).
    Returns a Rerooted: ids (the caller's number of each vertex of the result), pts, head, parent, vcost; and in the numbers of the
    root-first dense input: f_ids, f_pts, f_head, f_parent, G, start, cstar, new_parent, order; reached, cut; words, sweeps
    (Dijkstra's counts), pairs."""
    assert R >= 0
    if not 0 <= root < j:
        raise ValueError(f"root={root} outside [0, {j})")
    alive = None if og8_view is None else posekeepref.alive(og8_view, pts, head, parent, j, rho, nh)
    in_ids, ipts, ihead, icost, ipar = posegrowref.seed(pts, head, parent, cost, j, alive)
    at = np.flatnonzero(in_ids == root)
    if len(at) == 0:
        raise ValueError(f"root={root} is not alive in the kept view")
    perm, f_ids, fpts, fhead, fpar = front(in_ids, ipts, ihead, ipar, int(at[0]))
    G = Graph(og8, fpts, fhead, fpar, R, rho, nh)
    cstar, words, sweeps = dijkstra(G)
    new_parent = choose_parents(G, cstar)
    order, opts, ohead, opar, ovcost = renumber(fpts, fhead, new_parent, cstar, rho, nh)
    out = Rerooted()
    out.ids, out.pts, out.head, out.parent, out.vcost = f_ids[order], opts, ohead, opar, ovcost
    out.order, out.cstar, out.new_parent, out.G = order, cstar, new_parent, G
    out.f_ids, out.f_pts, out.f_head, out.f_parent, out.perm = f_ids, fpts, fhead, fpar, perm
    out.start = start_costs(G)
    out.reached, out.cut = len(order), G.j - len(order)
    out.words, out.sweeps, out.pairs = words, sweeps, G.pairs
    return out


def old_edges_of(X):
    """the old parent edges among the reached vertices, as (parent, child) pairs of the result's numbers: for poserelaxref.certify"""
    new = np.full(X.G.j, -1, dtype=np.int64)
    new[X.order] = np.arange(len(X.order))
    return {(int(new[int(X.f_parent[k])]), int(new[k])) for k in X.order.tolist() if X.f_parent[k] >= 0 and new[int(X.f_parent[k])] >= 0}
