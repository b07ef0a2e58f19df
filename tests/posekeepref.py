"""Host restatement of keep_pose_tree (rrt_batch_keep_pose_tree, RRTDubins / RRTStarDubins .keep_pose_tree): the check of the
keep-pose-tree tests, and the maps those tests share.

Given the finished Dubins tree (pts, head, parent, vcost; vertices [0, j), root 0) and the new map og':
  edge_ok[0] = the root's cell is free;  edge_ok[k] = poseref.sweep_free(og', pose[parent[k]], pose[k], the length of
  oracle.dub_shortest(pose[parent[k]], pose[k])) for k > 0 -- the oracle's word and oracle.dub_sweep_cells, the arithmetic of
  include/rrt_dubins.h, which gcc and gfx950 evaluate bit for bit alike;  alive[k] = every edge_ok on the walk from k to the root.
connect_poses afterwards is poseref.connect, run on the alive vertices alone (in their original order, with their unchanged costs
and headings) against og', and mapped back to the original vertex numbers.

Nothing here is shortened: every vertex walks its own way to the root, and parent[k] < k is not assumed.  (oracle/dubins_ref.c has
no entry for a single edge's sweep, so this check shares the header with the kernel, as poseref does.)"""
import functools

import numpy as np

import oracle
import poseref


def edge_ok(og8, pts, head, parent, j, rho, nh):
    ok = np.zeros(j, dtype=bool)
    for k in range(j):
        if k == 0:
            ok[0] = og8[int(pts[0][0]), int(pts[0][1])] == 0
            continue
        p = int(parent[k])
        if not 0 <= p < j:
            continue
        length = oracle.dub_shortest(float(pts[p][0]), float(pts[p][1]), poseref.theta(head[p], nh), float(pts[k][0]), float(pts[k][1]),
                                     poseref.theta(head[k], nh), rho)[3]
        ok[k] = poseref.sweep_free(og8, (int(pts[p][0]), int(pts[p][1])), int(head[p]), (int(pts[k][0]), int(pts[k][1]), int(head[k])), rho, nh, length)
    return ok


def alive_of(ok, parent, j):
    """bool[j] from the edge flags: every vertex by its own walk to the root, as keepref.alive"""
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


def alive(og8, pts, head, parent, j, rho, nh):
    """bool[j]"""
    return alive_of(edge_ok(og8, pts, head, parent, j, rho, nh), parent, j)


def connect_alive(og8, a, pts, head, vcost, goals, rho, nh):
    """(vertex int32[M], cost float64[M]) of poseref.connect on the vertices with a[k] alone, in the original vertex numbers"""
    ids = np.flatnonzero(a)
    m = len(np.asarray(goals).reshape(-1, 3))
    if len(ids) == 0:
        return np.full(m, -1, dtype=np.int32), np.full(m, np.inf)
    v, cost, _ = poseref.connect(og8, np.asarray(pts)[ids], np.asarray(head)[ids], np.asarray(vcost, dtype=np.float64)[ids], len(ids), goals, rho, nh)
    return np.where(v < 0, -1, ids[np.maximum(v, 0)]).astype(np.int32), cost


def connect(og8, pts, head, parent, vcost, j, goals, rho, nh):
    """(alive, vertex int32[M], cost float64[M]) as keep_pose_tree and then connect_poses return them"""
    a = alive(og8, pts, head, parent, j, rho, nh)
    return (a,) + connect_alive(og8, a, pts, head, vcost, goals, rho, nh)


# ------------------------------------------------------------------------------------------------------------- the changed maps
def blocks_map(og8, root, count=6, size=8, seed=7, clear=16):
    """og8 plus `count` blocks of size x size: x = integers(0, W - size), then y = integers(0, H - size), of default_rng(seed); a block
    whose centre is within `clear` cells of the root in both coordinates is skipped"""
    W, H = og8.shape
    rng = np.random.default_rng(seed)
    out = og8.copy()
    done = 0
    while done < count:
        x = int(rng.integers(0, W - size))
        y = int(rng.integers(0, H - size))
        if abs(x + size // 2 - int(root[0])) <= clear and abs(y + size // 2 - int(root[1])) <= clear:
            continue
        out[x:x + size, y:y + size] = 1
        done += 1
    return out


class Kept:
    pass


def kept(w, og8):
    """what keep_pose_tree and then connect_poses(w.goals) answer for workload w (poseref) on the map og8"""
    k = Kept()
    k.w, k.og8 = w, np.ascontiguousarray(og8, dtype=np.uint8)
    ro = w.ro
    k.ok = edge_ok(k.og8, ro.pts, ro.head, ro.parent, w.j, w.rho, w.nh)
    k.alive = alive_of(k.ok, ro.parent, w.j)
    k.vertex, k.cost = connect_alive(k.og8, k.alive, ro.pts, ro.head, ro.vcost, w.goals, w.rho, w.nh)
    return k


@functools.lru_cache(maxsize=None)
def changed(name):
    """workload `name` of poseref on its map plus the six blocks (computed once per process and shared; nobody writes to it)"""
    w = poseref.workload(name)
    return kept(w, blocks_map(w.og8, w.xs))


def whole_tree_on(k):
    """(vertex, cost) of the WHOLE tree priced on the new map: what a connect_poses that ignored the view would answer"""
    w = k.w
    v, c, _ = poseref.connect(k.og8, w.ro.pts, w.ro.head, w.ro.vcost, w.j, w.goals, w.rho, w.nh)
    return v, c


@functools.lru_cache(maxsize=None)
def chain_cut():
    """poseref.tie_chain() with the cell (700, 12) occupied"""
    w = poseref.tie_chain()
    og8 = w.og8.copy()
    og8[700, 12] = 1
    return kept(w, og8)


STRIDE_KEEP_J = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
STRIDE_BLOCK = (slice(40, 50), slice(20, 34))  # in the tree's half of poseref._stride_map(), away from the start (30, 48)


@functools.lru_cache(maxsize=None)
def stride_cut(j, star):
    w = poseref.stride_tree(j, star)
    og8 = w.og8.copy()
    og8[STRIDE_BLOCK] = 1
    return kept(w, og8)


def root_blocked(w):
    og8 = w.og8.copy()
    og8[w.xs[0], w.xs[1]] = 1
    return kept(w, og8)
