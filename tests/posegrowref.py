"""Host restatement of grow_poses (rrt_batch_grow_poses, RRTDubins / RRTStarDubins .grow_poses): the check of the grow-poses tests,
in the manner of growref.py.

  seed     the alive vertices of posekeepref.alive on the new map, in their original order, with their costs and headings, parents
           renumbered (the root keeps -1) -- or, without a view, the whole tree [0, j);
  sampled  the cells of seed vertices 1 .. j0-1 and nothing else: oracle/dubins_oracle.c:123,146,157 keys the set on the cell and never
           marks the start's, so the cell of a cut vertex can be drawn again, and so can the start's;
  loop     m iterations of oracle/dubins_oracle.c:128-215 on the map og8 with j starting at j0: nearest on (x, y), lowest index among
           equals; the word nearest -> sample (oracle.dub_shortest) and its sweep (oracle.dub_sweep_cells, the counting of
           dub_sweep_free); accept = free and not sampled and j != n with the query's own n; RRT* walks the ball in ascending index
           with strict <, sweeping only the entries below the best cost so far;
  goal     the go2goal decision for the query's own goal pose (poseref.connect_one); found: row j (and row n) is the goal; not found:
           j < n is ST_UNREACHABLE, else vgoal = 0 -- what growref.grow does.

Nothing here is shortened.  (The words and sweeps are those of include/rrt_dubins.h through the oracle, which gcc and gfx950 evaluate
bit for bit alike; the loop around them is written here, not called.)"""
import functools
import math

import numpy as np

import oracle
import posekeepref
import poseref
from rrtplanner_amd import hostprep

ST_OK, ST_UNREACHABLE = 0, -2


class Grown:
    pass


def seed(pts, head, parent, vcost, j, alive=None):
    """(ids int64[j0], pts int64 (j0, 2), head int64[j0], vcost f64[j0], parent int64[j0]); alive: bool[j] of the keep, None = no view"""
    pts = np.asarray(pts[:j], dtype=np.int64).reshape(-1, 2)
    head, vcost, parent = np.asarray(head[:j], dtype=np.int64), np.asarray(vcost[:j], dtype=np.float64), np.asarray(parent[:j], dtype=np.int64)
    ids = np.arange(j, dtype=np.int64) if alive is None else np.flatnonzero(np.asarray(alive[:j], dtype=bool)).astype(np.int64)
    rank = np.full(j, -1, dtype=np.int64)
    rank[ids] = np.arange(len(ids))
    par = np.full(len(ids), -1, dtype=np.int64)
    for k, v in enumerate(ids.tolist()):
        if v != 0:
            par[k] = rank[parent[v]]
            assert 0 <= par[k] < k, "an alive vertex hangs on an alive one of a lower number"
    return ids, pts[ids].copy(), head[ids].copy(), vcost[ids].copy(), par


def seed_on(og8, pts, head, parent, vcost, j, rho, nh):
    """the seed of a tree that was kept on og8 (posekeepref.alive)"""
    return seed(pts, head, parent, vcost, j, alive=posekeepref.alive(og8, pts, head, parent, j, rho, nh))


def sampled_of(spts):
    """the `sampled` set after the seed: cells of vertices 1 .. j0-1"""
    return {(int(x), int(y)) for x, y in np.asarray(spts)[1:]}


def sweep(og8, a, ha, b, hb, rho, nh, length):
    """(free, cells) of dub_sweep_free (oracle/dubins_oracle.c:69-85) for the word a -> b of that length"""
    if not math.isfinite(length):
        return False, 0
    cells = oracle.dub_sweep_cells(a[0], a[1], poseref.theta(ha, nh), b[0], b[1], poseref.theta(hb, nh), rho, cap=int(length / 0.5) + 16)
    W, H = og8.shape
    for k, (cx, cy) in enumerate(cells.tolist()):
        if cx < 0 or cx >= W or cy < 0 or cy >= H or og8[cx, cy] != 0:
            return False, k + 1
    return bool(og8[b[0], b[1]] == 0), len(cells) + 1


def grow(og8, star, n, xg, r2, rho, nh, spts, shead, scost, spar, samples):
    """the m = len(samples) iterations and go2goal on the map og8, from the seed (spts, shead, scost, spar) of a query of n samples;
    samples: (m, 3) rows (x, y, h); xg: the goal pose"""
    samples = np.asarray(samples, dtype=np.int64).reshape(-1, 3)
    j0, m = len(spts), len(samples)
    assert 1 <= j0 and j0 + m <= n
    g = Grown()
    g.n, g.j0 = n, j0
    g.pts = np.full((n + 1, 2), np.iinfo(np.int32).min, dtype=np.int64)
    g.head = np.zeros(n + 1, dtype=np.int64)
    g.vcost = np.full(n + 1, np.inf)
    g.parent = np.full(n + 1, -1, dtype=np.int64)
    g.pts[:j0], g.head[:j0], g.vcost[:j0], g.parent[:j0] = spts, shead, scost, spar
    g.nearest_log = np.full(m, -1, dtype=np.int32)
    g.accept_log = np.zeros(m, dtype=np.uint8)
    g.jlog = np.zeros(m, dtype=np.int32)
    g.sum_j = g.sum_near = g.sum_cells_nn = 0
    sampled = sampled_of(spts)
    j = j0

    def word(v, x, h):
        return oracle.dub_shortest(float(g.pts[v, 0]), float(g.pts[v, 1]), poseref.theta(g.head[v], nh), float(x[0]), float(x[1]), poseref.theta(h, nh), rho)[3]

    for i in range(m):
        x, h = (int(samples[i, 0]), int(samples[i, 1])), int(samples[i, 2])
        g.jlog[i] = j
        g.sum_j += j
        vn = oracle.nearest(g.pts[:j], x)  # dubins_oracle.c:132
        g.nearest_log[i] = vn
        ln = word(vn, x, h)
        free, cells = sweep(og8, g.pts[vn], g.head[vn], x, h, rho, nh, ln)
        g.sum_cells_nn += cells
        acc = free and x not in sampled and j != n  # dubins_oracle.c:146
        g.accept_log[i] = acc
        if not acc:
            continue
        sampled.add(x)
        vbest, cbest = vn, g.vcost[vn] + ln
        if star:
            near = oracle.within(g.pts[:j], x, r2)  # ascending index
            g.sum_near += len(near)
            for v in near.tolist():  # dubins_oracle.c:163-188
                lv = word(v, x, h)
                cn = g.vcost[v] + lv
                if cn < cbest and sweep(og8, g.pts[v], g.head[v], x, h, rho, nh, lv)[0]:
                    vbest, cbest = v, cn
        g.pts[j], g.head[j], g.vcost[j], g.parent[j] = x, h, cbest, vbest
        j += 1
    g.j = j
    xg = tuple(int(v) for v in xg)
    v, c, _, _ = poseref.connect_one(og8, g.pts, g.head, g.vcost, j, xg, rho, nh)
    g.found, g.vgoal, g.status = int(v >= 0), 0, ST_OK
    if v >= 0:
        g.vgoal = j
        g.pts[j], g.head[j], g.vcost[j], g.parent[j] = xg[:2], xg[2], c, v
        g.pts[n], g.head[n], g.vcost[n] = xg[:2], xg[2], c
    elif j < n:
        g.status = ST_UNREACHABLE
    g.rows = n + 1 if g.found else n
    return g


def grow_workload(w, og8, alive, samples, n=None):
    """grow for a poseref workload w kept on og8 (alive: bool[j], None: nothing kept, the whole tree on og8)"""
    ro = w.ro
    ids, sp, sh, sc, spar = seed(ro.pts, ro.head, ro.parent, ro.vcost, w.j, alive)
    g = grow(og8, w.star, w.n if n is None else n, w.xg, w.r2, w.rho, w.nh, sp, sh, sc, spar, samples)
    g.ids = ids
    return g


def accepted_stream(w, pad_cell, pads):
    """A stream that builds exactly the tree of workload w and leaves room to grow it: the poses of its vertices 1 .. j-1 -- the samples
    the oracle accepted, in order; the refused ones change nothing -- and then `pads` samples on the cell `pad_cell`, which every
    run refuses (an obstacle cell, or one that is in `sampled`).  Returns (samples (n, 2), headings (n,), n) with n = j - 1 + pads, so
    that `j != n` never binds on the way and the query has room for pads - 1 more samples."""
    ro, j = w.ro, w.j
    cells = np.concatenate([np.asarray(ro.pts[1:j], dtype=np.int64).reshape(-1, 2), np.tile(np.asarray(pad_cell, dtype=np.int64), (pads, 1))])
    heads = np.concatenate([np.asarray(ro.head[1:j], dtype=np.int64), np.zeros(pads, dtype=np.int64)])
    return cells, heads, j - 1 + pads


# The stream of the uncut grow of workload A by 600 samples that the GPU test also sends through oracle/dubins_ref.c's audit:
# default_rng(UNCUT_A_SEED) draws 600 free cells, then 600 headings.  The audit's policy (posecalls.assert_audit_clean) allows 3
# decisions of the ambiguous classes on a tree of this size, and how many a stream has is a property of the stream -- the ORACLE's own
# tree of the 2000 samples has 1 ambiguous accept with seed 32 and 3 with 34, but 4 with 31 and 33, one more than the policy allows
# for any tree.  test_grow_poses_cpu.py holds the oracle's tree of this stream to the policy, without a GPU.
UNCUT_A_SEED = 32

FILL_N, FILL_J = 60, 21


def fill_exactly():
    """An empty 64 x 64 map, turning radius 1: 20 accepted samples in the interior, then 40 refused ones (the first sample's cell
    again), n = 60.  The grow stream of 39 more interior cells fills the query exactly: j0 + m == n and every sample is accepted.  The
    goal pose sits in the corner (0, 0) heading out of it along the diagonal: a vehicle could only arrive from outside the grid, so no
    vertex connects, and what go2goal then says depends on j == n alone.  Returns (workload, grow samples (39, 3))."""
    og8 = np.zeros((64, 64), dtype=np.uint8)
    xs, xg = (32, 32, 0), (0, 0, 1)
    rng = np.random.default_rng(5)
    cells = np.array([(x, y) for x in range(8, 56) for y in range(8, 56) if (x, y) != xs[:2]])
    perm = cells[rng.permutation(len(cells))]
    hd = rng.integers(0, 8, len(cells))
    first = FILL_J - 1
    samples = np.concatenate([perm[:first], np.tile(perm[0], (FILL_N - first, 1))])
    heads = np.concatenate([hd[:first], np.zeros(FILL_N - first, dtype=np.int64)])
    w = poseref.made("fill exactly", og8, FILL_N, 1, 12, 1.0, 8, xs, xg, samples, heads, [xg])
    m = FILL_N - FILL_J
    return w, np.column_stack([perm[first:first + m], hd[first:first + m]])


def planted_stream(k, seed=77):
    """The stream of the cut workload k (posekeepref.Kept): m = vertices cut samples drawn as plan() draws them on the new map, with
    planted ones -- up to 8 cells of cut vertices that are free on the new map (a random stream almost never lands on one), the start's
    cell with a heading that the start pose reaches, and one obstacle cell -- at random rows.  Returns (samples (m, 3) int64, rows of the cut cells, row of the start's cell, row
    of the obstacle cell)."""
    w = k.w
    ro = w.ro
    cut = np.flatnonzero(~k.alive)
    alive_cells = {(int(x), int(y)) for x, y in ro.pts[:w.j][k.alive]}
    cut_free, seen = [], set()
    for v in cut.tolist():
        c = (int(ro.pts[v, 0]), int(ro.pts[v, 1]))
        if k.og8[c] == 0 and c not in alive_cells and c not in seen and c != tuple(w.xs[:2]):
            cut_free.append(c)
            seen.add(c)
    m = len(cut)
    rng = np.random.default_rng(seed)
    free = np.argwhere(k.og8 == 0)
    cells = hostprep.draw_free_samples(rng, free, m)
    heads = rng.integers(0, w.nh, m)
    s = np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), heads])
    ob = np.argwhere(k.og8 != 0)[0]
    special = cut_free[:8] + [tuple(w.xs[:2]), (int(ob[0]), int(ob[1]))]
    where = rng.choice(m, size=len(special), replace=False)
    for r, c in zip(where.tolist(), special):
        s[r, 0], s[r, 1] = c
    # the start's cell: its nearest vertex is the root (distance 0, lowest index), so the first heading, from the start's own on, whose
    # word from the start pose sweeps free on the new map is accepted (the start's own pose is a full circle unless its heading is 0)
    xs = tuple(w.xs[:2])
    for dh in range(w.nh):
        h = (w.xs[2] + dh) % w.nh
        ln = oracle.dub_shortest(float(xs[0]), float(xs[1]), poseref.theta(w.xs[2], w.nh), float(xs[0]), float(xs[1]), poseref.theta(h, w.nh), w.rho)[3]
        if sweep(k.og8, xs, w.xs[2], xs, h, w.rho, w.nh, ln)[0]:
            s[where[-2], 2] = h
            break
    return s, where[:-2], int(where[-2]), int(where[-1])


@functools.lru_cache(maxsize=None)
def planted(name):
    """(cut workload, its planted stream, rows of the cut cells, row of the start's cell, row of the obstacle cell, the restatement's grow)"""
    k = posekeepref.changed(name)
    s, rows, row_start, row_ob = planted_stream(k)
    return k, s, rows, row_start, row_ob, grow_workload(k.w, k.og8, k.alive, s)


def more_poses(w, og8, m, seed=31):
    """m pose samples drawn as plan() draws its n: the free cells first, then the headings"""
    rng = np.random.default_rng(seed)
    cells = hostprep.draw_free_samples(rng, np.argwhere(og8 == 0), m)
    return np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), rng.integers(0, w.nh, m)])
