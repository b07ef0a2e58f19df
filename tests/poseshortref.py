"""Host restatement of rrt_batch_pose_shortcuts (Batch.pose_routes(shortcut=True), RRTDubins / RRTStarDubins
.routes_to_poses(shortcut=True)): the check of the pose-shortcut tests, and the ring workloads those tests share.

It starts from the raw rows of poseroutesref.routes.  Per connected goal, over its raw route P[0..k): from the anchor a = 0 the next kept
row is the LARGEST b in (a, k-1] with b == a + 1 (never tested) or for which poseref.sweep_free says that the oracle's shortest word
(oracle.dub_shortest) from pose P[a] to pose P[b], swept from P[a] on the ACTIVE map, is free; on from a = b until a == k - 1.  The
candidates are tried from the far end down, one by one, and every trial is recorded (`anchors`), so that the CPU tests can say what a
workload exercises.  Length and points are rebuilt with poseroutesref.leg over the kept rows: a Routes, which poseroutesref.same
compares."""
import functools
import math

import numpy as np

import oracle
import poseref
import poseroutesref as prr


def word_free(og8, a, b, rho, nh, cache=None):
    """is the shortest word from pose a to pose b = (x, y, heading index), swept from a on og8, free"""
    key = (a, b)
    if cache is not None and key in cache:
        return cache[key]
    length = oracle.dub_shortest(float(a[0]), float(a[1]), poseref.theta(a[2], nh), float(b[0]), float(b[1]), poseref.theta(b[2], nh), float(rho))[3]
    free = bool(poseref.sweep_free(og8, (a[0], a[1]), a[2], b, rho, nh, length))
    if cache is not None:
        cache[key] = free
    return free


def greedy(poses, og8, rho, nh, cache=None):
    """(kept row numbers, anchors) of one raw route; anchors: per anchor (a, b, candidates that were blocked before b was taken,
    candidates there were), b == a + 1 taken untested"""
    k = len(poses)
    kept, anchors = [0], []
    a = 0
    while a < k - 1:
        b, blocked = a + 1, 0
        for c in range(k - 1, a + 1, -1):
            if word_free(og8, poses[a], poses[c], rho, nh, cache):
                b = c
                break
            blocked += 1
        anchors.append((a, b, blocked, k - 2 - a))
        kept.append(b)
        a = b
    return kept, anchors


def shorten(raw, og8, rho, nh, shortcut=True):
    """the Routes of the shortcut call from the raw Routes `raw` (poseroutesref.routes) on the active map og8.  Besides the arrays:
    raw (the Routes it started from), kept_rows[g] (row numbers within the raw route of goal g) and anchors[g] (see greedy)."""
    if not shortcut:
        return raw
    m = len(raw.vertex)
    r = prr.Routes()
    r.raw, r.vertex, r.cost = raw, raw.vertex, raw.cost
    r.length = np.full(m, np.inf)
    r.offsets, r.point_offsets = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    rows, ids, chunks, spans = [], [], [], []
    r.kept_rows, r.anchors = [], []
    free, legs = {}, {}
    npoints = 0
    for g in range(m):
        kept, anchors = [], []
        if raw.vertex[g] >= 0:
            at = int(raw.offsets[g])
            poses = [tuple(int(x) for x in p) for p in raw.route(g)]
            kept, anchors = greedy(poses, og8, rho, nh, free)
            total = 0.0
            for ia, ib in zip(kept[:-1], kept[1:]):
                a, b = poses[ia], poses[ib]
                if (a, b) not in legs:
                    legs[(a, b)] = prr.leg(a, b, rho, nh)
                length, p = legs[(a, b)]
                total = total + length
                spans.append((npoints, len(p)))
                chunks.append(p)
                npoints += len(p)
            spans.append((npoints, -1))
            chunks.append(np.array([[float(poses[-1][0]), float(poses[-1][1])]]))
            npoints += 1
            r.length[g] = total
            rows += [poses[i] for i in kept]
            ids += [int(raw.ids[at + i]) for i in kept]
        r.kept_rows.append(kept)
        r.anchors.append(anchors)
        r.offsets[g + 1] = len(rows)
        r.point_offsets[g + 1] = npoints
    r.rows = np.array(rows, dtype=np.int32).reshape(-1, 3)
    r.ids = np.array(ids, dtype=np.int32)
    r.points = np.concatenate(chunks) if chunks else np.zeros((0, 2))
    r.leg_spans = spans
    return r


def routes(pts, head, parent, j, goals, vertex, cost, rho, nh, og8, shortcut=True):
    """what Batch.pose_routes(points=True, shortcut=shortcut) returns for these goals on the active map og8, as a Routes"""
    return shorten(prr.routes(pts, head, parent, j, goals, vertex, cost, rho, nh), og8, rho, nh, shortcut)


def of_case(c):
    """the shortened routes of a poseroutesref Case (case, kept_case, made_case, the chains), computed once and kept on it"""
    if "_pose_shortcuts" not in c.__dict__:
        c._pose_shortcuts = shorten(c.routes, c.og8, c.w.rho, c.w.nh)
    return c._pose_shortcuts


def counts(r):
    """(connected routes, routes shortened, anchors that took a tested candidate after a farther one was blocked, anchors that found
    every candidate blocked, the most blocked candidates in front of a tested winner)"""
    connected = int((r.vertex >= 0).sum())
    shortened = sum(1 for g, kept in enumerate(r.kept_rows) if kept and len(kept) < int(r.raw.offsets[g + 1] - r.raw.offsets[g]))
    flat = [x for anchors in r.anchors for x in anchors]
    past = sum(1 for a, b, blocked, cands in flat if b > a + 1 and blocked > 0)
    none = sum(1 for a, b, blocked, cands in flat if b == a + 1 and cands > 0)
    most = max([blocked for a, b, blocked, cands in flat if b > a + 1], default=0)
    return connected, shortened, past, none, most


# ---- rings.  The tree is one chain of poses around a filled disc: a route to the far side has as many rows as the chain has vertices,
# and from any anchor the words to the far rows cross the disc -- dozens of blocked candidates before the farthest visible one.
RING_RHO, RING_NH = 4.0, 64
RINGS = {"small": (60, 85, 50, 170, 150), "large": (120, 150, 110, 300, 300)}  # R, centre (both coordinates), disc radius, grid side, vertices


@functools.lru_cache(maxsize=None)
def ring(name):
    """the integer-rounded points every 2 cells of arc on a circle of radius R, counter-clockwise from angle 0, each with the heading
    index nearest its tangent, given as the sample stream in order (RRTDubins: the nearest vertex is the one before).  The goals: the
    last vertex's pose, the poses of vertices j // 2 and j // 3, the last pose with heading + 3, and the centre cell (on the disc)."""
    R, ctr, disc, side, nv = RINGS[name]
    og8 = np.zeros((side, side), dtype=np.uint8)
    xx, yy = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    og8[(xx - ctr) ** 2 + (yy - ctr) ** 2 <= disc * disc] = 1
    poses = []
    for i in range(nv):
        phi = 2.0 * i / R
        h = int(round((phi + math.pi / 2.0) / (2.0 * math.pi / RING_NH))) % RING_NH
        poses.append((int(round(ctr + R * math.cos(phi))), int(round(ctr + R * math.sin(phi))), h))

    def goals(ro):
        j = ro.j
        at = lambda u: (int(ro.pts[u][0]), int(ro.pts[u][1]), int(ro.head[u]))
        last = at(j - 1)
        return [last, at(j // 2), at(j // 3), (last[0], last[1], (last[2] + 3) % RING_NH), (ctr, ctr, 0)]

    w = poseref.made(f"ring {name}", og8, nv, 0, 0, RING_RHO, RING_NH, poses[0], (2, 2, 0), [p[:2] for p in poses[1:]] + [(0, 0)],
                     [p[2] for p in poses[1:]] + [0], goals)
    return prr.made_case(w)
