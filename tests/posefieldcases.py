"""The cases of the pose_field tests that more than one module uses, each restated by posefieldref once per process: windows of the
poseref workloads, the whole of a small map, windows at the edges of a grid no bucket edge divides, the trees of a given size, the
exact ties between vertices and between headings, a kept view, and a 256 x 256 map whose windows get runs of several cells.  A reference is all nh answers of every free cell of its window --
the fixed-heading answers and the any-heading answer are read off it --, and every one stays below about 1.5 million (vertex, pose)
pairs."""
import os
import re

import numpy as np

import oracle
import posefieldref
import posekeepref
import poseref
from rrtplanner_amd import hostprep, perlin_occupancygrid
from rrtplanner_amd.oggen import random_connected_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def reference(key, w, window, alive=None, og8=None):
    """posefieldref.field of the oracle's tree of workload w over a window, once per process"""
    ro = w.ro
    return _once(("field", key, tuple(window)),
                 lambda: posefieldref.field(w.og8 if og8 is None else og8, ro.pts, ro.head, ro.vcost, w.j, w.rho, w.nh, window, alive))


def headings_of(nh):
    """what every case asks: any heading, and two fixed ones (one, where the planner has one heading)"""
    return [-1] + sorted({nh // 3, nh - 1})


def cells_of(window, seed, m=16):
    """m cells drawn from a window"""
    x0, y0, w, h = window
    rng = np.random.default_rng(seed)
    return np.stack([x0 + rng.integers(0, w, size=m), y0 + rng.integers(0, h, size=m)], axis=1)


# ------------------------------------------------------------------------------------------------ the workloads of poseref
# nh is 16, 8, 64, 1 and 256.  The windows lie away from the root; those of CLUTTERED span obstacles, cells cut off from the tree and
# the territories of several vertices (test_pose_field_cpu.py holds them to it).
WINDOWS = {"A": (56, 50, 10, 10), "B": (72, 48, 10, 10), "E": (43, 9, 8, 8), "G1": (45, 52, 10, 10), "G256": (28, 31, 5, 4)}
CLUTTERED = ("B", "E")


def workload(name):
    """(workload, window, reference)"""
    w = poseref.workload(name)
    return w, WINDOWS[name], reference(name, w, WINDOWS[name])


# ------------------------------------------------------------------------------------------------ one call on a whole map
def small_map():
    """a 24 x 24 map with a wall and a block, a tree of some 40 poses: the whole grid is one window"""
    def make():
        og8 = np.zeros((24, 24), dtype=np.uint8)
        og8[11:13, 0:16] = 1
        og8[17:20, 18:22] = 1
        rng = np.random.default_rng(77)
        free = np.argwhere(og8 == 0)
        n, nh = 60, 8
        cells = free[rng.permutation(len(free))[:n]]
        return poseref.made("small map", og8, n, 1, 8, 1.5, nh, (3, 3, 0), (21, 4, 6), cells, rng.integers(0, nh, n), [(21, 4, 6)])
    w = _once("small", make)
    return w, (0, 0, 24, 24), reference("small", w, (0, 0, 24, 24))


# ------------------------------------------------------------------------------------------------ window shapes on 96 x 100
def edge_windows():
    """one cell, one row, one column, the last column, the four corners of workload B's grid: 96 x 100, which no power of two above 2
    divides on both sides, so the last row and the last column of buckets are cut"""
    W, H = poseref.workload("B").og8.shape
    assert (W, H) == (96, 100)
    return [(70, 30, 1, 1), (0, 41, W, 1), (65, 0, 1, H), (W - 1, 0, 1, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]


def edge_window(k):
    w = poseref.workload("B")
    win = edge_windows()[k]
    return w, win, reference("B", w, win)


# ------------------------------------------------------------------------------------------------ trees of a given size
SIZES = (1, 2, 63, 64, 65, 129, 1025)  # no vertex but the root, exactly one wave of pairs at one heading, one more, more than one list chunk
# before the wall of poseref's stride map, in the tree's half behind the screen that hides it from the root; behind the wall; and around the
# root's own cell, where the cost is 0.0 and a bound clamped to 0 equals it
SIZED_WINDOWS = ((44, 46, 3, 4), (98, 28, 3, 4), (30, 47, 2, 2))


def sized(j, k):
    """(workload, window, reference) of poseref.stride_tree(j, j % 2) over SIZED_WINDOWS[k]"""
    w = poseref.stride_tree(j, j % 2)
    return w, SIZED_WINDOWS[k], reference(("sized", j), w, SIZED_WINDOWS[k])


# ------------------------------------------------------------------------------------------------ ties between vertices
TIE_WINDOW = (43, 46, 3, 3)      # around (44, 47), the cell poseref.tie_duplicate asks every heading of
MIRROR_WINDOW = (89, 49, 3, 3)   # around (90, 50), the goal of poseref.tie_collinear


def tie_duplicate(rho, nh, star):
    w = poseref.tie_duplicate(rho, nh, star, "first")
    return w, TIE_WINDOW, reference(("dup", rho, nh, star), w, TIE_WINDOW)


def tie_mirror(rho, nh, star):
    a, b, iL, iR = poseref.tie_collinear(rho, nh, star, 0)
    return b, iL, iR, MIRROR_WINDOW, reference(("mirror", rho, nh, star), b, MIRROR_WINDOW)


# ------------------------------------------------------------------------------------------------ a tie between headings
def heading_tie():
    """The cells straight behind poseref.TIE_START on its empty map, for the trees of poseref.tie_duplicate over TIE_PAIRS: the first
    cell whose two cheapest headings (each with its (cost, index)-first vertex) have bit-equal costs.  (workload, window of that one
    cell, reference, the two headings), or None if the search finds none."""
    def make():
        x, y, _ = poseref.TIE_START
        for rho, nh in poseref.TIE_PAIRS:
            w = poseref.tie_duplicate(rho, nh, 1, "first")
            for cx in range(x - 1, -1, -1):
                f = reference(("behind", rho, nh), w, (cx, y, 1, 1))
                c = f.cost[0, 0]
                order = np.argsort(c, kind="stable")
                if nh > 1 and np.isfinite(c[order[0]]) and c[order[0]].view(np.int64) == c[order[1]].view(np.int64):
                    return w, (cx, y, 1, 1), f, (int(order[0]), int(order[1]))
        return None
    return _once("heading tie", make)


# ------------------------------------------------------------------------------------------------ a kept view
KEPT = "B"


def kept():
    """(Kept of posekeepref on workload B's map plus the six blocks, window, the reference over the alive vertices on the new map)"""
    k = posekeepref.changed(KEPT)
    win = WINDOWS[KEPT]
    return k, win, reference("kept", k.w, win, alive=k.alive, og8=k.og8)


# ------------------------------------------------------------------------------------------------ runs of more than one cell
def _abi(name):
    text = open(os.path.join(ROOT, "rrtplanner_amd", "csrc", "rrt_kernel_abi.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def run_of(window):
    """the consecutive cells of a column that one wavefront decides in this window, as rrt_tree_calls.hip chooses them:
    clamp(w * h / POSE_FIELD_WAVES, 1, POSE_FIELD_RUN).  From the second cell of a run on, a cell starts from the winner of the cell
    before it, and its scan leaves no bucket out; with runs of one cell neither happens."""
    return int(np.clip(window[2] * window[3] // _abi("POSE_FIELD_WAVES"), 1, _abi("POSE_FIELD_RUN")))


def tiles(window, side=64):
    """the window cut into tiles of at most side x side cells, each of which gets runs of one cell"""
    x0, y0, w, h = window
    return [(x, y, min(side, x0 + w - x), min(side, y0 + h - y)) for x in range(x0, x0 + w, side) for y in range(y0, y0 + h, side)]


WIDE_WINDOWS = ((0, 0, 256, 256), (3, 5, 192, 128), (0, 0, 256, 250))  # runs of 16, of 6 (128 = 21 * 6 + 2) and of 15 (250 = 16 * 15 + 10)
WIDE_PROBES = ((0, 8), (1, 6), (2, 6))  # (place, side): windows of side x side around the tree's root, a vertex that the kept view loses and its middle one


def wide():
    """a 256 x 256 noise map and a Dubins-RRT* tree of some 300 poses with 8 headings: windows of it have 24 576 to 65 536 cells"""
    def make():
        og = perlin_occupancygrid(256, 256, seed=4)
        og8 = oracle.og_u8(og)
        xs, xg = random_connected_pair(og, np.random.default_rng(12))
        rng = np.random.default_rng(13)
        n, nh = 320, 8
        samples = hostprep.draw_free_samples(rng, np.argwhere(og8 == 0), n)
        return poseref.made("wide", og8, n, 1, 24, 3.0, nh, (int(xs[0]), int(xs[1]), 1), (int(xg[0]), int(xg[1]), 5), samples, rng.integers(0, nh, n),
                            [(int(xg[0]), int(xg[1]), 5)])
    return _once("wide", make)


def wide_probes(w):
    """small windows inside every window of WIDE_WINDOWS, around three vertices of the tree: where the restatement is affordable"""
    pts, dead = w.ro.pts[:w.j], ~wide_kept()[1]
    inside = (pts[:, 0] >= 8) & (pts[:, 0] < 185) & (pts[:, 1] >= 10) & (pts[:, 1] < 123)
    lost = int(np.flatnonzero(dead & inside)[0])  # the first vertex inside all windows that the kept view lost
    out = []
    for place, side in WIDE_PROBES:
        v = (0, lost, w.j // 2)[place]
        x, y = int(w.ro.pts[v, 0]), int(w.ro.pts[v, 1])
        out.append((int(np.clip(x - 1, 3, 195 - side)), int(np.clip(y - 1, 5, 133 - side)), side, side))
    return out


def wide_kept():
    """the wide tree kept on its map plus six blocks: (new map, alive)"""
    def make():
        w = wide()
        og2 = posekeepref.blocks_map(w.og8, w.xs, count=8, size=12, seed=2, clear=20)
        return og2, posekeepref.alive(og2, w.ro.pts, w.ro.head, w.ro.parent, w.j, w.rho, w.nh)
    return _once("wide kept", make)
