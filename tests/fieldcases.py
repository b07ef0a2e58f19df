"""The cases of the cost_field tests that more than one module uses, each planned by the oracle and restated by fieldref once per
process: the three maps of plans_A.npz, the exact tie across buckets, and the trees of a given size on a grid no bucket edge divides."""
import numpy as np

import fieldref
import plannedcases
import treecalls as tc
from rrtplanner_amd import hostprep

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def tree(c):
    """(pts, vcost, j) of a case the oracle planned"""
    ro = c["ro"]
    return ro.pts, ro.vcost, ro.j


def reference(key, c, window=None):
    """fieldref.field of a case over a window, once per process: (vertex, cost, tried)"""
    return _once(("field", key, window), lambda: fieldref.field(c["og8"], *tree(c), window))


# ------------------------------------------------------------------------------------------------ the three maps of the issue
NOISE_WINDOW = (60, 70, 64, 48)
PLANNED = {  # name -> (the case, the window of the field; None: the whole grid)
    "maze": (lambda: plannedcases.oracle_planned(*plannedcases.MAZE), None),
    "square": (lambda: plannedcases.oracle_planned("square100", 1, 200, 15), None),
    "noise": (lambda: plannedcases.oracle_planned(*plannedcases.NOISE), NOISE_WINDOW),
}


def planned(name):
    """(case, window as four numbers, fieldref's (vertex, cost, tried) over it)"""
    make, window = PLANNED[name]
    c = make()
    window = fieldref.whole(c["og8"]) if window is None else window
    return c, window, reference(name, c, window)


# ------------------------------------------------------------------------------------------------ an exact tie across buckets
TIE_CELL = (40, 8)
TIE_SAMPLES = ((8, 40), (72, 40))


def tie(swapped):
    """An empty 96 x 96 grid but for the cell (40, 24); RRTStandard from (40, 40) on the samples (8, 40) and (72, 40), or the two
    swapped.  The cell (40, 8) is hidden from the start and costs 32 + sqrt(2048) through either sample, bit for bit; the samples lie
    64 cells apart, in different buckets whatever the edge."""
    def make():
        og8 = np.zeros((96, 96), dtype=np.uint8)
        og8[40, 24] = 1
        samples = np.array(TIE_SAMPLES[::-1] if swapped else TIE_SAMPLES, dtype=np.int64)
        c = tc.oracle_case(og8, 0, 3, (40, 40), (90, 90), np.concatenate([samples, samples[:1]]), 0)
        assert c["ro"].j == 3 and c["ro"].pts[1:3].tolist() == samples.tolist()
        return c
    return _once(("tie", swapped), make)


# ------------------------------------------------------------------------------------------------ trees of a given size
SIZES = (1, 2, 63, 64, 65, 129)
SIZED_SHAPE = (96, 100)  # no power of two above 2 divides both sides: the last row and the last column of buckets are cut


def sized(k):
    """a 96 x 100 map with a wall that leaves a gap at the top, and a tree of exactly k vertices in the empty part left of it: k distinct
    cells in a random order, each accepted (RRT* with a radius of 12 cells).  Right of the wall most cells are hidden from the start."""
    def make():
        og8 = np.zeros(SIZED_SHAPE, dtype=np.uint8)
        og8[60:63, :80] = 1
        cells = np.array([(x, y) for x in range(56) for y in range(100) if (x, y) != (0, 0)])
        samples = cells[np.random.default_rng(300 + k).permutation(len(cells))[:k]]
        c = tc.oracle_case(og8, 1, k, (0, 0), (90, 95), samples, hostprep.radius_threshold(12))
        assert c["ro"].j == k, (c["ro"].j, k)
        return c
    return _once(("sized", k), make)


def sized_windows():
    """one cell, one row, one column, the last column, the four corners"""
    W, H = SIZED_SHAPE
    return [(70, 30, 1, 1), (0, 41, W, 1), (65, 0, 1, H), (W - 1, 0, 1, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
