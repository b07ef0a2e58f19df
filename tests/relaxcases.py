"""The inputs of the relax tests (tests/test_relax_cpu.py, tests/test_relax_gpu.py): crafted sample streams through RRTStandard /
RRTStar, planned by the oracle and cached once per process, and the restatement's answer for each (relaxref.relax), cached too.
test_relax_cpu.py asserts what each input is for."""
import numpy as np

import relaxref
import treecalls as tc
from rrtplanner_amd import hostprep

_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _padded(samples, n):
    """the stream filled up to n with repeats of its first sample, which the loop refuses: its cell is a vertex's"""
    s = np.asarray(samples, dtype=np.int64).reshape(-1, 2)
    return np.concatenate([s, np.tile(s[:1], (n - len(s), 1))])


def _case(key, og8, alg, xs, xg, samples, r2):
    def make():
        n = max(len(samples) + 8, 300)  # (room behind the tree, and no smaller a query than the other tree-call tests plan)
        c = tc.oracle_case(np.ascontiguousarray(og8, dtype=np.uint8), alg, n, np.asarray(xs), xg, _padded(samples, n), r2)
        c["key"] = key
        return c
    return _once(key, make)


def ties():
    """three vertices in a row: (20, 10) is reached at the same cost over (15, 10) and over (13, 10), and with r = 11 from the root too"""
    return _case(("ties",), np.zeros((40, 24)), 0, (10, 10), (30, 10), [(15, 10), (13, 10), (20, 10)], 0)


def long_edge():
    """a detour 0 -> 1 -> 2 -> 3, an edge 3 -> 4 of 37 cells with a cluster behind it, and the root's cell sampled again (vertex 7)"""
    return _case(("long_edge",), np.zeros((24, 64)), 0, (5, 5), (20, 60), [(12, 5), (12, 12), (6, 13), (6, 50), (8, 52), (4, 53), (5, 5)], 0)


def blocked(cols, rows, alg):
    """a wall with one gap far from the start; a cluster of cols x rows vertices on the start's side of it and a few vertices right
    behind it, which the tree reaches through the gap: for those every vertex of the cluster is a cheaper candidate that is blocked"""
    def build():
        og = np.zeros((64, 64))
        og[30:32, :] = 1
        og[30:32, 2:5] = 0
        way = tc.march([(10, 32), (10, 3), (36, 3), (36, 32)], step=3)
        behind = [(x, y) for x in (35, 34) for y in range(29, 36)]
        cluster = [(16 + a, 26 + b) for a in range(cols) for b in range(rows)]
        return og, np.concatenate([way, behind, cluster])
    og, samples = build()
    return _case(("blocked", cols, rows, alg), og, alg, (10, 32), (60, 60), samples, tc.R2 if alg else 0)


def zigzag():
    """a chain of 1100 vertices in steps of (3, +-1): skipping a vertex is 6 cells against 2 sqrt(10).  At 3 cells a step the chain is
    3300 cells long and the kernels' grids end at 2048 a side, so it runs along x, turns in three steps of (+-1, 3) and runs back 10
    rows further, out of reach of r = 7."""
    pts = [(2, 2)]
    for k in range(1, 550):
        pts.append((2 + 3 * k, 2 + k % 2))
    x, y = pts[-1]
    for t in range(1, 4):
        pts.append((x + t % 2, y + 3 * t))
    x, y = pts[-1]
    for k in range(1, 1100 - len(pts) + 1):
        pts.append((x - 3 * k, y + k % 2))
    assert len(pts) == 1100
    return _case(("zigzag",), np.zeros((1680, 24)), 0, pts[0], (1670, 20), pts[1:], 0)


def sized(k):
    og8, xs, samples, n = tc.sized(k, 100 + k)
    xg = (63, 63) if tuple(xs) != (63, 63) else (0, 0)
    return _once(("sized", k), lambda: dict(tc.oracle_case(og8, 0, n, xs, xg, samples, 0), key=("sized", k)))


def base(alg):
    return tc.base(alg=alg)


def R_of(r):
    return hostprep.radius_threshold(r)


FIXTURES = {  # name -> (case, r)
    "ties8": (ties, 8), "ties11": (ties, 11), "long_edge": (long_edge, 10), "blocked70": (lambda: blocked(7, 10, 0), 24),
    "blocked144": (lambda: blocked(12, 12, 1), 24), "near1025": (lambda: sized(1025), 24), "zigzag": (zigzag, 7),
}


def tree(c):
    ro = c["ro"]
    return np.array(ro.pts[:ro.j], dtype=np.int64), np.array(ro.parent[:ro.j], dtype=np.int64), np.array(ro.vcost[:ro.j]), ro.j


def relaxed(c, r, og8=None, view=False):
    """relaxref.relax of the oracle's tree of case c with radius r, on the case's map or on og8 (view: the tree was kept on og8)"""
    key = ("relaxed", c["key"], r, None if og8 is None else og8.tobytes(), view)
    m = c["og8"] if og8 is None else og8
    return _once(key, lambda: relaxref.relax(m, *tree(c), R_of(r), og8_view=m if view else None))


def fixture(name):
    make, r = FIXTURES[name]
    c = make()
    return c, r, relaxed(c, r)
