"""The inputs of the pose relax tests (tests/test_pose_relax_cpu.py, tests/test_pose_relax_gpu.py): poseref's workloads and crafted pose
streams through RRTDubins / RRTStarDubins, planned by the oracle and cached once per process, and the restatement's answer for each
(poserelaxref.relax), cached too.  test_pose_relax_cpu.py asserts what each input is for."""
import functools
import os
import re

import numpy as np

import poserelaxref
import poseref
from rrtplanner_amd import hostprep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025)
SIZES_R = 12


def R_of(r):
    return hostprep.radius_threshold(r)


def list_cap():
    """POSE_RELAX_LIST as rrt_kernel_abi.h states it: the survivors a wavefront lists in LDS at a time"""
    text = open(os.path.join(ROOT, "rrtplanner_amd", "csrc", "rrt_kernel_abi.h")).read()
    return int(re.search(r"constexpr int POSE_RELAX_LIST = (\d+);", text).group(1))


def _march(corners, step):
    """the cells from corner to corner in steps of `step`, each corner included, with the heading index (of 8) of the leg that leaves the cell"""
    cells, heads = [], []
    for (ax, ay), (bx, by) in zip(corners[:-1], corners[1:]):
        dx, dy = np.sign(bx - ax), np.sign(by - ay)
        h = {(1, 0): 0, (0, 1): 2, (-1, 0): 4, (0, -1): 6}[(int(dx), int(dy))]
        n = max(abs(bx - ax), abs(by - ay))
        for t in range(0, n, step):
            cells.append((ax + dx * t, ay + dy * t))
            heads.append(h)
    cells.append(corners[-1])
    heads.append(heads[-1])
    return cells, heads


@functools.lru_cache(maxsize=None)
def ties():
    """the start heads along +x; (15, 10), (13, 10) and (20, 10) with that heading.  RRTDubins hangs the last two on (15, 10), the second
    by a loop.  Relaxed at r = 8, (13, 10) is reached straight from the start at cost 3, and (20, 10) at cost 10 over (15, 10) [5 + 5]
    and over (13, 10) [3 + 7]: the lower number loses to the lower cost."""
    og8 = np.zeros((40, 24), dtype=np.uint8)
    cells = [(15, 10), (13, 10), (20, 10), (0, 0)]
    return poseref.made("relax ties", og8, len(cells), 0, 0, 1.5, 8, (10, 10, 0), (30, 10, 0), cells, [0, 0, 0, 0], [(30, 10, 0)])


@functools.lru_cache(maxsize=None)
def blocked(cols, rows, star):
    """a wall with one gap far from the start; the tree marches through the gap and up behind the wall; a cluster of cols x rows poses
    on the start's side: for the vertices right behind the wall every vertex of the cluster is a cheaper candidate whose word is blocked"""
    og8 = np.zeros((64, 64), dtype=np.uint8)
    og8[30:32, :] = 1
    og8[30:32, 2:7] = 0
    way, wh = _march([(10, 32), (10, 4), (36, 4), (36, 33)], 2)
    behind = [(x, y) for x in (35, 34) for y in range(29, 36)]
    cluster = [(16 + a, 26 + b) for a in range(cols) for b in range(rows)]
    cells = way[1:] + behind + cluster + [(0, 0)]
    heads = wh[1:] + [2] * len(behind) + [0] * len(cluster) + [0]
    return poseref.made(f"relax blocked {cols}x{rows} star {star}", og8, len(cells) + 24, star, 24, 1.5, 8, (10, 32, 6), (60, 60, 0),
                        cells + [(0, 0)] * 24, heads + [0] * 24, [(60, 60, 0)])


@functools.lru_cache(maxsize=None)
def chain():
    """a chain of 260 poses heading along +x in steps of (3, +-1), each hung on the one before by RRTDubins: skipping a vertex is a
    straight word of 6 cells against two S-curves of more than sqrt(10) each, and the gain travels down the chain two vertices a round"""
    j = 260
    og8 = np.zeros((3 * j + 16, 8), dtype=np.uint8)
    cells = [(2 + 3 * k, 3 + k % 2) for k in range(1, j)] + [(0, 0)]
    return poseref.made("relax chain", og8, len(cells), 0, 0, 0.5, 8, (2, 3, 0), (3 * j + 10, 3, 0), cells, [0] * len(cells), [(3 * j + 10, 3, 0)])


def sized(j):
    return poseref.stride_tree(j, 1)


def crowd():
    """1025 vertices of RRTDubins in 60 x 96 cells: at r = 30 a late vertex has more cheaper neighbours than the LDS list holds"""
    return poseref.stride_tree(1025, 0)


FIXTURES = {  # name -> (workload, r)
    "ties8": (ties, 8), "duplicate": (lambda: poseref.tie_duplicate(1.5, 8, 1, "first"), 20), "long_edge": (lambda: poseref.workload("D"), 6),
    "blocked70": (lambda: blocked(7, 10, 0), 24), "blocked144": (lambda: blocked(12, 12, 1), 24), "crowd": (crowd, 30), "chain": (chain, 7),
}
WORKLOADS = {"A": 20, "C": 40, "D": 20, "E": 12}  # poseref's, and the radius each is relaxed at (D, an RRTDubins tree, has none of its own)

_cache = {}


def tree(w):
    ro, j = w.ro, w.j
    return (np.array(ro.pts[:j], dtype=np.int64), np.array(ro.head[:j], dtype=np.int64), np.array(ro.parent[:j], dtype=np.int64),
            np.array(ro.vcost[:j], dtype=np.float64), j)


def relaxed(w, r, og8=None, view=False):
    """poserelaxref.relax of the oracle's tree of workload w with radius r, on its own map or on og8 (view: the tree was kept on og8)"""
    key = (w.name, r, None if og8 is None else og8.tobytes(), view)
    if key not in _cache:
        m = w.og8 if og8 is None else og8
        _cache[key] = poserelaxref.relax(m, *tree(w), R_of(r), w.rho, w.nh, og8_view=m if view else None)
    return _cache[key]


def fixture(name):
    if name in WORKLOADS:
        w, r = poseref.workload(name), WORKLOADS[name]
    elif name.startswith("sized"):
        w, r = sized(int(name[5:])), SIZES_R
    else:
        make, r = FIXTURES[name]
        w = make()
    return w, r, relaxed(w, r)


def certified(w, r, X, og8=None):
    return poserelaxref.certify(w.og8 if og8 is None else og8, X.pts, X.head, X.parent, X.vcost, R_of(r), w.rho, w.nh,
                                poserelaxref.old_edges_of(X.in_parent, X.order), prev=X.order)
