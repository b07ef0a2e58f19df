"""Which iterations of a query reach the terminal pass of the cell-record nearest-vertex search.

rrt_pipe_kernel (rrt_pipe.h) and the Dubins block kernel (rrt_dubins_block.h) do not look at the whole node array for the
nearest vertex: they stream the records of the cells in a box around the sample, leave out every cell whose rectangle is
farther from the sample than the box radius, and widen the box while nothing was found near enough.  The last box of that
search (the *terminal pass*) is the one after which the search stops widening; if it still leaves out a cell, a vertex in
that cell is never looked at unless something else (a scan over every vertex) follows.

This module restates that geometry, nothing more:
  * cell shift: `cell_geometry` in rrt_engine.hip -- 16-pixel cells, wider only when sqrt(r2) / div reaches 32 (div 4 for the
    one-CU pipeline, RRT_CELL_DIV_PIPE; div 2 for every other kernel, RRT_CELL_DIV, Dubins among them), and wider again while
    the grid has more than MAX_CELLS cells;
  * first radius: rrt_pipe.h / rrt_dubins_block.h, "radius of the first record stream": rr0 = r2 for RRT* when r2 exceeds two
    cells squared, else (2 << shift)^2; rad0 = the largest integer with rad0^2 <= rr0 - 1 (4096 from rr0 >= 2^23); that stream
    keeps every cell within rr0 - 1;
  * the widening as the parent commit had it: the pipe doubles once (2 rad0 + 1, keeping radn^2) and scans every vertex if a
    miss remains and radn < max(W, H); Dubins doubles while radn < max(W, H);
  * trees of up to PP_TINY = DB_TINY = 64 vertices are read whole (no cells).

An iteration *reaches the terminal pass* when the terminal radius is at least max(W, H) (so no full scan follows), the
snapshot holds more than 64 vertices, and the cell of the oracle's nearest vertex lies farther from the sample than the
terminal pass keeps (the vertex itself is then farther than the terminal radius too).  It is a *no-vertex* iteration when
every vertex of the snapshot sits in such a cell.  Only the oracle's tree is looked at; the kernel's answer is not modelled,
so the counts mean the same before and after the kernels were fixed.
"""
import math

import numpy as np

import oracle
from rrtplanner_amd import hostprep

TINY = 64          # PP_TINY (rrt_pipe.h), DB_TINY (rrt_dubins_block.h)
MAX_CELLS = 4096   # rrt_kernel_abi.h
DIV_PIPE, DIV_OTHER = 4.0, 2.0  # RRT_CELL_DIV_PIPE, RRT_CELL_DIV (rrt_engine.hip)


def cell_shift(W, H, r2, div):
    r = math.sqrt(max(int(r2), 1))
    shift = 4
    while (1 << (shift + 1)) <= r / div and shift < 11:
        shift += 1
    while ((W + (1 << shift) - 1) >> shift) * ((H + (1 << shift) - 1) >> shift) > MAX_CELLS:
        shift += 1
    return shift


def first_radius(star, r2, shift):
    """(rad0, keep0): the first stream's box half-width and the largest squared cell distance it keeps."""
    two = (2 << shift) * (2 << shift)
    rr = r2 if (star and r2 > two) else two
    rad0 = 4096 if rr >= (1 << 23) else math.isqrt(rr - 1)
    return rad0, rr - 1


def terminal_pass(kind, W, H, star, r2):
    """(shift, radius, keep) of the parent's terminal pass, or None where a miss after the last box scans every vertex."""
    m = max(W, H)
    if kind == "pipe":
        shift = cell_shift(W, H, r2, DIV_PIPE)
        rad0, keep0 = first_radius(star, r2, shift)
        if rad0 >= m:
            return shift, rad0, keep0
        radn = 2 * rad0 + 1
        return (shift, radn, radn * radn) if radn >= m else None
    assert kind == "dubins"
    shift = cell_shift(W, H, r2, DIV_OTHER)
    radn, keep = first_radius(star, r2, shift)
    while radn < m:
        radn = 2 * radn + 1
        keep = radn * radn
    return shift, radn, keep


def _cell_d2(sx, sy, cx, cy, shift):
    """squared distance of samples (sx, sy) to the rectangles of cells (cx, cy) (broadcasting)"""
    xl, yl = cx << shift, cy << shift
    xh, yh = xl + (1 << shift) - 1, yl + (1 << shift) - 1
    dx = np.where(sx < xl, xl - sx, np.where(sx > xh, sx - xh, 0))
    dy = np.where(sy < yl, yl - sy, np.where(sy > yh, sy - yh, 0))
    return dx * dx + dy * dy


def coverage(kind, W, H, star, r2, samples, pts, nearest_log, jlog):
    """Per-query counts: iterations that reach the terminal pass, no-vertex iterations, and reaching iterations where a kept
    vertex is as near as the (culled, lower-index) nearest one.  jlog[i] = tree size before iteration i."""
    out = dict(reach=0, novertex=0, ties=0, first=-1, start_culled=0)
    tp = terminal_pass(kind, W, H, star, r2)
    if tp is None:
        return out
    shift, _, keep = tp
    samples = np.asarray(samples, dtype=np.int64)
    pts = np.asarray(pts, dtype=np.int64)
    nl = np.asarray(nearest_log, dtype=np.int64)
    jl = np.asarray(jlog, dtype=np.int64)
    it = np.flatnonzero((jl > TINY) & (nl >= 0))
    if it.size == 0:
        return out
    sx, sy = samples[it, 0], samples[it, 1]
    nn = nl[it]
    culled = _cell_d2(sx, sy, pts[nn, 0] >> shift, pts[nn, 1] >> shift, shift) > keep
    # the lowest vertex index of every cell: a cell holds a vertex of snapshot j iff that index is below j
    ncx, ncy = (W + (1 << shift) - 1) >> shift, (H + (1 << shift) - 1) >> shift
    jmax = int(jl.max())
    cid = (pts[:jmax, 0] >> shift) * ncy + (pts[:jmax, 1] >> shift)
    first_in = np.full(ncx * ncy, np.iinfo(np.int64).max)
    np.minimum.at(first_in, cid, np.arange(jmax))
    cx, cy = np.divmod(np.arange(ncx * ncy), ncy)
    cd2 = _cell_d2(sx[:, None], sy[:, None], cx[None, :], cy[None, :], shift)
    kept_occupied = ((cd2 <= keep) & (first_in[None, :] < jl[it, None])).any(axis=1)
    out["reach"] = int(culled.sum())
    out["novertex"] = int((culled & ~kept_occupied).sum())
    # vertex 0 is in every snapshot, also in an older one that a kernel resolves against ahead of retirement
    out["start_culled"] = int((_cell_d2(sx, sy, pts[0, 0] >> shift, pts[0, 1] >> shift, shift) > keep).sum())
    for k in np.flatnonzero(culled & kept_occupied):
        i, j = it[k], jl[it[k]]
        d2 = ((pts[:j] - samples[i]) ** 2).sum(axis=1)
        vc = _cell_d2(samples[i, 0], samples[i, 1], pts[:j, 0] >> shift, pts[:j, 1] >> shift, shift)
        out["ties"] += int(np.any((vc <= keep) & (d2 == d2[nl[i]])))
    if out["reach"]:
        out["first"] = int(it[np.flatnonzero(culled)[0]])
    return out


# ------------------------------------------------------------------------------------------------------ pocket maps
def _union(W, H, rects):
    m = np.zeros((W, H), dtype=bool)
    for (x0, x1), (y0, y1) in rects:
        m[x0:x1 + 1, y0:y1 + 1] = True
    return m


def pocket_grid(W, H, rects, field=None):
    """A free W x H map with one obstacle ring (8-neighbourhood, one cell wide) around the union of `rects`, each
    ((x0, x1), (y0, y1)) inclusive.  A tree started inside stays inside; samples are drawn over the whole free map.
    field: instead, every cell is an obstacle but the pocket and the union of these rectangles (free cells that only draw
    samples: a field near the opposite corner sends a larger share of the samples to where the far cells are left out)."""
    inside = _union(W, H, rects)
    if field is not None:
        return (~(inside | _union(W, H, field))).astype(np.uint8)
    grown = inside.copy()
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            sh = np.zeros_like(inside)
            sh[max(dx, 0):W + min(dx, 0), max(dy, 0):H + min(dy, 0)] = inside[max(-dx, 0):W + min(-dx, 0), max(-dy, 0):H + min(-dy, 0)]
            grown |= sh
    return (grown & ~inside).astype(np.uint8)


# RRTStandard / RRT* on the one-CU pipeline.  alg 0 / 1, r_rewire (None: RRTStandard), start and goal inside the pocket.
# parent_safe: the CPU check finds no no-vertex iteration, and the start (vertex 0, in every snapshot) sits in the strip, in a
# cell that no terminal pass leaves out -- so no snapshot is without a kept vertex (the parent commit's library may run it).
PIPE_CASES = [
    dict(id="L63_std", W=63, H=63, rects=[((48, 62), (48, 62)), ((56, 62), (40, 47))], alg=0, rr=None, n=3000, seed=1,
         xs=(59, 44), xg=(50, 52), parent_safe=True),
    dict(id="L63_star64", W=63, H=63, rects=[((48, 62), (48, 62)), ((56, 62), (40, 47))], alg=1, rr=64, n=3000, seed=1,
         xs=(59, 44), xg=(50, 52), parent_safe=True),
    dict(id="sq63_std", W=63, H=63, rects=[((48, 62), (48, 62))], alg=0, rr=None, n=3000, seed=1,
         xs=(60, 60), xg=(50, 52), parent_safe=False),
    # W != H: only max(W, H) = 63 ends the doubling; a field of free cells at the origin draws the samples that cull the pocket
    dict(id="rect63x56_std", W=63, H=56, rects=[((48, 62), (48, 55)), ((59, 62), (40, 47))], field=[((0, 6), (0, 6))], alg=0,
         rr=None, n=3000, seed=2, xs=(60, 44), xg=(50, 50), parent_safe=True),
]

# Dubins-RRT / RRT* (the default kernel and the serial one) on 127 x 127: the doubling 31 -> 63 -> 127 ends short of the
# diagonal (179).  r_rewire = 24 keeps the first radius at two 16-pixel cells; rho is small against the pocket.
_L127 = [((96, 126), (96, 126)), ((121, 126), (60, 95))]
DUBINS_CASES = [
    dict(id="L127_dub", W=127, H=127, rects=_L127, field=[((0, 12), (0, 12))], star=0, rr=None, rho=2.0, n=6000, seed=1,
         xs=(123, 62, 16), xg=(100, 104, 20), parent_safe=True),
    dict(id="L127_dubstar", W=127, H=127, rects=_L127, field=[((0, 12), (0, 12))], star=1, rr=24, rho=2.0, n=6000, seed=1,
         xs=(123, 62, 16), xg=(100, 104, 20), parent_safe=True),
    # a culled vertex and a kept one equally near, the culled one of lower index (the lowest index must win)
    dict(id="L127_dub_ties", W=127, H=127, rects=[((96, 126), (96, 126)), ((121, 126), (60, 95))], field=[((0, 12), (0, 12))],
         star=0, rr=None, rho=1.0, n=6000, seed=1, xs=(123, 61, 16), xg=(100, 104, 20), parent_safe=True, ties=True),
    dict(id="sq127_dub", W=127, H=127, rects=[((96, 126), (96, 126))], field=[((0, 9), (0, 9))], star=0, rr=None, rho=2.0,
         n=6000, seed=1, xs=(122, 122, 5), xg=(100, 104, 20), parent_safe=False),
]


def pipe_case(c):
    """(og8, samples, r2) of a pipe case: the draws of devcheck.oracle_vs_device"""
    og8 = pocket_grid(c["W"], c["H"], c["rects"], c.get("field"))
    samples = hostprep.draw_free_samples(np.random.default_rng(c["seed"]), np.argwhere(og8 == 0), c["n"])
    r2 = hostprep.radius_threshold(c["rr"]) if c["rr"] is not None else 0
    return og8, samples, r2


def dubins_case(c, nh=64):
    """(og8, samples, heads, r2) of a Dubins case: the draws of test_dubins._dub_query"""
    og8 = pocket_grid(c["W"], c["H"], c["rects"], c.get("field"))
    rng = np.random.default_rng(c["seed"])
    samples = hostprep.draw_free_samples(rng, np.argwhere(og8 == 0), c["n"])
    heads = rng.integers(0, nh, size=c["n"])
    r2 = hostprep.radius_threshold(c["rr"]) if c["star"] else 0
    return og8, samples, heads, r2


def pipe_fuzz_cases(count=24, seed=20261016):
    """The pocket fuzz: W, H in [60, 63], n = 8000, pocket [48, W-1] x [48, H-1], in about half the cases a strip
    [W-k, W-1] x [40, 47] with k in [4, 7]; RRTStandard or RRT* with r_rewire = 64; start and goal drawn in the pocket."""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(count):
        W, H = int(rng.integers(60, 64)), int(rng.integers(60, 64))
        rects = [((48, W - 1), (48, H - 1))]
        if rng.uniform() < 0.5:
            k = int(rng.integers(4, 8))
            rects.append(((W - k, W - 1), (40, 47)))
        alg = int(rng.integers(0, 2))
        xs = (int(rng.integers(48, W)), int(rng.integers(48, H)))
        xg = (int(rng.integers(48, W)), int(rng.integers(48, H)))
        out.append(dict(id=f"fuzz{case}", W=W, H=H, rects=rects, alg=alg, rr=64 if alg else None, n=8000, seed=1000 + case,
                        xs=xs, xg=xg))
    return out


def dubins_fuzz_cases(count=8, seed=20261017):
    """Dubins pockets on squares and rectangles with 63 < max(W, H) <= 127 whose doubling (31, 63, 127) ends short of the
    diagonal: the far corner block of 16-pixel cells, in about half the cases with a strip along the far edge, and a field of
    free cells at the origin."""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(count):
        W, H = int(rng.integers(112, 128)), int(rng.integers(112, 128))
        rects = [((96, W - 1), (96, H - 1))]
        if rng.uniform() < 0.5:
            rects.append(((W - int(rng.integers(3, 7)), W - 1), (int(rng.integers(56, 61)), 95)))
        f = int(rng.integers(8, 13))
        star = int(rng.integers(0, 2))
        xs = (int(rng.integers(98, W - 1)), int(rng.integers(98, H - 1)), int(rng.integers(0, 64)))
        xg = (int(rng.integers(98, W - 1)), int(rng.integers(98, H - 1)), int(rng.integers(0, 64)))
        out.append(dict(id=f"dfuzz{case}", W=W, H=H, rects=rects, field=[((0, f), (0, f))], star=star, rr=24 if star else None,
                        rho=float(rng.choice([1.0, 1.5, 2.0])), n=5000, seed=2000 + case, xs=xs, xg=xg))
    return out


def run_pipe_oracle(c):
    og8, samples, r2 = pipe_case(c)
    st, ro = oracle.plan(og8, c["n"], c["alg"], c["xs"], c["xg"], samples, r2_rewire=r2)
    cov = coverage("pipe", c["W"], c["H"], c["alg"] >= 1, r2, samples, ro.pts, ro.nearest_log, ro.jlog)
    return og8, samples, r2, st, ro, cov


def dubins_jlog(ro):
    """tree size before every iteration of oracle.dubins_plan (vertex 0 is the start; the goal vertex is appended at the end)"""
    acc = np.asarray(ro.accept_log, dtype=np.int64)
    return 1 + np.concatenate([[0], np.cumsum(acc)[:-1]])


def run_dubins_oracle(c, nh=64):
    og8, samples, heads, r2 = dubins_case(c, nh)
    st, ro = oracle.dubins_plan(og8, c["n"], c["star"], c["xs"], c["xg"], samples, heads, r2_rewire=r2, rho=c["rho"], nh=nh)
    cov = coverage("dubins", c["W"], c["H"], bool(c["star"]), r2, samples, ro.pts, ro.nearest_log, dubins_jlog(ro))
    return og8, samples, heads, r2, st, ro, cov
