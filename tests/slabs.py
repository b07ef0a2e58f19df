"""Which iterations of a query make the near-set record stream go past its first 64 cells.

Every cell-record kernel streams the records of the cells in the bounding box of the rewire ball 64 cells at a time
(`stream_cells` in rrt_block_nearset.inc: `for (cbase = 0; cbase < ncr; cbase += 64)`; the same loop in rrt_cell_stream.h, which
rrt_pipe.h and rrt_dubins_block.h run).  Counters, list positions and screens carry over from one slab of 64 cells to the next.  A box has more
than 64 cells only where the radius is large against the cell: for cells r/4 to r/2 wide (divisor 2) that is the top eighth
below a power of two ([56, 64), [112, 128), [224, 256)); a kernel that runs on the other kernel's cell size (divisor 4 cells
under a divisor 2 kernel) gets there at every radius from 64 on.

This module restates that geometry, nothing more (cell shift and constants: tests/farnn.py):
  * the ball's box: rad = the largest integer with rad^2 < r2h, the cells of [x - rad, x + rad] x [y - rad, y + rad] clamped
    to the grid, numbered column by column: position (cx - cx0) * ny + (cy - cy0);
  * a cell is left out (culled) when its rectangle is r2h or farther (squared) from the sample.
An iteration *reaches a later slab* when its snapshot holds more than 64 vertices, the box has more than 64 cells and a cell
at position 64 or later is unculled and holds a vertex of the snapshot: a later slab then delivers a record that the near set
needs.  Only the oracle's tree is looked at; no kernel's answer is modelled.
"""
import math

import numpy as np

import farnn
import oracle
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pair

SLAB = 64            # cells per slab of the record stream
TINY = farnn.TINY    # trees up to this size are read whole by the pipeline kernels
DIV_TEAM, DIV_PIPE = farnn.DIV_OTHER, farnn.DIV_PIPE


def cell_shift(W, H, r2, div):
    return farnn.cell_shift(W, H, r2, div)


def shift_pair(W, H, r2):
    """(divisor 2, divisor 4) cell shifts of a query: a cross-geometry case needs them to differ"""
    return cell_shift(W, H, r2, DIV_TEAM), cell_shift(W, H, r2, DIV_PIPE)


def ball_rad(r2h):
    """largest |dx| with dx * dx < r2h (4096 from 2^23 on, as the kernels have it)"""
    if r2h <= 0:
        return 0
    return 4096 if r2h >= (1 << 23) else math.isqrt(r2h - 1)


def box_cells(W, H, r2h, shift, x, y):
    """(cx0, cx1, cy0, cy1) of the ball's bounding box around (x, y), clamped to the grid; x, y may be arrays"""
    rad = ball_rad(r2h)
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    cx0, cx1 = np.maximum(x - rad, 0) >> shift, np.minimum(x + rad, W - 1) >> shift
    cy0, cy1 = np.maximum(y - rad, 0) >> shift, np.minimum(y + rad, H - 1) >> shift
    return cx0, cx1, cy0, cy1


def largest_box(W, H, r2h, shift):
    """the largest number of cells of a box over every sample position of the grid"""
    cx0, cx1, _, _ = box_cells(W, H, r2h, shift, np.arange(W), 0)
    _, _, cy0, cy1 = box_cells(W, H, r2h, shift, 0, np.arange(H))
    return int((cx1 - cx0 + 1).max() * (cy1 - cy0 + 1).max())


def coverage(W, H, r2h, shift, xy, valid, jlog, pts, nearest_log, accept_log, parent):
    """Counts over the iterations i with valid[i] and a snapshot of more than 64 vertices (jlog[i] = tree size before i, which
    is also the index an accepted sample gets):
      post_tiny   such iterations
      reach       ... whose box has more than 64 cells, one of them at position >= 64 unculled and occupied
      nearest     ... whose nearest vertex sits in such a cell
      parent      accepted ones whose chosen parent sits in such a cell
      max_box     the largest box met"""
    out = dict(post_tiny=0, reach=0, nearest=0, parent=0, max_box=0)
    xy = np.asarray(xy, dtype=np.int64)
    pts = np.asarray(pts, dtype=np.int64)
    jl = np.asarray(jlog, dtype=np.int64)
    it = np.flatnonzero(np.asarray(valid, dtype=bool) & (jl > TINY))
    out["post_tiny"] = int(it.size)
    if it.size == 0 or r2h <= 0:
        return out
    x, y, j = xy[it, 0], xy[it, 1], jl[it]
    cx0, cx1, cy0, cy1 = box_cells(W, H, r2h, shift, x, y)
    nx, ny = cx1 - cx0 + 1, cy1 - cy0 + 1
    out["max_box"] = int((nx * ny).max())
    ncy = (H + (1 << shift) - 1) >> shift
    ncx = (W + (1 << shift) - 1) >> shift
    jmax = int(jl.max()) + 1
    cid = (pts[:jmax, 0] >> shift) * ncy + (pts[:jmax, 1] >> shift)
    first_in = np.full(ncx * ncy, np.iinfo(np.int64).max)
    np.minimum.at(first_in, cid, np.arange(jmax))
    # every cell of every box: [iteration, column of the box, row of the box]
    dx, dy = np.arange(int(nx.max()))[None, :, None], np.arange(int(ny.max()))[None, None, :]
    inside = (dx < nx[:, None, None]) & (dy < ny[:, None, None])
    cx, cy = cx0[:, None, None] + dx, cy0[:, None, None] + dy
    pos = dx * ny[:, None, None] + dy
    d2 = farnn._cell_d2(x[:, None, None], y[:, None, None], cx, cy, shift)
    cell = np.where(inside, cx * ncy + cy, 0)
    late = inside & (pos >= SLAB) & (d2 < r2h) & (first_in[cell] < j[:, None, None])
    reach = late.any(axis=(1, 2))
    out["reach"] = int(reach.sum())

    def in_late_cell(v):  # vertex v[k] of iteration it[k] sits in a late cell of that iteration's box
        vx, vy = pts[v, 0] >> shift, pts[v, 1] >> shift
        ok = (vx >= cx0) & (vx <= cx1) & (vy >= cy0) & (vy <= cy1)
        p = (vx - cx0) * ny + (vy - cy0)
        return ok & (p >= SLAB) & (farnn._cell_d2(x, y, vx, vy, shift) < r2h)

    nl = np.asarray(nearest_log, dtype=np.int64)[it]
    out["nearest"] = int((in_late_cell(np.maximum(nl, 0)) & (nl >= 0)).sum())
    acc = np.asarray(accept_log)[it] != 0
    par = np.asarray(parent, dtype=np.int64)[np.minimum(j, len(parent) - 1)]
    acc &= par >= 0
    out["parent"] = int((in_late_cell(np.maximum(par, 0)) & acc).sum())
    return out


def meets_floor(cov):
    """The floor of every slab case: at least 1 % of the post-tiny iterations reach a later slab, and at least one accepted
    vertex takes its parent from a later-slab cell."""
    return cov["post_tiny"] > 0 and 100 * cov["reach"] >= cov["post_tiny"] and cov["parent"] >= 1


# ------------------------------------------------------------------------------------------------------------ cases
# The radii of the GPU tests that ran the team and block kernels before this module existed (grid, r_rewire): all of them stay
# within one slab on divisor 2 cells.
OLD_RADII = [(2048, 200.5), (1024, 48), (300, 70), (512, 40), (1024, 64), (2048, 64), (512, 30), (96, 30)]
LATE_RADII = [(1024, 60), (1024, 120), (1024, 127), (1024, 255)]

# group 1: one query per case, every kernel.  alg 1 = RRT*, 2 = Informed RRT*.
SLAB_CASES = [
    dict(id="star_r60", W=1024, H=1024, gseed=1, alg=1, rr=60, rg=None, n=9000, seed=0, pair=7),
    dict(id="star_r120", W=1024, H=1024, gseed=1, alg=1, rr=120, rg=None, n=9000, seed=1, pair=7),
    dict(id="star_r127.5", W=1024, H=1024, gseed=1, alg=1, rr=127.5, rg=None, n=9000, seed=2, pair=7),
    dict(id="star_r255_2048", W=2048, H=2048, gseed=3, alg=1, rr=255, rg=None, n=9000, seed=5, pair=11),
    dict(id="informed_r120", W=1024, H=1024, gseed=1, alg=2, rr=120, rg=12, n=9000, seed=0, pair=7),
    # nx != ny, boxes clamped at two edges (a height of 200 would cap the box at 9 x 7 = 63 cells of 32 pixels: one slab)
    dict(id="rect700x300_r120", W=700, H=300, gseed=2, alg=1, rr=120, rg=None, n=9000, seed=3, pair=5),
]

# group 2: Dubins-RRT* near sets (divisor 2 cells as well)
DUBINS_SLAB_CASES = [
    dict(id="dubins_r60", grid=1024, n=9000, rr=60, rho=6.0, seed=1),
    dict(id="dubins_r120", grid=1024, n=9000, rr=120, rho=8.0, seed=2),
]

_grids, _runs = {}, {}


def grid_of(W, H, gseed):
    key = (W, H, gseed)
    if key not in _grids:
        og = perlin_occupancygrid(W, H, seed=gseed)
        _grids[key] = (og, oracle.og_u8(og))
    return _grids[key]


def iteration_points(samples, ro, n):
    """(xy, valid): the point iteration i looked at.  Up to i_switch it is samples[i]; an Informed query draws the later ones from
    its ellipse, and those are known only where they were accepted (they are then the vertex jlog[i])."""
    xy = np.array(samples, dtype=np.int64)
    valid = np.ones(n, dtype=bool)
    sw = int(getattr(ro, "i_switch", n))
    if sw < n:
        acc = np.asarray(ro.accept_log)[sw:] != 0
        idx = np.asarray(ro.jlog, dtype=np.int64)[sw:]
        xy[sw:][acc] = np.asarray(ro.pts, dtype=np.int64)[idx[acc]]
        valid[sw:] = acc
    return xy, valid


def run_query(og8, alg, n, xs, xg, samples, rng, rr, rg):
    """The oracle's run of one query, through the unit-ball hand-over for an Informed one (rng: the generator that drew
    `samples`).  Returns (status, result, r2, unitball or None)."""
    r2 = hostprep.radius_threshold(rr) if rr is not None else 0
    Cm = hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64)) if alg == 2 else None
    kw = dict(r2_rewire=r2, r_goal=rg or 0.0, Cmat=Cm)
    st, ro = oracle.plan(og8, n, alg, xs, xg, samples, **kw)
    ub = None
    if st == oracle.ORC_NEED_UNITBALL:
        ub = hostprep.draw_unitball(rng, n - ro.i_switch)
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, unitball=ub, ub_offset=ro.i_switch, **kw)
    return st, ro, r2, ub


def query_coverage(W, H, r2, shift, samples, ro, n):
    xy, valid = iteration_points(samples, ro, n)
    return coverage(W, H, r2, shift, xy, valid, ro.jlog, ro.pts, ro.nearest_log, ro.accept_log, ro.parent)


def slab_case(c):
    """The oracle's run of a group-1 case, once per process: dict(og8, xs, xg, samples, r2, ub, st, ro, cov)"""
    if c["id"] not in _runs:
        og, og8 = grid_of(c["W"], c["H"], c["gseed"])
        xs, xg = random_connected_pair(og, np.random.default_rng(c["pair"]))
        rng = np.random.default_rng(c["seed"])
        samples = hostprep.draw_free_samples(rng, np.argwhere(og8 == 0), c["n"])
        st, ro, r2, ub = run_query(og8, c["alg"], c["n"], xs, xg, samples, rng, c["rr"], c["rg"])
        shift = cell_shift(c["W"], c["H"], r2, DIV_TEAM)
        cov = query_coverage(c["W"], c["H"], r2, shift, samples, ro, c["n"])
        _runs[c["id"]] = dict(og8=og8, xs=xs, xg=xg, samples=samples, r2=r2, ub=ub, st=st, ro=ro, cov=cov, shift=shift)
    return _runs[c["id"]]


def dubins_slab_case(c, nh=64):
    if c["id"] not in _runs:
        og, og8 = grid_of(c["grid"], c["grid"], 1)
        a, b = random_connected_pair(og, np.random.default_rng(11))
        xs, xg = (int(a[0]), int(a[1]), 5), (int(b[0]), int(b[1]), 20)
        rng = np.random.default_rng(c["seed"])
        samples = hostprep.draw_free_samples(rng, np.argwhere(og8 == 0), c["n"])
        heads = rng.integers(0, nh, size=c["n"])
        r2 = hostprep.radius_threshold(c["rr"])
        st, ro = oracle.dubins_plan(og8, c["n"], 1, xs, xg, samples, heads, r2_rewire=r2, rho=c["rho"], nh=nh)
        shift = cell_shift(c["grid"], c["grid"], r2, DIV_TEAM)
        cov = coverage(c["grid"], c["grid"], r2, shift, samples, np.ones(c["n"], dtype=bool), farnn.dubins_jlog(ro), ro.pts,
                       ro.nearest_log, ro.accept_log, ro.parent)
        _runs[c["id"]] = dict(og8=og8, xs=xs, xg=xg, samples=samples, heads=heads, r2=r2, st=st, ro=ro, cov=cov, shift=shift)
    return _runs[c["id"]]


# ---------------------------------------------------------------------------------------------- batches (groups 3 and 4)
def batch_queries(key, W, H, gseed, specs, pair_seed, div):
    """The queries of a batch and their oracle runs, once per process.  specs: one dict(alg, rr, n, seed) per query (rg for an
    Informed one).  Returns (og8, [dict(alg, n, xs, xg, samples, rng0, r2, rg, st, ro, ub, cov, shifts)]); cov is taken on the
    cells of divisor `div`, for the queries whose box on those cells can exceed a slab (None otherwise, and for Informed)."""
    if key not in _runs:
        og, og8 = grid_of(W, H, gseed)
        free = np.argwhere(og8 == 0)
        sg = np.random.default_rng(pair_seed)
        out = []
        for s in specs:
            xs, xg = random_connected_pair(og, sg)
            rng = np.random.default_rng(s["seed"])
            samples = hostprep.draw_free_samples(rng, free, s["n"])
            d = dict(alg=s["alg"], n=s["n"], xs=xs, xg=xg, samples=samples, rr=s.get("rr"), rg=s.get("rg"), cov=None)
            d["r2"] = hostprep.radius_threshold(s["rr"]) if s["alg"] else 0
            d["shifts"] = shift_pair(W, H, d["r2"])
            if s["alg"] == 2:
                d["rng"] = rng  # (continues with the unit-ball draws once the device names i_switch)
                d["st"] = d["ro"] = None
            else:
                d["st"], d["ro"], _, _ = run_query(og8, s["alg"], s["n"], xs, xg, samples, rng, s["rr"] if s["alg"] else None, None)
                shift = cell_shift(W, H, d["r2"], div)
                if s["alg"] == 1 and largest_box(W, H, d["r2"], shift) > SLAB:
                    d["cov"] = query_coverage(W, H, d["r2"], shift, samples, d["ro"], s["n"])
            out.append(d)
        _runs[key] = (og8, out)
    return _runs[key]


# (a) one CU per query with an Informed query among them: the block kernel on the pipeline's (divisor 4) cells
XGEO_A = dict(W=1024, H=1024, gseed=1, pair=41, n=8000, specs=[
    dict(alg=1, rr=64, n=8000, seed=700), dict(alg=2, rr=100, rg=12, n=8000, seed=701), dict(alg=1, rr=100, n=8000, seed=702),
    dict(alg=1, rr=127.5, n=8000, seed=703), dict(alg=0, rr=None, n=8000, seed=704), dict(alg=1, rr=127.5, n=7777, seed=705),
    dict(alg=1, rr=64, n=8000, seed=706)])
# (b) 100 queries, an Informed one among them: the unpipelined team of two on divisor 4 cells (n and the start / goal draws
# chosen so that every RRT* query meets the floor: at r_rewire = 70 few parents come from the far columns of the box)
XGEO_B = dict(W=300, H=260, gseed=6, pair=13, n=2000,
              specs=[dict(alg=2 if q == 7 else q % 2, rr=70 if q % 4 == 1 else 100, rg=5, n=2000, seed=2000 + q) for q in range(100)])
# (c) a default-team batch that finds every CU claimed: the one-CU pipeline on divisor 2 cells
XGEO_C = dict(W=1024, H=1024, gseed=1, pair=43, n=8000, specs=[
    dict(alg=1, rr=64, n=8000, seed=800), dict(alg=1, rr=127.5, n=8000, seed=801), dict(alg=1, rr=64, n=6000, seed=802),
    dict(alg=1, rr=127.5, n=8000, seed=803)])


# ------------------------------------------------------------------------------------------------ the cases on a device batch
def same_as_oracle(res, st, ro, tag, logs=True, rewire=False):
    """the comparison of devcheck.oracle_vs_device (rewire: that of test_rewire._device_vs_oracle_rewire, which has the
    rewire counts in place of the tree-size log and the three sums)"""
    live = ro.j + (1 if ro.found else 0)
    assert res.status == st and res.j == ro.j and res.found == ro.found and res.vgoal == ro.vgoal and res.i_switch == ro.i_switch, tag
    if logs:
        assert np.array_equal(res.nearest_log, ro.nearest_log), tag
        assert np.array_equal(res.accept_log, ro.accept_log), tag
        assert rewire or np.array_equal(res.j_log, ro.jlog), tag
        assert np.array_equal(res.cbest_log, ro.cbest_log, equal_nan=True), tag
    assert np.array_equal(res.pts[:live], ro.pts[:live]), tag
    assert np.array_equal(res.parent[:live], ro.parent[:live]), tag
    assert np.array_equal(res.vcost[:live], ro.vcost[:live]), tag
    if rewire:
        assert (res.n_rewired, res.n_propagated) == (ro.n_rewired, ro.n_propagated), tag
    else:
        assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near, tag


def query_of(alg, n, xs, xg, samples, r2, rg):
    kw = {}
    if alg == 2:
        kw = dict(goal_d2=hostprep.goal_threshold(rg), Cmat=hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64)))
    return _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2, **kw)


def hand_over_unitballs(b, qs, tag):
    """The queries of a launched batch whose oracle run took the unit-ball hand-over (d["ub"]): each must wait at the oracle's
    i_switch; every one gets its stream and the batch is launched again.  Returns how many there were."""
    waiting = 0
    for q, d in enumerate(qs):
        if d.get("ub") is None:
            continue
        r = b.get_result(q, arrays=False)
        assert r.c.status == _ffi.RRT_NEED_UNITBALL and r.c.i_switch == d["ro"].i_switch, (tag, q)
        b.set_unitball(q, d["ub"], r.c.i_switch)
        waiting += 1
    if waiting:
        b.launch()
        b.sync()
    return waiting


def fill_batch(b, qs):
    keep = []
    for q, d in enumerate(qs):
        qu, k = query_of(d["alg"], d["n"], d["xs"], d["xg"], d["samples"], d["r2"], d["rg"])
        keep.append(k)
        b.set_query(q, qu)
    return keep
