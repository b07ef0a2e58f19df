"""GPU: one RRTStandard / RRT* query on the committer + worker pair of 64, in two shifts (a batch without a cap: members 1 .. 64 take
blocks 1, 3, 5, ..., members 65 .. 128 blocks 2, 4, 6, ...) and in one (team=64), off the fresh plan: launches that start in the
middle of a stream (grow, reroot, relax), the same batch launched again with another number of blocks and across an Informed
query, go2goal folded across the shifts on small trees, unseen goals and exact ties, the maps and radii that have broken kernels
before, and a team that loses its member 1.

Every case runs on both shapes.  Each run asserts the kernel's name exactly and that no hand-off timed out (except in the last
section, where one must), and compares pts, parent, vcost (as raw bits), nearest_log, accept_log, j_log, cbest_log, sum_j, sum_near
and sum_cells_nn with the host reference; and the two shapes must agree bit for bit.  tests/test_shift_pair_cpu.py holds the cases
(tests/shiftcases.py) to what they are for.

Not repeated here, because with the names of devcheck.KERNELS they assert the name exactly: the slab radii 60 ... 255 of
tests/test_record_slabs.py (`test_slab_radii_on_every_kernel[*-team]` and `[*-team64]`).  tests/test_far_nearest.py goes through
Context.plan, which cannot name its kernel, so its pocket cases run here through the Batch twin."""
import numpy as np
import pytest

import farnn
import oracle
import relaxcases as rc
import shiftcases as sc
import treecalls as tc
from devcheck import KERNEL_ARGS, oracle_vs_batch, same_as_oracle_with_logs
from orchelp import differ
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pair

pytestmark = pytest.mark.gpu

ARRAYS = ("pts", "parent", "vcost", "nearest_log", "accept_log", "j_log", "cbest_log")


def _batch(ctx, shape, n_cap, **kw):
    return _ffi.Batch(ctx, 1, n_cap, logs=True, **KERNEL_ARGS[shape], **kw)


def _ran(b, shape, timeouts=0):
    """the last launch ran this shape's kernel, by its exact name, on all its workers, and no hand-off timed out"""
    name, workers = sc.PAIR[shape]
    info = b.team_info()
    assert b.kernel_name() == name, (shape, b.kernel_name())
    assert b.team() == (workers, 0) and info == dict(created=workers, last=workers, timeouts=timeouts, shrunk=0), (shape, b.team(), info)


def _bits(res, rows, log_rows):
    """what the two shapes must agree on bit for bit: status and counts, the live rows of the tree, the log rows, the statistics"""
    head = (res.status, res.j, res.found, res.vgoal, res.i_switch, res.sum_j, res.sum_near, res.sum_cells_nn)
    out = [np.asarray(getattr(res, a))[:rows].copy() for a in ARRAYS[:3]] + [np.asarray(getattr(res, a))[log_rows].copy() for a in ARRAYS[3:]]
    out[2], out[6] = out[2].view(np.int64), out[6].view(np.int64)  # costs as raw bits
    return head, out


def _same_bits(got):
    (ha, a), (hb, b) = got["team"], got["team64"]
    assert ha == hb, (ha, hb)
    for name, x, y in zip(ARRAYS, a, b):
        assert np.array_equal(x, y), (name, differ(x, y))


def _launch(b):
    b.launch()
    b.sync()


def _plan(b, c, n=None):
    """the query of case c set, armed and launched on batch b; the result"""
    qu, keep = _ffi.make_query(c["alg"], c["n"], c["xs"], c["xg"], c["samples"], r2_rewire=c["r2"])
    b.set_query(0, qu)
    b.rearm()
    _launch(b)
    return b.get_result(0)


def _grown_checked(b, res, g, log0, og2, samples, shape):
    """the result of a launched grow / reroot / relax against its restatement g: tc.same_result, and what it leaves out"""
    m = len(samples)
    tc.same_result(res, g, log0)
    assert res.sum_cells_nn == sc.cells_nn(og2, g.pts, g.nearest_log, samples), res.sum_cells_nn
    assert np.isnan(res.cbest_log[log0:log0 + m]).all()  # (the ellipse cost of an iteration: NaN when the sample was drawn freely)
    _ran(b, shape)
    return _bits(res, g.j + g.found, slice(log0, log0 + m))


# ------------------------------------------------------------------------------------------------ a. mid-stream starts
def _kept_seed(ctx, shape, which):
    """the base query planned on a batch of this shape and kept on the seed's map: (batch, tree of the plan)"""
    c, d = tc.base(), sc.seed_case(which)
    ctx.set_grid(c["og8"])
    b = _batch(ctx, shape, c["n"])
    r0 = _plan(b, c)
    assert r0.j == c["ro"].j and np.array_equal(r0.vcost[:r0.j].view(np.int64), c["ro"].vcost[:r0.j].view(np.int64))
    _ran(b, shape)
    ctx.set_grid(d["og2"])
    assert np.array_equal(b.keep_tree(0), d["alive"])
    return b, tc.tree_of(r0)


@pytest.mark.parametrize("m", sc.GROW_M)
@pytest.mark.parametrize("which", ["aligned", "wall"])
def test_a_grow_that_starts_mid_stream(gpu_ctx, which, m):
    """The launch is armed at iteration j0 (a multiple of 64, or 775): block 1 of the launch is [j0, j0 + 64), so m samples are
    sc.GROW_BLOCKS[m] blocks: one short block (the second shift resolves nothing), exactly one, a second-shift block of one sample,
    the short last block on either shift.  The stream holds cells of vertices, blocked cells, repeated samples and a run of rejected
    samples over a whole block, after which the state slot a worker reads is what it was an epoch earlier."""
    d, g = sc.seed_case(which), sc.grown(which, m)
    samples = d["samples"][:m]
    got = {}
    for shape in sc.PAIR:
        b, prev = _kept_seed(gpu_ctx, shape, which)
        j0, old_id, log0 = b.grow(0, samples)
        assert j0 == len(d["ids"]) == log0 == g.j0 and np.array_equal(old_id, d["ids"])
        _launch(b)
        got[shape] = _grown_checked(b, b.get_result(0), g, log0, d["og2"], samples, shape)
        b.close()
    _same_bits(got)


@pytest.mark.parametrize("m", sc.SEED_M)
def test_a_reroot_that_starts_mid_stream(gpu_ctx, m):
    d = sc.seed_case("wall")
    R, g = sc.rerooted(m)
    samples = d["samples"][:m]
    got = {}
    for shape in sc.PAIR:
        b, prev = _kept_seed(gpu_ctx, shape, "wall")
        j0, old_id, log0 = b.reroot(0, sc.reroot_vertex(), samples)
        assert j0 == len(R.ids) == log0 and np.array_equal(old_id, R.ids)
        _launch(b)
        res = b.get_result(0)
        assert np.array_equal(res.pts[0], prev[0][sc.reroot_vertex()]) and res.vcost[0] == 0.0 and res.parent[0] == -1
        got[shape] = _grown_checked(b, res, g, log0, d["og2"], samples, shape)
        b.close()
    _same_bits(got)


@pytest.mark.parametrize("m", sc.SEED_M)
def test_a_relax_that_starts_mid_stream(gpu_ctx, m):
    d = sc.seed_case("wall")
    X, g = sc.relaxed(m)
    samples = d["samples"][:m]
    got = {}
    for shape in sc.PAIR:
        b, prev = _kept_seed(gpu_ctx, shape, "wall")
        j0, old_id, log0 = b.relax(0, rc.R_of(tc.RR), samples)
        assert j0 == len(X.ids) == log0 and np.array_equal(old_id, X.ids) and b.relax_stats()["fell"] == X.fell
        _launch(b)
        got[shape] = _grown_checked(b, b.get_result(0), g, log0, d["og2"], samples, shape)
        b.close()
    _same_bits(got)


def test_a_grow_whose_second_block_is_far_heavier_than_the_first(gpu_ctx):
    """sc.late_case(): block 1 of the grow is 64 cells of vertices, none accepted; block 2, the second shift's first, is 64 free
    draws with near sets of a thousand vertices and more, on a seed of 9000 vertices that crosses a scan chunk, on a batch whose
    launch before (the plan) left FINAL in every flag of the second shift."""
    d = sc.late_case()
    g, more = d["grown"], d["more"]
    gpu_ctx.set_grid(d["og8"])
    got = {}
    for shape in sc.PAIR:
        b = _batch(gpu_ctx, shape, d["n"])
        r0 = _plan(b, d)
        assert r0.j == d["ro"].j and np.array_equal(r0.vcost[:r0.j].view(np.int64), d["ro"].vcost[:r0.j].view(np.int64))
        _ran(b, shape)
        j0, old_id, log0 = b.grow(0, more)
        assert j0 == g.j0 == log0 and np.array_equal(old_id, np.arange(j0))
        _launch(b)
        got[shape] = _grown_checked(b, b.get_result(0), g, log0, d["og8"], more, shape)
        b.close()
    _same_bits(got)


# ------------------------------------------------------------------------------------------------ b. the same batch again
def _planned_checked(b, c, shape):
    res = _plan(b, c)
    st, ro = c["plan"]
    same_as_oracle_with_logs(res.status, res, st, ro)
    assert np.array_equal(res.vcost[:ro.j + ro.found].view(np.int64), ro.vcost[:ro.j + ro.found].view(np.int64))
    _ran(b, shape)
    return _bits(res, ro.j + ro.found, slice(0, c["n"]))


def test_one_batch_launched_again_with_another_block_count(gpu_ctx):
    """set_query + rearm + launch with n = 257, 65, 1, 129, 64, 193, 2 on one batch of capacity 300: 5, 2, 1, 3, 1, 4, 1 blocks.
    Whatever a launch leaves in the second shift's arrival flags and go2goal answers, in the record and state slots or at the FINAL
    epoch must not reach the next: each run is the oracle's plan of its own stream, every log included."""
    gpu_ctx.set_grid(tc.base()["og8"])
    got = {shape: [] for shape in sc.PAIR}
    for shape in sc.PAIR:
        b = _batch(gpu_ctx, shape, sc.RELAUNCH_CAP)
        for n in sc.RELAUNCH_NS:
            got[shape].append(_planned_checked(b, sc.relaunch(n), shape))
        b.close()
    for k in range(len(sc.RELAUNCH_NS)):
        _same_bits({shape: got[shape][k] for shape in sc.PAIR})


def test_an_informed_query_between_two_launches_of_an_rrtstar_query(gpu_ctx):
    """set_query flips the batch to one shift for an Informed query and back: the RRT* query runs the pair (in two shifts on the
    batch without a cap), the Informed one the one-body kernel on 64 + 1 through the unit-ball hand-over, the RRT* query again the
    pair, with the result it had."""
    c = tc.base()
    gpu_ctx.set_grid(c["og8"])
    star, inf = sc.relaunch(sc.INFORMED_N), sc.informed()
    got = {}
    for shape in sc.PAIR:
        b = _batch(gpu_ctx, shape, sc.INFORMED_N)
        first = _planned_checked(b, star, shape)
        qu, keep = _ffi.make_query(2, inf["n"], c["xs"], c["xg"], inf["samples"], r2_rewire=c["r2"], goal_d2=hostprep.goal_threshold(sc.INFORMED_RG), Cmat=inf["Cmat"])
        b.set_query(0, qu)
        b.rearm()
        _launch(b)
        r = b.get_result(0)
        st0, ro0 = inf["first"]
        assert r.status == st0 == _ffi.RRT_NEED_UNITBALL and r.i_switch == ro0.i_switch
        assert b.kernel_name() == sc.INFORMED and b.team() == (64, 0), (b.kernel_name(), b.team())
        b.set_unitball(0, inf["ub"], ro0.i_switch)
        _launch(b)
        r = b.get_result(0)
        same_as_oracle_with_logs(r.status, r, *inf["plan"])
        assert b.kernel_name() == sc.INFORMED and b.team() == (64, 0), (b.kernel_name(), b.team())
        assert b.team_info() == dict(created=64, last=64, timeouts=0, shrunk=0), b.team_info()
        again = _planned_checked(b, star, shape)
        _same_bits({"team": first, "team64": again})  # (the run before the Informed query and the run after it)
        got[shape] = again
        b.close()
    _same_bits(got)


# ------------------------------------------------------------------------------------------------ c. go2goal across the shifts
def _case_checked(ctx, c, shape):
    ctx.set_grid(c["og8"])
    b = _batch(ctx, shape, c["n"])
    out = _planned_checked(b, dict(c, plan=(c["st"], c["ro"])), shape)
    b.close()
    return out


@pytest.mark.parametrize("seen", [True, False], ids=["seen", "unseen"])
@pytest.mark.parametrize("k", sc.SIZED_K)
def test_go2goal_on_trees_of_exactly_k_vertices(gpu_ctx, k, seen):
    """Vertex v is answered for by member v mod 129 (two shifts) or v mod 65 (one): a tree of fewer vertices leaves members with
    no candidate, whose answer (inf, none) the fold must pass over.  A goal that no vertex sees gives the oracle's status and its
    fall-back vgoal = 0."""
    c = sc.sized_case(k, seen)
    _same_bits({shape: _case_checked(gpu_ctx, c, shape) for shape in sc.PAIR})


@pytest.mark.parametrize("which", list(sc.TIES))
def test_go2goal_ties_across_the_shifts(gpu_ctx, which):
    """Two vertices u < v whose keys vcost + dist are equal bit for bit, and cheaper than every other vertex that sees the goal.
    go2goal deals vertex k to member k mod NWG: NWG = 129 workgroups in two shifts (member 0 the committer, 1 .. 64 the first
    shift, 65 .. 128 the second), 65 in one.  Each member answers with its best (cost, index); the committer folds the answers in
    one wave, lane l taking member 1 + l and (two shifts) member 65 + l, the better of the two by (cost, index), then the wave's
    minimum, then its own answer.
      same_lane: u = 5, v = 69 -- members 5 and 69, both read by lane 4 of the fold (one shift: members 5 and 4)
      two_lanes: u = 5, v = 71 -- members 5 and 71, lanes 4 and 6 (one shift: members 5 and 6)
    In both the goal's parent must be u, as in oracle.plan; in neither do the one-shift shape's members hold the pair together."""
    c = sc.tie_case(which)
    got = {shape: _case_checked(gpu_ctx, c, shape) for shape in sc.PAIR}
    u, v = sc.TIES[which]
    for shape in sc.PAIR:
        head, arrays = got[shape]
        assert arrays[1][c["ro"].vgoal] == u, (shape, arrays[1][c["ro"].vgoal])
    _same_bits(got)


# ------------------------------------------------------------------------------------------------ d. maps that break kernels
def _twin_on_both_shapes(ctx, og8, alg, n, seed, xs, xg, rr, rg=None):
    ctx.set_grid(og8)
    cache, got = {}, {}
    for shape in sc.PAIR:
        res, ro, name, info = oracle_vs_batch(ctx, og8, alg, n, seed, xs, xg, rr, rg, kernel=shape, cache=cache)
        want, workers = sc.PAIR[shape] if alg != 2 else (sc.INFORMED, 64)
        assert name == want, (shape, name)
        assert info == dict(created=workers, last=workers, timeouts=0, shrunk=0, team=(workers, 0)), (shape, info)
        got[shape] = _bits(res, ro.j + ro.found, slice(0, n))
    _same_bits(got)


@pytest.mark.parametrize("c", farnn.PIPE_CASES, ids=lambda c: c["id"])
def test_pocket_cases_on_the_named_pair(gpu_ctx, c):
    og8 = farnn.pocket_grid(c["W"], c["H"], c["rects"], c.get("field"))
    _twin_on_both_shapes(gpu_ctx, og8, c["alg"], c["n"], c["seed"], c["xs"], c["xg"], c["rr"])


def test_a_strip_map_of_300_by_260(gpu_ctx):
    S = sc.STRIP
    _twin_on_both_shapes(gpu_ctx, sc.strip_grid(), 1, S["n"], S["seed"], S["xs"], S["xg"], S["rr"])


# ---- the team and team64 cases of the four KERNELS_NOFAULT tests of tests/test_gpu_parity.py, through the twin that names its kernel
def test_beyond_lds_capacity_on_the_named_pair(gpu_ctx):
    og = perlin_occupancygrid(1024, 1024, seed=1)
    xs, xg = random_connected_pair(og, np.random.default_rng(7))
    _twin_on_both_shapes(gpu_ctx, oracle.og_u8(og), 1, 40000, 0, xs, xg, 64)


def test_near_set_spills_on_the_named_pair(gpu_ctx):
    og = perlin_occupancygrid(256, 256, seed=4)
    xs, xg = random_connected_pair(og, np.random.default_rng(1))
    _twin_on_both_shapes(gpu_ctx, oracle.og_u8(og), 1, 5000, 3, xs, xg, 1e6)


def test_2048_grid_on_the_named_pair(gpu_ctx):
    og = perlin_occupancygrid(2048, 2048, seed=3)
    og8 = oracle.og_u8(og)
    xs, xg = random_connected_pair(og, np.random.default_rng(11))
    _twin_on_both_shapes(gpu_ctx, og8, 1, 30000, 5, xs, xg, 64)
    assert og8[3, 2044] == 0 and og8[2040, 5] == 0
    _twin_on_both_shapes(gpu_ctx, og8, 2, 12000, 6, (3, 2044), (2040, 5), 200.5, 40)


def test_fuzz_small_queries_on_the_named_pair(gpu_ctx):
    """the 600 queries of test_fuzz_small_queries_vs_oracle, drawn the same way"""
    rng = np.random.default_rng(20260101)
    ran = 0
    for case in range(600):
        w, h = int(rng.integers(8, 70)), int(rng.integers(8, 70))
        dens = rng.choice([0.0, 0.1, 0.3, 0.5])
        og8 = (rng.uniform(size=(w, h)) < dens).astype(np.uint8)
        if case % 3 == 0:
            og8 = oracle.og_u8(perlin_occupancygrid(w, h, seed=case))
        free = np.argwhere(og8 == 0)
        if free.shape[0] < 2:
            continue
        alg = int(rng.integers(0, 3))
        n = int(rng.choice([1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 100, 127, 128, 129, 192, 193, 257, 700, 1500]))
        rr = float(rng.choice([0, 1, 1.5, 3, 7.9, 12, 25, 64, 500]))
        rg = float(rng.choice([0, 1, 2.5, 6, 15, 100]))
        xs = free[rng.integers(0, free.shape[0])] if case % 11 else np.array([int(rng.integers(0, w)), int(rng.integers(0, h))])
        xg = free[rng.integers(0, free.shape[0])]
        if alg == 2 and (xs == xg).all():
            continue
        try:
            _twin_on_both_shapes(gpu_ctx, og8, alg, n, case, xs, xg, rr if alg else None, rg if alg == 2 else None)
        except AssertionError as e:
            raise AssertionError(f"fuzz case {case}: grid {w}x{h} dens {dens} alg {alg} n {n} r {rr} rg {rg} xs {xs} xg {xg}") from e
        ran += 1
    assert ran >= 550


# ------------------------------------------------------------------------------------------------ e. a team that loses member 1
def test_a_team_of_the_pair_that_loses_member_1(gpu_ctx):
    """team_fault makes member 1 return at once.  Every wait of the others ends on the fail flag or on its own half second
    (the two-shifts paragraph): the committer's wait for the arrival flags of block 1 times out and raises the flag, the
    workers' waits for go end on it, and the engine runs the rest on one CU from the block boundary.  So: at least one time-out, the
    oracle's result bit for bit, and the same again from a second launch of the batch."""
    c = sc.fault_case()
    gpu_ctx.set_grid(c["og8"])
    st, ro = c["plan"]
    got = {}
    for shape in sc.PAIR:
        b = _batch(gpu_ctx, shape, c["n"], team_fault=True)
        runs = []
        for launch in range(2):
            res = _plan(b, c)
            same_as_oracle_with_logs(res.status, res, st, ro)
            info = b.team_info()
            workers = sc.PAIR[shape][1]
            assert info["timeouts"] >= 1 and info["created"] == workers and info["last"] == 1 and info["shrunk"] == 0, (shape, info)
            # (the kernel that finished the run: a launch that timed out continues on the block kernel, one CU per query -- tests/variants.py)
            assert b.team() == (workers, info["timeouts"]) and b.kernel_name() == "rrt_expand_block_kernel<1, 16, false, false>", (b.team(), b.kernel_name())
            runs.append(_bits(res, ro.j + ro.found, slice(0, c["n"])))
        _same_bits({"team": runs[0], "team64": runs[1]})  # (the first launch and the second)
        got[shape] = runs[1]
        b.close()
    _same_bits(got)
