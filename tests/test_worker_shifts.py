"""GPU: a single RRTStandard / RRT* query with no cap on its team runs two shifts of 64 workers next to one committer -- members
1 .. 64 resolve blocks 1, 3, 5, ..., members 65 .. 128 blocks 2, 4, 6, ... -- on the same kernel pair as the team of 64 + 1
(rrt_block_commit_kernel + rrt_block_work_kernel<64, 1, false>).  Which tree a block is resolved against does not change, so
trees, parents and f64 costs must be the oracle's bit for bit, whatever the number of blocks; an explicit team=64 is the
one-shift shape of before, and whatever does not fit two shifts (two queries, a second batch in flight, an Informed query) runs
as it did."""
import numpy as np
import pytest

import oracle
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pairs
from treecalls import ONE_SHIFT, TWO_SHIFTS

pytestmark = pytest.mark.gpu

N_MAX = 12000

_cache = {}


def _grid():
    if "grid" not in _cache:
        og = perlin_occupancygrid(1024, 1024, thresh=0.33, seed=1)  # bench.py's grid
        _cache["grid"] = (og, hostprep.og_nonzero(og), np.argwhere(og == 0), random_connected_pairs(og, np.random.default_rng(7), 3))
    return _cache["grid"]


def _query(q, n, alg=1):
    """query q of the three (start / goal pair q, sample stream q) cut to n samples, and what the oracle makes of it (computed once)"""
    og, og8, free, pairs = _grid()
    if ("samples", q) not in _cache:
        _cache[("samples", q)] = hostprep.draw_free_samples(np.random.default_rng(q), free, N_MAX)
    samples = _cache[("samples", q)][:n]
    xs, xg = pairs[q]
    r2 = hostprep.radius_threshold(64) if alg != 0 else 0
    if ("oracle", q, n, alg) not in _cache:
        _cache[("oracle", q, n, alg)] = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, logs=False)
    qu, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2)
    return qu, keep, _cache[("oracle", q, n, alg)]


def _results(b, Q):
    out = []
    for q in range(Q):
        r = b.get_result(q)
        live = r.j + (1 if r.found else 0)
        out.append((r.status, r.j, r.vgoal, r.found, r.pts[:live].copy(), r.parent[:live].copy(), r.vcost[:live].copy()))
    return out


def _launch(b):
    b.rearm()
    b.launch()
    b.sync()


def _equal(a, b):
    return a[:4] == b[:4] and all(np.array_equal(x, y) for x, y in zip(a[4:], b[4:]))


def _same_as_oracle(got, st_ro, tag):
    st, ro = st_ro
    status, j, vgoal, found, pts, parent, vcost = got
    live = ro.j + (1 if ro.found else 0)
    assert status == st and j == ro.j and vgoal == ro.vgoal and found == ro.found, tag
    assert np.array_equal(pts, ro.pts[:live]) and np.array_equal(parent, ro.parent[:live]), tag
    assert np.array_equal(vcost, ro.vcost[:live]), tag  # bit-exact f64


def _no_timeouts(b, shrunk=0):
    info = b.team_info()
    assert b.team()[1] == 0 and info["timeouts"] == 0, info
    if shrunk is not None:
        assert info["shrunk"] == shrunk, info


@pytest.mark.parametrize("alg", [1, 0], ids=["star", "std"])
def test_default_single_query_runs_two_shifts_twice(gpu_ctx, alg):
    og, og8, _, _ = _grid()
    gpu_ctx.set_grid(og8)
    n = N_MAX
    qu, keep, ref = _query(0, n, alg)
    b = _ffi.Batch(gpu_ctx, 1, n)
    b.set_query(0, qu)
    runs = []
    for _ in range(2):
        _launch(b)
        runs.append(_results(b, 1))
    assert b.kernel_name() == TWO_SHIFTS and b.kernel_name().endswith(" in 2 shifts"), b.kernel_name()
    assert b.team()[0] == 128 and b.team_info()["last"] == 128 and b.pipelined()
    _no_timeouts(b)
    _same_as_oracle(runs[0][0], ref, "first launch")
    assert _equal(runs[1][0], runs[0][0])
    b.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 128, 129, 191, 192, 193, 257])
def test_block_count_edges(gpu_ctx, n):
    """one block (the second shift never resolves), one block per shift, odd and even block counts, a short last block on either shift"""
    og, og8, _, _ = _grid()
    gpu_ctx.set_grid(og8)
    qu, keep, ref = _query(0, n)
    b = _ffi.Batch(gpu_ctx, 1, n)
    b.set_query(0, qu)
    _launch(b)
    assert b.kernel_name() == TWO_SHIFTS and b.team()[0] == 128, (b.kernel_name(), b.team())
    _no_timeouts(b)
    _same_as_oracle(_results(b, 1)[0], ref, n)
    b.close()


def test_two_shifts_equal_one_shift(gpu_ctx):
    """three queries, one at a time: the default against team=64, every array identical; team=64 is exactly the shape it was"""
    og, og8, _, _ = _grid()
    gpu_ctx.set_grid(og8)
    n = 9000
    for q in range(3):
        qu, keep, ref = _query(q, n)
        got = {}
        for team in (None, 64):
            b = _ffi.Batch(gpu_ctx, 1, n, team=team)
            b.set_query(0, qu)
            _launch(b)
            got[team] = _results(b, 1)[0]
            if team == 64:
                assert b.kernel_name() == ONE_SHIFT and b.team() == (64, 0), (b.kernel_name(), b.team())
                assert b.team_info() == dict(created=64, last=64, timeouts=0, shrunk=0)
            else:
                assert b.kernel_name() == TWO_SHIFTS and b.team() == (128, 0), (b.kernel_name(), b.team())
            _no_timeouts(b)
            b.close()
        assert _equal(got[None], got[64]), q
        _same_as_oracle(got[None], ref, q)


def test_a_batch_of_two_queries_keeps_one_shift(gpu_ctx):
    """2 x 129 compute units are more than the device has: 64 + 1 per query, one shift"""
    og, og8, _, _ = _grid()
    gpu_ctx.set_grid(og8)
    n = 6000
    qs = [_query(q, n) for q in range(2)]
    b = _ffi.Batch(gpu_ctx, 2, n)
    for q, (qu, keep, ref) in enumerate(qs):
        b.set_query(q, qu)
    _launch(b)
    assert b.kernel_name() == ONE_SHIFT and b.team()[0] == 64 and b.team_info()["last"] == 64, (b.kernel_name(), b.team_info())
    _no_timeouts(b)
    out = _results(b, 2)
    for q, (qu, keep, ref) in enumerate(qs):
        _same_as_oracle(out[q], ref, q)
    b.close()


def test_two_single_query_batches_in_flight(gpu_ctx):
    """The first launch claims 129 compute units; the second batch (a context of its own) gets whatever fits next to them and says so
    in `shrunk`.  Nothing depends on timing: a claim lasts until its batch is synchronised."""
    og, og8, _, _ = _grid()
    gpu_ctx.set_grid(og8)
    ctx2 = _ffi.Context(0)
    ctx2.set_grid(og8)
    n = 6000
    qa, keep_a, ref_a = _query(0, n)
    qb, keep_b, ref_b = _query(1, n)
    a = _ffi.Batch(gpu_ctx, 1, n)
    b = _ffi.Batch(ctx2, 1, n)
    a.set_query(0, qa)
    b.set_query(0, qb)
    a.rearm()
    b.rearm()
    a.launch()
    b.launch()
    a.sync()
    b.sync()
    assert a.kernel_name() == TWO_SHIFTS and a.team_info()["last"] == 128
    _no_timeouts(a)
    info = b.team_info()
    assert info["created"] == 128 and info["last"] < 128 and info["shrunk"] == 1, info
    _no_timeouts(b, shrunk=None)
    _same_as_oracle(_results(a, 1)[0], ref_a, "first batch")
    _same_as_oracle(_results(b, 1)[0], ref_b, "second batch")
    a.close()
    b.close()
    ctx2.close()


def test_an_informed_single_query_keeps_the_one_body_kernel(gpu_ctx):
    """An Informed query alone in a default batch: the one-body kernel on 64 + 1 in one shift, on a batch whose spill area has room
    for two shifts.  The run stops for its unit-ball samples, gets them and goes on; status, tree, parents and costs are the
    oracle's on the same streams."""
    og, og8, free, pairs = _grid()
    gpu_ctx.set_grid(og8)
    n = 3000
    xs, xg = pairs[0]
    rng = np.random.default_rng(0)
    samples = hostprep.draw_free_samples(rng, free, n)
    r2 = hostprep.radius_threshold(64)
    Cm = hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64))
    qu, keep = _ffi.make_query(2, n, xs, xg, samples, r2_rewire=r2, goal_d2=hostprep.goal_threshold(12), Cmat=Cm)
    b = _ffi.Batch(gpu_ctx, 1, n)
    b.set_query(0, qu)
    _launch(b)
    name = b.kernel_name()
    assert name == "rrt_expand_block_kernel<64, 1, true, true>" and b.team() == (64, 0), (name, b.team())
    assert b.team_info() == dict(created=64, last=64, timeouts=0, shrunk=0)
    kw = {}
    st0, ro0 = oracle.plan(og8, n, 2, xs, xg, samples, r2_rewire=r2, r_goal=12.0, Cmat=Cm)
    r = b.get_result(0, arrays=False)
    assert r.c.status == st0 and r.c.i_switch == ro0.i_switch, (r.c.status, st0, r.c.i_switch, ro0.i_switch)
    if r.c.status == _ffi.RRT_NEED_UNITBALL:  # the generator stands right behind the free draws
        ub = hostprep.draw_unitball(rng, n - r.c.i_switch)
        kw = dict(unitball=ub, ub_offset=r.c.i_switch)
        b.set_unitball(0, ub, r.c.i_switch)
        b.launch()
        b.sync()
        assert b.kernel_name() == name and b.team_info()["last"] == 64
    _no_timeouts(b)
    _same_as_oracle(_results(b, 1)[0], oracle.plan(og8, n, 2, xs, xg, samples, r2_rewire=r2, r_goal=12.0, Cmat=Cm, **kw), "Informed")
    b.close()
