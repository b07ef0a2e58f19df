"""GPU: pipelined teams of 8 and more workers run as two kernels -- rrt_block_commit_kernel (one 8-wave workgroup per team) next to
rrt_block_work_kernel on a second stream -- by default; RRT_FLAG_ONEBODY keeps the one-body rrt_expand_block_kernel.  Trees, costs
and parents must be the oracle's bit for bit, the two forms must agree with each other, and launches in a row on the same
buffers must give the same trees."""
import numpy as np
import pytest

import oracle
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pairs
from treecalls import TWO_SHIFTS

pytestmark = pytest.mark.gpu


def _grid(size=1024):
    og = perlin_occupancygrid(size, size, thresh=0.33, seed=1)  # bench.py's grid
    return og, hostprep.og_nonzero(og)


def _queries(og, og8, Q, n, alg=1, r_rewire=64):
    free = np.argwhere(og == 0)
    pairs = random_connected_pairs(og, np.random.default_rng(7), Q)
    r2 = hostprep.radius_threshold(r_rewire) if alg != 0 else 0
    out = []
    for q in range(Q):
        xs, xg = pairs[q]
        samples = hostprep.draw_free_samples(np.random.default_rng(q), free, n)
        qu, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2)
        out.append((qu, keep, xs, xg, samples, r2))
    return out


def _run(ctx, qs, n, launches=1, **kw):
    b = _ffi.Batch(ctx, len(qs), n, **kw)
    for q, (qu, *_rest) in enumerate(qs):
        b.set_query(q, qu)
    runs = []
    for _ in range(launches):
        b.rearm()
        b.launch()
        b.sync()
        out = []
        for q in range(len(qs)):
            r = b.get_result(q)
            live = r.j + (1 if r.found else 0)
            out.append((r.status, r.j, r.vgoal, r.found, r.pts[:live].copy(), r.parent[:live].copy(), r.vcost[:live].copy()))
        runs.append(out)
    name, fallbacks = b.kernel_name(), b.team()[1]
    b.close()
    return runs, name, fallbacks


def _equal(a, b):
    return a[:4] == b[:4] and all(np.array_equal(x, y) for x, y in zip(a[4:], b[4:]))


def _check_oracle(og8, alg, n, qs, out):
    for q, (qu, keep, xs, xg, samples, r2) in enumerate(qs):
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, logs=False)
        status, j, vgoal, found, pts, parent, vcost = out[q]
        live = ro.j + (1 if ro.found else 0)
        assert j == ro.j and vgoal == ro.vgoal and found == ro.found, q
        assert np.array_equal(pts, ro.pts[:live]) and np.array_equal(parent, ro.parent[:live]), q
        assert np.array_equal(vcost, ro.vcost[:live]), q  # bit-exact f64


def test_config2_full_size_split_team_equals_the_oracle_twice(gpu_ctx):
    """BASELINE config 2 (RRT*, 1024^2, n = 50 000) on the default of one query, the committer + worker pair of 64 in two shifts, two
    launches on the same buffers."""
    og, og8 = _grid()
    gpu_ctx.set_grid(og8)
    n = 50000
    qs = _queries(og, og8, 1, n)
    runs, name, fallbacks = _run(gpu_ctx, qs, n, launches=2)
    assert name == TWO_SHIFTS, name
    assert fallbacks == 0
    _check_oracle(og8, 1, n, qs, runs[0])
    assert _equal(runs[1][0], runs[0][0])


@pytest.mark.parametrize("team", [32, 16, 8])
@pytest.mark.parametrize("alg", [1, 0], ids=["star", "std"])
def test_smaller_split_teams_equal_the_oracle(gpu_ctx, team, alg):
    og, og8 = _grid()
    gpu_ctx.set_grid(og8)
    n = 12000
    qs = _queries(og, og8, 1, n, alg=alg)
    runs, name, fallbacks = _run(gpu_ctx, qs, n, launches=2, team=team)
    bsm = 64 // team
    assert name == f"rrt_expand_block_kernel<{team}, {bsm}, true, false> as rrt_block_commit_kernel + rrt_block_work_kernel<{team}, {bsm}, false>"
    assert fallbacks == 0
    _check_oracle(og8, alg, n, qs, runs[0])
    assert _equal(runs[1][0], runs[0][0])


@pytest.mark.parametrize("team", [None, 16, 8])
def test_split_equals_the_one_body_kernel(gpu_ctx, team):
    """The same batch of three queries as two kernels and as one (RRT_FLAG_ONEBODY): every array identical."""
    og, og8 = _grid()
    gpu_ctx.set_grid(og8)
    n = 9000
    qs = _queries(og, og8, 3, n)
    split, sname, sf = _run(gpu_ctx, qs, n, team=team)
    one, oname, of = _run(gpu_ctx, qs, n, team=team, onebody=True)
    assert "rrt_block_commit_kernel" in sname and "rrt_block_commit_kernel" not in oname
    assert sname.startswith(oname)
    assert sf == 0 and of == 0
    for q in range(3):
        assert _equal(split[0][q], one[0][q]), q


def test_informed_batch_keeps_the_one_body_kernel(gpu_ctx):
    og, og8 = _grid()
    gpu_ctx.set_grid(og8)
    n = 3000
    free = np.argwhere(og == 0)
    (xs, xg), = random_connected_pairs(og, np.random.default_rng(7), 1)
    samples = hostprep.draw_free_samples(np.random.default_rng(0), free, n)
    Cm = hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64))
    qu, keep = _ffi.make_query(2, n, xs, xg, samples, r2_rewire=hostprep.radius_threshold(64), goal_d2=hostprep.goal_threshold(12), Cmat=Cm)
    b = _ffi.Batch(gpu_ctx, 1, n)
    b.set_query(0, qu)
    b.rearm()
    b.launch()
    b.sync()
    assert "rrt_block_commit_kernel" not in b.kernel_name() and b.kernel_name().endswith("true, true>")
    b.close()
