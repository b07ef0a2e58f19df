"""GPU: grids up to 4096 x 4096 on the large-grid form of the one-CU pipeline (rrt_pipe_large_kernel, RRT_FLAG_LARGE_GRID).

Everything is compared with the CPU oracle array for array (bit-exact f64 costs), the flag on small grids also with the
reference's goldens.  Grids are built here from rectangles; nothing of that size is committed."""
import numpy as np
import pytest

import farnn
import oracle
import orchelp
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd

pytestmark = pytest.mark.gpu

LARGE_KERNEL = "rrt_pipe_large_kernel"


# ------------------------------------------------------------------------------------------------------------ primitives
def test_wide_sqrt_is_exact_for_every_radicand_below_2_25(gpu_ctx):
    """sqrt_u25 (rrt_device.h) against the host's correctly rounded f64 root, every integer in [0, 2^25)"""
    step = 1 << 22
    for lo in range(0, 1 << 25, step):
        got = gpu_ctx.prim_sqrt_u25(lo, step)
        assert np.array_equal(got, np.sqrt(np.arange(lo, lo + step, dtype=np.float64))), lo
    with pytest.raises(_ffi.RRTError):
        gpu_ctx.prim_sqrt_u25((1 << 25) - 1, 2)
    with pytest.raises(_ffi.RRTError):  # the short one keeps its own limit
        gpu_ctx.prim_sqrt_u24((1 << 24) - 1, 2)


def _rect_map(W, H, seed, count=40):
    rng = np.random.default_rng(seed)
    og8 = np.zeros((W, H), dtype=np.uint8)
    for _ in range(count):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        w, h = int(rng.integers(1, max(2, W // 8))), int(rng.integers(1, max(2, H // 8)))
        og8[x:x + w, y:y + h] = 1
    return og8


def test_large_walk_on_the_device_equals_the_literal_walk():
    """los_wave_large (rrt_line_cell_u26 for long segments, short_line below 64 steps) through rrt_prim_collisionfree_walk against
    the oracle's literal Bresenham walk on 4096 x 4096: free or not, and the number of cells read."""
    W = H = 4096
    og8 = _rect_map(W, H, 5)
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    # the four segments of test_no_size_at_which_the_class_refuses (2600 x 2200), scaled to this grid
    base = np.array([[5, 5, 2599, 2199], [2599, 0, 0, 2199], [0, 1500, 2599, 1501], [1200, 100, 1201, 2100]], dtype=np.float64)
    seg = np.round(base * np.array([4095 / 2599, 4095 / 2199, 4095 / 2599, 4095 / 2199])).astype(np.int32)
    rng = np.random.default_rng(6)
    rnd = rng.integers(0, W, size=(20000, 4)).astype(np.int32)
    near = rnd[:2000].copy()  # some short ones, some of exactly 63 / 64 / 65 steps
    near[:, 2:] = np.clip(near[:, :2] + rng.integers(-70, 71, size=(2000, 2)), 0, W - 1)
    near[:300, 2] = np.clip(near[:300, 0] + np.repeat([63, 64, 65], 100), 0, W - 1)
    seg = np.concatenate([seg, rnd, near])
    free, cells = ctx.prim_collisionfree(seg, walk=_ffi.WALK_U26)
    free_w, cells_w = ctx.prim_collisionfree(seg)  # (what a grid of this size gets by default: the 64-bit walk)
    assert np.array_equal(free, free_w) and np.array_equal(cells, cells_w)
    long_steps = int((np.abs(seg[:, 2:] - seg[:, :2]).max(axis=1) >= 64).sum())
    assert long_steps >= 20000
    for k in range(len(seg)):
        ok, c = oracle.collisionfree(og8, seg[k, :2], seg[k, 2:])
        assert ok == free[k] and c == cells[k], seg[k]
    # a walk asked for a grid it does not take
    ctx.set_grid(np.zeros((4097, 4), dtype=np.uint8))
    with pytest.raises(_ffi.RRTError) as e:
        ctx.prim_collisionfree(seg[:1] * 0, walk=_ffi.WALK_U26)
    assert e.value.code == _ffi.RRT_E_UNSUPPORTED
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the flag
def test_the_flag_takes_a_4096_x_8_grid_and_nothing_else_does():
    ctx = _ffi.Context(0)
    ctx.set_grid(np.zeros((4096, 8), dtype=np.uint8))
    b = _ffi.Batch(ctx, 1, 100, large_grid=True)
    assert b.kernel_name() == LARGE_KERNEL and b.team()[0] == 1
    samples = hostprep.draw_free_samples(np.random.default_rng(0), np.argwhere(np.zeros((4096, 8)) == 0), 100)
    q, keep = _ffi.make_query(_ffi.ALG_STAR, 100, (1, 1), (4090, 6), samples, r2_rewire=hostprep.radius_threshold(500))
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert b.kernel_name() == LARGE_KERNEL and not b.pipelined() and b.team_info()["last"] == 1
    st, ro = oracle.plan(np.zeros((4096, 8), dtype=np.uint8), 100, 1, (1, 1), (4090, 6), samples, r2_rewire=hostprep.radius_threshold(500))
    res = b.get_result(0)
    live = ro.j + (1 if ro.found else 0)
    assert res.j == ro.j and np.array_equal(res.parent[:live], ro.parent[:live]) and np.array_equal(res.vcost[:live], ro.vcost[:live])
    # Informed on such a batch: refused when the query is set
    qi, keep2 = _ffi.make_query(_ffi.ALG_INFORMED, 100, (1, 1), (4090, 6), samples, r2_rewire=100, goal_d2=100, Cmat=np.eye(2))
    with pytest.raises(_ffi.RRTError) as e:
        b.set_query(0, qi)
    assert e.value.code == _ffi.RRT_E_UNSUPPORTED and "RRT_ALG_INFORMED" in str(e.value)
    with pytest.raises(_ffi.RRTError) as e:
        ctx.plan(qi, 100, large_grid=True)
    assert e.value.code == _ffi.RRT_E_UNSUPPORTED
    b.close()
    # without the flag: as before
    with pytest.raises(_ffi.RRTError) as e:
        _ffi.Batch(ctx, 1, 100)
    assert e.value.code == _ffi.RRT_E_UNSUPPORTED
    # the flag with what runs on other kernels
    for kw, word in ((dict(rewire=True), "RRT_FLAG_REWIRE"), (dict(dubins=True), "RRT_FLAG_DUBINS"), (dict(serial=True), "RRT_FLAG_SERIAL"),
                     (dict(pipe1=False), "RRT_FLAG_NOPIPE1")):
        with pytest.raises(_ffi.RRTError) as e:
            _ffi.Batch(ctx, 1, 100, large_grid=True, **kw)
        assert e.value.code == _ffi.RRT_E_UNSUPPORTED and word in str(e.value), kw
    # past 4096 the flag does not help; n past 262143 neither
    ctx.set_grid(np.zeros((4097, 8), dtype=np.uint8))
    with pytest.raises(_ffi.RRTError) as e:
        _ffi.Batch(ctx, 1, 100, large_grid=True)
    assert e.value.code == _ffi.RRT_E_UNSUPPORTED
    ctx.set_grid(np.zeros((4096, 8), dtype=np.uint8))
    with pytest.raises(_ffi.RRTError) as e:
        _ffi.Batch(ctx, 1, 262144, large_grid=True)
    assert e.value.code == _ffi.RRT_E_UNSUPPORTED
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ planners
def _wall_map(W, H):
    """two walls across the map, each with a gap at one end"""
    og = np.zeros((W, H), dtype=np.int64)
    og[W // 3:W // 3 + 6, :H * 3 // 4] = 1
    og[2 * W // 3:2 * W // 3 + 4, H // 4:] = 1
    return og


def _check_planner(cls, og, n, xs, xg, seed=0, **kw):
    """plan() of a planner class on the device against oracle.plan on the same sample stream"""
    alg = 0 if cls is amd.RRTStandard else 1
    og8 = oracle.og_u8(og)
    samples = hostprep.draw_free_samples(np.random.default_rng(seed), np.argwhere(og == 0), n)
    r2 = hostprep.radius_threshold(kw["r_rewire"]) if alg else 0
    st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, logs=False)
    p = cls(og, n, pbar=False, seed=seed, **kw)
    assert p._on_the_large_grid_kernel()
    if st == oracle.ORC_E_GOAL_UNREACHABLE:
        with pytest.raises(IndexError):
            p.plan(np.array(xs), np.array(xg))
        assert p.last_route == "kernel-large"
        return ro
    assert st == 0
    T, gv = p.plan(np.array(xs), np.array(xg))
    assert p.last_route == "kernel-large"
    live = ro.j + (1 if ro.found else 0)
    assert gv == ro.vgoal and p.last_stats["j"] == ro.j
    assert p.last_stats["sum_j"] == ro.sum_j and p.last_stats["sum_near"] == ro.sum_near
    assert T.number_of_nodes() == (n + 1 if ro.found else n)
    par = np.full(live, -1, dtype=np.int64)
    cost = np.zeros(live)
    for u, v, d in T.edges(data=True):
        par[v], cost[v] = u, d["cost"]
    assert np.array_equal(np.array([T.nodes[v]["pt"] for v in range(live)]), ro.pts[:live])
    assert np.array_equal(par, ro.parent[:live])
    assert np.array_equal(cost[1:], ro.vcost[1:live])
    want = np.random.default_rng(seed)
    hostprep.draw_free_samples(want, np.argwhere(og == 0), n)
    assert p.rand_gen.bit_generator.state == want.bit_generator.state
    return ro


# every grid, both classes, every radius and every n of the list at least once; n = 60 000 where the oracle (a brute-force loop
# on one core) takes seconds: with r_rewire = 1500 it takes minutes, with 10^6 half an hour
PLANNER_CASES = [
    ((4096, 4096), "star", 64, 60000), ((4096, 4096), "std", None, 60000), ((4096, 4096), "star", 1e6, 3000),
    ((4096, 4096), "star", 1500, 3000), ((4096, 4096), "star", 5, 3000), ((4096, 4096), "star", 300, 1),
    ((4096, 2100), "star", 300, 60000), ((4096, 2100), "std", None, 3000), ((4096, 2100), "star", 1500, 3000),
    ((4096, 2100), "star", 1e6, 1),
    ((2049, 10), "star", 64, 3000), ((2049, 10), "std", None, 60000), ((2049, 10), "star", 1e6, 3000), ((2049, 10), "star", 5, 1),
    ((2600, 2200), "star", 300, 60000), ((2600, 2200), "std", None, 1), ((2600, 2200), "star", 1500, 3000),
    ((2600, 2200), "star", 1e6, 3000), ((2600, 2200), "star", 5, 60000),
]


@pytest.mark.parametrize("shape,kind,rr,n", PLANNER_CASES)
def test_planner_classes_on_large_grids(shape, kind, rr, n):
    W, H = shape
    og = _wall_map(W, H)
    cls, kw = (amd.RRTStandard, {}) if kind == "std" else (amd.RRTStar, dict(r_rewire=rr))
    ro = _check_planner(cls, og, n, (3, 3), (W - 4, H - 4), **kw)
    if n >= 60000 and shape != (2049, 10):
        assert ro.found and ro.j > 10000


def test_goal_walled_off_and_start_on_an_obstacle():
    W = H = 4096
    og = _wall_map(W, H)
    og[W - 30:W - 28, H - 30:] = 1  # a closed pocket around the goal corner
    og[W - 30:, H - 30:H - 28] = 1
    ro = _check_planner(amd.RRTStar, og, 3000, (3, 3), (W - 4, H - 4), r_rewire=300)
    assert not ro.found  # (the IndexError of the reference's go2goal)
    og = _wall_map(W, H)
    assert og[W // 3 + 2, 100] == 1
    _check_planner(amd.RRTStar, og, 3000, (W // 3 + 2, 100), (W - 4, H - 4), r_rewire=300)
    _check_planner(amd.RRTStandard, og, 3000, (W // 3 + 2, 100), (W - 4, H - 4))


def test_informed_on_a_large_grid_still_runs_on_the_host():
    og = _wall_map(2600, 2200)
    og8 = oracle.og_u8(og)
    xs, xg = np.array((5, 5)), np.array((2500, 2100))
    n = 1500
    p = amd.RRTStarInformed(og, n, 300, 200, pbar=False, seed=0)
    assert not p._on_the_large_grid_kernel() and p._beyond_the_kernels()
    T, gv = p.plan(xs, xg)
    assert p.last_route == "host"
    q = orchelp.use_oracle(amd.RRTStarInformed(og, n, 300, 200, pbar=False, seed=0))  # (the kernels' semantics: the oracle behind _run)
    q._beyond_the_kernels = lambda: False
    To, go = q.plan(xs, xg)
    assert q.last_route == "kernel"
    assert gv == go and list(T.nodes) == list(To.nodes) and list(T.edges) == list(To.edges)
    assert [d["cost"] for *_, d in T.edges(data=True)] == [d["cost"] for *_, d in To.edges(data=True)]
    assert p.rand_gen.bit_generator.state == q.rand_gen.bit_generator.state
    # and the small grids keep their route
    small = amd.RRTStar(np.zeros((64, 64), dtype=int), 200, 10, pbar=False)
    small.plan(np.array((1, 1)), np.array((60, 60)))
    assert small.last_route == "kernel"


# ------------------------------------------------------------------------------------------------------------ C ABI level, with logs
def _ffi_vs_oracle(ctx, og8, alg, n, samples, xs, xg, r2):
    q, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2)
    rc, res = ctx.plan(q, n, logs=True, large_grid=True)
    st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2)
    _same(rc, res, st, ro)
    return res, ro


def _same(rc, res, st, ro, logs=True):
    assert rc == st
    assert res.j == ro.j and res.found == ro.found and res.vgoal == ro.vgoal
    live = ro.j + (1 if ro.found else 0)
    if logs:
        assert np.array_equal(res.nearest_log, ro.nearest_log)
        assert np.array_equal(res.accept_log, ro.accept_log)
        assert np.array_equal(res.j_log, ro.jlog)
    assert np.array_equal(res.pts[:live], ro.pts[:live])
    assert np.array_equal(res.parent[:live], ro.parent[:live])
    assert np.array_equal(res.vcost[:live], ro.vcost[:live])
    assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near


# the pocket recipe of farnn.py at size: every cell is an obstacle but a 600 x 600 pocket at the origin and the one-cell-wide
# diagonal from its corner (599, 599), where the tree starts, to the opposite corner of the map.  One sample in a hundred falls on
# the diagonal; it is visible from the start and from other diagonal vertices only.  With these seeds (found with the oracle on
# the CPU) the tree holds more than 64 vertices, all in the pocket, when a sample near the far corner is accepted: its nearest
# vertex is more than 4096 cells away (d2 > 2^24), behind the last box of the record search, found by the scan over all vertices.
_DIAG = [((t, t), (t, t)) for t in range(600, 4000)]
FAR_CASES = [
    dict(id="far4000_std", W=4000, H=4000, rects=[((0, 599), (0, 599))], field=_DIAG, alg=0, rr=None, n=4000, seed=3, xs=(599, 599), xg=(150, 170)),
    dict(id="far4000_star", W=4000, H=4000, rects=[((0, 599), (0, 599))], field=_DIAG, alg=1, rr=300, n=4000, seed=16, xs=(599, 599), xg=(150, 170)),
]


@pytest.mark.parametrize("c", FAR_CASES, ids=[c["id"] for c in FAR_CASES])
def test_far_nearest_at_size(c):
    og8, samples, r2 = farnn.pipe_case(c)
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    res, ro = _ffi_vs_oracle(ctx, og8, c["alg"], c["n"], samples, c["xs"], c["xg"], r2)
    ctx.close()
    acc = np.flatnonzero((np.asarray(ro.accept_log) != 0) & (np.asarray(ro.jlog) > farnn.TINY))
    d = samples[acc].astype(np.int64) - ro.pts[np.asarray(ro.nearest_log)[acc]].astype(np.int64)
    d2 = (d * d).sum(axis=1)
    assert (d2 > (1 << 24)).sum() >= 1 and ro.j > farnn.TINY, (int(d2.max()), ro.j)


def _golden_ids():
    """ten RRTStandard / RRTStar goldens of policy A, the longest run of ten different (grid, planner, radius) settings"""
    G = orchelp.golden("plans_A.npz")
    seen, out = set(), []
    for m in sorted(G.manifest, key=lambda m: -m["n"]):
        key = (m["grid"], m["alg"], m["r_rewire"])
        if m["alg"] in (0, 1) and key not in seen:
            seen.add(key)
            out.append(m["id"])
    return out[:10]


def _golden_on_the_large_kernel(ctx, G, m):
    og = G.grid(m["grid"])
    og8 = oracle.og_u8(og)
    ctx.set_grid(og8)
    n = m["n"]
    samples = hostprep.draw_free_samples(np.random.default_rng(m["seed"]), np.argwhere(og == 0), n)
    r2 = hostprep.radius_threshold(m["r_rewire"]) if m["alg"] else 0
    b = _ffi.Batch(ctx, 1, n, large_grid=True)
    q, keep = _ffi.make_query(m["alg"], n, m["xstart"], m["xgoal"], samples, r2_rewire=r2)
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert b.kernel_name() == LARGE_KERNEL
    res = b.get_result(0)
    b.close()
    live = res.j + (1 if res.found else 0)
    assert res.vgoal == m["vgoal"] and (n + 1 if res.found else n) == m["rows"]
    assert np.array_equal(res.pts[:live], G.arr(m["id"], "pts")[:live])
    assert np.array_equal(res.parent[:live], G.arr(m["id"], "parent")[:live])
    assert np.array_equal(res.vcost[:live], G.arr(m["id"], "vcost")[:live])


@pytest.mark.parametrize("cid", _golden_ids())
def test_flag_on_small_grids_equals_the_reference(gpu_ctx, cid):
    G = orchelp.golden("plans_A.npz")
    _golden_on_the_large_kernel(gpu_ctx, G, G.by_id[cid])


def test_flag_on_the_bench_scale_golden(gpu_ctx):
    G = orchelp.golden("plans_big_A.npz")
    _golden_on_the_large_kernel(gpu_ctx, G, G.by_id["bench1024__star_r64__s0__n20000"])


def test_batch_of_eight_on_4096_x_4096_launched_twice():
    W = H = 4096
    og = _wall_map(W, H)
    og8 = oracle.og_u8(og)
    free = np.argwhere(og == 0)
    Q, n = 8, 20000
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    b = _ffi.Batch(ctx, Q, n, large_grid=True)
    rng = np.random.default_rng(11)
    refs, keeps = [], []
    for k in range(Q):
        alg = k % 2
        r2 = hostprep.radius_threshold([0, 64, 0, 300, 0, 900, 0, 150][k])
        xs, xg = free[rng.integers(0, len(free))], free[rng.integers(0, len(free))]
        samples = hostprep.draw_free_samples(rng, free, n)
        q, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2)
        keeps.append(keep)
        b.set_query(k, q)
        refs.append(oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, logs=False))
    for launch in range(2):
        b.launch()
        b.sync()
        assert b.kernel_name() == LARGE_KERNEL and b.team_info()["last"] == 1
        for k in range(Q):
            st, ro = refs[k]
            res = b.get_result(k)
            _same(res.status, res, st, ro, logs=False)
        b.rearm()
    b.close()
    ctx.close()
