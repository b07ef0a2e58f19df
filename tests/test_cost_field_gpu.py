"""GPU: the cost-to-come field of a finished tree (rrt_field_kernel / rrt_field_large_kernel, rrt_batch_cost_field / rrt_plan_cost_field,
rrtplanner_amd.field).

Every comparison is exact: vertices with array_equal, costs as raw bits.  The check is fieldref.py -- goalref.connect over the free cells,
-1 / inf for the blocked ones -- on the trees the oracle planned (fieldcases.py, held to their purpose in test_cost_field_cpu.py), and
connect_goals on the device for cells drawn from every window."""
import numpy as np
import pytest

import devcheck
import fieldcases
import fieldref
import oracle
import plannedcases
import relaxcases as rc
import shiftcases as sc
import treecalls as tc
from rrtplanner_amd import _ffi, field, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTStarDubins

pytestmark = pytest.mark.gpu


def _planned_on_a_batch(ctx, c, **bkw):
    """case c planned on a batch of its own; the device's tree is the oracle's"""
    ctx.set_grid(c["og8"])
    b, res = tc.plan_on_own_batch(ctx, c["alg"], c["n"], c["xs"], c["xg"], c["samples"], r2=c["r2"], **bkw)
    _same_tree(res, c["ro"])
    return b, res


def _same_tree(res, ro):
    j = ro.j
    assert res.j == j and np.array_equal(res.pts[:j], ro.pts[:j]) and np.array_equal(res.vcost[:j].view(np.int64), ro.vcost[:j].view(np.int64))


def _inner(window, seed):
    """a window inside `window`, drawn"""
    x0, y0, w, h = window
    rng = np.random.default_rng(seed)
    iw, ih = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
    return (x0 + int(rng.integers(0, w - iw + 1)), y0 + int(rng.integers(0, h - ih + 1)), iw, ih)


def _cells(window, seed, m=64):
    x0, y0, w, h = window
    rng = np.random.default_rng(seed)
    return np.stack([x0 + rng.integers(0, w, size=m), y0 + rng.integers(0, h, size=m)], axis=1)


def _field_window_and_goals(take, goals, window, want, seed):
    """what every case asks of a handle: the field of the window is fieldref's; a window of it is the slice; connect_goals on 64 cells of
    each agrees entry for entry.  take(window) -> (vertex, cost); goals(cells) -> (vertex, cost)"""
    got = take(window)
    fieldref.same(got, want)
    inner = _inner(window, seed)
    part = take(inner)
    fieldref.same(part, fieldref.cut(want, window, inner))
    for win, (v, c), s in ((window, got, seed + 1), (inner, part, seed + 2)):
        cells = _cells(win, s)
        gv, gc = goals(cells)
        at = (cells[:, 0] - win[0], cells[:, 1] - win[1])
        assert np.array_equal(gv, v[at]) and np.array_equal(gc.view(np.int64), c[at].view(np.int64))
    return got


# ------------------------------------------------------------------------------------------------ the three maps, through Batch and Context
@pytest.mark.parametrize("name", sorted(fieldcases.PLANNED))
def test_the_field_is_connect_goals_for_every_cell_on_a_batch(gpu_ctx, name):
    c, window, want = fieldcases.planned(name)
    b, res = _planned_on_a_batch(gpu_ctx, c)
    before = tc.snapshot(res)
    v, cost = _field_window_and_goals(lambda w: field.batch_cost_field(b, 0, w), lambda g: b.connect_goals(0, g), window, want, 11)
    assert tc.same_snapshot(before, tc.snapshot(b.get_result(0)))  # the tree arrays are never written
    # the statistics, of the call on the whole window (taken again: the last call was a part of it)
    field.batch_cost_field(b, 0, window)
    st, ms = field.cost_field_stats(b), field.cost_field_ms(b)
    x0, y0, w, h = window
    free = c["og8"][x0:x0 + w, y0:y0 + h] == 0
    print(name, st, ms)
    assert st["cells"] == free.sum() and st["los"] >= (want[0] >= 0).sum() and st["buckets"] >= free.sum() and st["priced"] >= (want[0] >= 0).sum()
    assert len(ms) == 4 and all(t >= 0.0 for t in ms) and ms[1] > 0.0
    b.close()


@pytest.mark.parametrize("name", sorted(fieldcases.PLANNED))
def test_the_field_through_a_context(name):
    c, window, want = fieldcases.planned(name)
    ctx = _ffi.Context(0)
    ctx.set_grid(c["og8"])
    q, keep = _ffi.make_query(c["alg"], c["n"], c["xs"], c["xg"], c["samples"], r2_rewire=c["r2"])
    rc_, res = ctx.plan(q, c["n"])
    _same_tree(res, c["ro"])
    _field_window_and_goals(lambda w: field.context_cost_field(ctx, w), ctx.connect_goals, window, want, 21)
    assert field.cost_field_stats(ctx)["cells"] > 0 and len(field.cost_field_ms(ctx)) == 4
    ctx.close()


@pytest.mark.parametrize("grid", ["maze64x96", "square100"])
def test_the_field_of_a_planner(grid):
    """cost_field(planner): the planner draws its own samples, so the check is fieldref on the tree plan() returned"""
    og = plannedcases.G.grid(grid)
    og8 = oracle.og_u8(og)
    free = np.argwhere(og8 == 0)
    rng = np.random.default_rng(5)
    xs, xg = free[rng.integers(len(free))], free[rng.integers(len(free))]
    p = amd.RRTStar(og, 200, 12, pbar=False, seed=3)
    T, gv = p.plan(xs, xg)
    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    window = fieldref.whole(og8)
    want = fieldref.field(og8, points, vcosts, j)
    got = _field_window_and_goals(lambda w: field.cost_field(p, None if w == window else w), p.connect_goals, window, want, 31)
    assert got[0].shape == og8.shape and (got[0] >= 0).any()
    with pytest.raises(ValueError, match="inside"):
        field.cost_field(p, (0, 0, og8.shape[0] + 1, 1))
    with pytest.raises(ValueError, match="window"):
        field.cost_field(p, (0, 0, 1))
    p.set_og(og)
    with pytest.raises(RuntimeError, match="plan"):
        field.cost_field(p)


# ------------------------------------------------------------------------------------------------ whoever grew the tree
@pytest.mark.parametrize("kernel", devcheck.KERNELS_NOFAULT)
def test_the_field_does_not_depend_on_who_grew_the_tree(gpu_ctx, kernel):
    c, window, want = fieldcases.planned("maze")
    b, res = _planned_on_a_batch(gpu_ctx, c, **devcheck.KERNEL_ARGS[kernel])
    fieldref.same(field.batch_cost_field(b, 0, window), want)
    b.close()


def test_the_field_of_an_informed_query(gpu_ctx):
    """an Informed RRT* query through its unit-ball hand-over, as devcheck.oracle_vs_batch runs it; the check is fieldref on its tree"""
    c, _, _ = fieldcases.planned("maze")
    og8, n = c["og8"], 250
    gpu_ctx.set_grid(og8)
    rng = np.random.default_rng(44)
    free = np.argwhere(og8 == 0)
    samples = hostprep.draw_free_samples(rng, free, n)
    xs, xg = c["xs"], c["xg"]
    q, keep = _ffi.make_query(2, n, xs, xg, samples, r2_rewire=hostprep.radius_threshold(12), goal_d2=hostprep.goal_threshold(6),
                              Cmat=hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64)))
    b = _ffi.Batch(gpu_ctx, 1, n)
    b.set_query(0, q)
    b.launch()
    b.sync()
    res = b.get_result(0)
    if res.status == _ffi.RRT_NEED_UNITBALL:
        b.set_unitball(0, hostprep.draw_unitball(rng, n - res.i_switch), res.i_switch)
        b.launch()
        b.sync()
        res = b.get_result(0)
    assert res.j > 20
    window = (8, 10, 40, 60)
    fieldref.same(field.batch_cost_field(b, 0, window), fieldref.field(og8, res.pts, res.vcost, res.j, window))
    b.close()


# ------------------------------------------------------------------------------------------------ sizes, windows, ties
@pytest.mark.parametrize("k", fieldcases.SIZES)
def test_trees_around_the_wavefront_and_windows_at_the_edges(gpu_ctx, k):
    c = fieldcases.sized(k)
    b, res = _planned_on_a_batch(gpu_ctx, c)
    window = fieldref.whole(c["og8"])
    want = fieldcases.reference(("sized", k), c, window)
    fieldref.same(field.batch_cost_field(b, 0, window), want)
    for win in fieldcases.sized_windows():
        got = field.batch_cost_field(b, 0, win)
        assert got[0].shape == (win[2], win[3])
        fieldref.same(got, fieldref.cut(want, window, win))
    if k >= 63:
        assert (want[0] > 0).sum() > 100 and (want[0] < 0).sum() > 100
    b.close()


@pytest.mark.parametrize("swapped", [False, True])
def test_an_exact_tie_across_buckets_goes_to_the_lower_index(gpu_ctx, swapped):
    c = fieldcases.tie(swapped)
    b, res = _planned_on_a_batch(gpu_ctx, c)
    window = fieldref.whole(c["og8"])
    want = fieldcases.reference(("tie", swapped), c, window)
    got = field.batch_cost_field(b, 0, window)
    assert got[0][fieldcases.TIE_CELL] == 1 and got[1][fieldcases.TIE_CELL] == 32.0 + np.sqrt(np.float64(2048))
    fieldref.same(got, want)
    b.close()


# ------------------------------------------------------------------------------------------------ kept, grown, re-rooted and relaxed trees
KEPT_WINDOW = (84, 64, 32, 24)  # across the wall of treecalls.wall: cells on both sides, more than half of them cut off


def _kept(ctx):
    """treecalls.base() planned and kept on the wall map of shiftcases.seed_case: (batch, case, seed case)"""
    c, d = tc.base(), sc.seed_case("wall")
    b, res = _planned_on_a_batch(ctx, c)
    ctx.set_grid(d["og2"])
    assert np.array_equal(b.keep_tree(0), d["alive"])
    return b, c, d


def test_after_keep_tree_the_field_runs_over_the_alive_view_in_the_old_numbers(gpu_ctx):
    b, c, d = _kept(gpu_ctx)
    ro = c["ro"]
    alive, v, cost, tried = fieldref.kept_field(d["og2"], ro.pts, ro.parent, ro.vcost, ro.j, KEPT_WINDOW)
    got = _field_window_and_goals(lambda w: field.batch_cost_field(b, 0, w), lambda g: b.connect_goals(0, g), KEPT_WINDOW, (v, cost, tried), 41)
    winners = got[0][got[0] >= 0]
    assert (~alive).sum() > 50 and np.all(alive[winners]) and len(winners) > 200 and (got[0] < 0).sum() > 200
    assert np.any((np.cumsum(alive) - 1)[winners] != winners)  # the old numbers, not the view's
    assert field.cost_field_ms(b)[2] > 0.0  # the remap ran
    b.close()


@pytest.mark.parametrize("op", ["grow", "reroot", "relax"])
def test_after_a_seed_call_the_field_runs_on_the_new_tree(gpu_ctx, op):
    m = sc.SEED_M[0]
    b, c, d = _kept(gpu_ctx)
    samples = d["samples"][:m]
    if op == "grow":
        g = sc.grown("wall", m)
        b.grow(0, samples)
    elif op == "reroot":
        R, g = sc.rerooted(m)
        b.reroot(0, sc.reroot_vertex(), samples)
    else:
        X, g = sc.relaxed(m)
        b.relax(0, rc.R_of(tc.RR), samples)
    b.launch()
    b.sync()
    tc.same_result(b.get_result(0), g)
    want = fieldref.field(d["og2"], g.pts, g.vcost, g.j, KEPT_WINDOW)
    fieldref.same(field.batch_cost_field(b, 0, KEPT_WINDOW), want)
    assert (want[0] >= 0).sum() > 200 and (want[0] < 0).sum() > 200
    b.close()


def test_one_query_of_a_batch_of_three(gpu_ctx):
    cases = [fieldcases.planned("maze")[0], plannedcases.oracle_planned("maze64x96", 1, 300, 61), plannedcases.oracle_planned("maze64x96", 1, 120, 62)]
    gpu_ctx.set_grid(cases[0]["og8"])
    b = _ffi.Batch(gpu_ctx, 3, 300)
    keeps = [tc.set_case_query(b, q, c) for q, c in enumerate(cases)]
    b.launch()
    b.sync()
    window = (5, 20, 30, 40)
    for q in (2, 0, 1):
        res = b.get_result(q)
        _same_tree(res, cases[q]["ro"])
        fieldref.same(field.batch_cost_field(b, q, window), fieldref.field(cases[q]["og8"], res.pts, res.vcost, res.j, window))
    b.close()
    del keeps


# ------------------------------------------------------------------------------------------------ large grids
def test_a_large_grid_batch():
    """4096 x 8: the smallest grid with a side beyond 2048 that test_connect_goals_gpu.py runs such a batch on"""
    W, H = 4096, 8
    og = np.zeros((W, H), dtype=np.int64)
    og[2000:2003, :6] = 1
    og8 = oracle.og_u8(og)
    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    b, res = tc.plan_on_own_batch(ctx, 1, 400, (1, 1), (4090, 6), tc.free_samples(og, 400, 14), r2=hostprep.radius_threshold(500), large_grid=True)
    assert b.kernel_name() == "rrt_pipe_large_kernel" and res.j > 100
    window = (1900, 0, 220, 8)
    want = fieldref.field(og8, res.pts, res.vcost, res.j, window)
    got = _field_window_and_goals(lambda w: field.batch_cost_field(b, 0, w), lambda g: b.connect_goals(0, g), window, want, 51)
    assert (got[0] >= 0).sum() > 1000 and (want[2] > 1).sum() > 100
    for win in ((0, 0, 64, 8), (4032, 0, 64, 8), (4095, 7, 1, 1)):  # the far ends: lines of up to 4095 cells
        fieldref.same(field.batch_cost_field(b, 0, win), fieldref.field(og8, res.pts, res.vcost, res.j, win))
    b.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------ refusals
def _refusal(call, *args):
    with pytest.raises(_ffi.RRTError) as e:
        call(*args)
    return e.value.code, str(e.value)


def _as_connect_goals(b, q, window, prefix="rrt_batch_"):
    """the field call is refused with connect_goals' code and text, its own name in place of connect_goals'"""
    code, text = _refusal(b.connect_goals, q, [(5, 5)]) if prefix == "rrt_batch_" else _refusal(b.connect_goals, [(5, 5)])
    assert prefix + "connect_goals" in text
    got = _refusal(field.batch_cost_field, b, q, window) if prefix == "rrt_batch_" else _refusal(field.context_cost_field, b, window)
    assert got == (code, text.replace(prefix + "connect_goals", prefix + "cost_field")), got
    return text


def test_refusals():
    ctx = _ffi.Context(0)
    og = tc.wall_map()
    og8 = oracle.og_u8(og)
    ctx.set_grid(og8)
    win = (0, 0, 8, 8)
    assert "no rrt_plan" in _as_connect_goals(ctx, None, win, "rrt_plan_")
    for report in (field.cost_field_ms, field.cost_field_stats):
        assert _refusal(report, ctx)[0] == _ffi.RRT_E_ARG
    samples = tc.free_samples(og, 300, 17)
    b = _ffi.Batch(ctx, 2, 300)
    assert "no query set" in _as_connect_goals(b, 0, win)
    q, keep = _ffi.make_query(1, 300, (5, 5), (190, 150), samples, r2_rewire=900)
    b.set_query(0, q)
    assert "not launched" in _as_connect_goals(b, 0, win)
    code, text = _refusal(field.cost_field_ms, b)
    assert code == _ffi.RRT_E_ARG and "no rrt_batch_cost_field on this batch yet" in text
    b.launch()
    b.sync()
    v, cost = field.batch_cost_field(b, 0, win)
    assert v.shape == (8, 8)
    assert "q=2" in _as_connect_goals(b, 2, win)
    assert "q=-1" in _as_connect_goals(b, -1, win)
    assert "no query set" in _as_connect_goals(b, 1, win)
    # the refusals of its own, behind connect_goals': code and text
    W, H = og8.shape
    for bad, text in (((0, 0, 0, 5), "rrt_batch_cost_field: a window of 0 x 5 cells"), ((0, 0, 5, 0), "rrt_batch_cost_field: a window of 5 x 0 cells"),
                      ((0, 0, -1, 5), "rrt_batch_cost_field: a window of -1 x 5 cells"),
                      ((W - 3, 0, 4, 4), f"rrt_batch_cost_field: the window ({W - 3}, 0) + 4 x 4 is not inside the {W}x{H} grid"),
                      ((0, H - 3, 4, 4), f"rrt_batch_cost_field: the window (0, {H - 3}) + 4 x 4 is not inside the {W}x{H} grid"),
                      ((-1, 0, 4, 4), f"rrt_batch_cost_field: the window (-1, 0) + 4 x 4 is not inside the {W}x{H} grid"),
                      ((0, 0, W + 1, H), f"rrt_batch_cost_field: the window (0, 0) + {W + 1} x {H} is not inside the {W}x{H} grid"),
                      ((2 ** 31 - 2, 0, 4, 4), f"rrt_batch_cost_field: the window ({2 ** 31 - 2}, 0) + 4 x 4 is not inside the {W}x{H} grid")):
        assert _refusal(field.batch_cost_field, b, 0, bad) == (_ffi.RRT_E_ARG, f"librrt_hip error {_ffi.RRT_E_ARG}: {text}"), bad
    L = field._lib()
    out_v, out_c = np.zeros(64, dtype=np.int32), np.zeros(64, dtype=np.float64)
    for pv, pc in ((None, out_c.ctypes.data), (out_v.ctypes.data, None)):
        assert L.rrt_batch_cost_field(b._h, 0, 0, 0, 8, 8, pv, pc) == _ffi.RRT_E_ARG
        assert L.rrt_last_error_string(ctx.handle).decode() == "rrt_batch_cost_field: NULL"
    assert L.rrt_batch_cost_field(None, 0, 0, 0, 8, 8, out_v.ctypes.data, out_c.ctypes.data) == _ffi.RRT_E_ARG
    assert L.rrt_batch_cost_field_stats(b._h, None) == _ffi.RRT_E_ARG and L.rrt_plan_cost_field_ms(None, None) == _ffi.RRT_E_ARG
    # a window refused behind a query that has not finished: connect_goals' refusal comes first
    b.rearm()
    assert "not finished" in _as_connect_goals(b, 0, (0, 0, 0, 0))
    b.launch()
    b.sync()
    want = field.batch_cost_field(b, 0, win)
    assert field.cost_field_stats(b)["cells"] == (og8[:8, :8] == 0).sum()
    # a call after set_grid: same shape, another generation; then another shape
    ctx.set_grid(og8)
    assert "replaced" in _as_connect_goals(b, 0, win)
    assert field.cost_field_stats(b)["cells"] == (og8[:8, :8] == 0).sum()  # a refusal changes nothing
    b.rearm()
    b.launch()
    b.sync()
    fieldref.same(field.batch_cost_field(b, 0, win), want)
    ctx.set_grid(np.zeros((64, 64), dtype=np.uint8))
    assert "shape" in _as_connect_goals(b, 0, win)
    b.close()
    # a Dubins batch: a text of its own, in front of everything of connect_goals'
    s = hostprep.draw_free_samples(np.random.default_rng(18), np.argwhere(np.zeros((64, 64)) == 0), 300)
    hd = np.random.default_rng(19).integers(0, 16, size=300)
    b = _ffi.Batch(ctx, 1, 300, dubins=True)
    dub = "a Dubins batch (its goal is a pose, and there is no field of poses here; these kernels price straight lines to cells)"
    assert _refusal(field.batch_cost_field, b, 5, win) == (_ffi.RRT_E_UNSUPPORTED, f"librrt_hip error {_ffi.RRT_E_UNSUPPORTED}: rrt_batch_cost_field: {dub}")
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR, 300, (5, 5, 0), (40, 40, 3), s, r2_rewire=400, headings=hd, rho=3.0, nh=16)
    b.set_query(0, q)
    b.launch()
    b.sync()
    assert _refusal(field.batch_cost_field, b, 0, win) == (_ffi.RRT_E_UNSUPPORTED, f"librrt_hip error {_ffi.RRT_E_UNSUPPORTED}: rrt_batch_cost_field: {dub}")
    b.close()
    ctx.close()
    with pytest.raises(ValueError, match="Dubins"):
        field.cost_field(RRTStarDubins(np.zeros((64, 64), dtype=int), 100, 20, 3.0, pbar=False))
