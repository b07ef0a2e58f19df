"""GPU: the pose cost field of a finished Dubins tree (rrt_pose_field_kernel, rrt_batch_pose_field / rrt_plan_pose_field,
rrtplanner_amd.posefield).

Every comparison is exact: vertices and headings with array_equal, costs as raw bits.  The check is posefieldref.py -- poseref.connect
for every free cell and every heading, -1 / inf / -1 for the blocked ones -- on the cases of posefieldcases.py (held to their purpose in
test_pose_field_cpu.py), and connect_poses on the device for 16 cells drawn from every window."""
import json
import os

import numpy as np
import pytest

import posefieldcases as pfc
import posefieldref
import posegrowref
import poserelaxcases as pc
import poseref
from posecalls import planned_batch, planned_logged_batch, refused_with_golden_text
from rrtplanner_amd import _ffi, hostprep, moving, posefield
from rrtplanner_amd import rrt as amd
from treecalls import same_snapshot, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pose_field_refusals.json")))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _inner(window, seed):
    """a window inside `window`, drawn"""
    x0, y0, w, h = window
    rng = np.random.default_rng(seed)
    iw, ih = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
    return (x0 + int(rng.integers(0, w - iw + 1)), y0 + int(rng.integers(0, h - ih + 1)), iw, ih)


def _as_connect_poses(connect, cells, H, nh):
    """(vertex, cost, heading) of the device's own connect_poses for the cells at heading H; H < 0: every heading of every cell, and of
    each cell the (cost, heading)-first answer"""
    m = len(cells)
    hs = np.arange(nh) if H < 0 else np.array([H])
    poses = np.column_stack([np.repeat(cells, len(hs), axis=0), np.tile(hs, m)])
    v, c = connect(poses)
    v, c = v.reshape(m, len(hs)), c.reshape(m, len(hs))
    e = np.argmin(c, axis=1)  # (the first among equal costs: the smallest heading)
    at = (np.arange(m), e)
    return v[at], c[at], np.where(v[at] >= 0, hs[e], -1)


def _field_window_and_poses(take, connect, window, f, seed):
    """what every case asks of a handle, at any heading and at two fixed ones: the field of the window is posefieldref's; a window of it
    is the slice; connect_poses on 16 cells of each agrees entry for entry.  take(window, H) -> (vertex, cost, heading);
    connect(poses) -> (vertex, cost)"""
    out = {}
    for H in pfc.headings_of(f.nh):
        want = posefieldref.answer(f, H)
        got = take(window, H)
        posefieldref.same(got, want)
        inner = _inner(window, seed + H)
        part = take(inner, H)
        posefieldref.same(part, posefieldref.cut(want, window, inner))
        for win, (v, c, h), s in ((window, got, seed + 100), (inner, part, seed + 200)):
            cells = pfc.cells_of(win, s)
            gv, gc, gh = _as_connect_poses(connect, cells, H, f.nh)
            at = (cells[:, 0] - win[0], cells[:, 1] - win[1])
            assert np.array_equal(gv, v[at]) and np.array_equal(_bits(gc), _bits(c[at])) and np.array_equal(gh, h[at]), (H, win)
        out[H] = got
    return out


def _spot(connect, window, got, H, nh, seed):
    """connect_poses on 16 cells drawn from the window agrees with the field `got` taken at heading H"""
    cells = pfc.cells_of(window, seed)
    gv, gc, gh = _as_connect_poses(connect, cells, H, nh)
    at = (cells[:, 0] - window[0], cells[:, 1] - window[1])
    assert np.array_equal(gv, got[0][at]) and np.array_equal(_bits(gc), _bits(got[1][at])) and np.array_equal(gh, got[2][at]), (H, window)


def _on_a_batch(ctx, w, f, window, seed, serial=False):
    b = planned_batch(ctx, w, serial=serial)
    got = _field_window_and_poses(lambda win, H: posefield.batch_pose_field(b, 0, win, H), lambda p: b.connect_poses(0, p), window, f, seed)
    return b, got


def _on_a_context(w, f, window, seed, serial=False):
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    q, keep = poseref.device_query(w)
    rc, res = ctx.plan(q, w.n, serial=serial)
    assert rc == w.status and res.j == w.j
    _field_window_and_poses(lambda win, H: posefield.context_pose_field(ctx, win, H), ctx.connect_poses, window, f, seed)
    posefield.context_pose_field(ctx, window)
    st, ms = posefield.pose_field_stats(ctx), posefield.pose_field_ms(ctx)
    assert st["cells"] == f.free.sum() and len(ms) == 4 and ms[1] > 0.0
    ctx.close()


# ------------------------------------------------------------------------------------------------ the workloads: Batch, Context, planner
@pytest.mark.parametrize("name", sorted(pfc.WINDOWS))
def test_the_field_is_connect_poses_for_every_cell_on_a_batch(gpu_ctx, name):
    w, window, f = pfc.workload(name)
    b, got = _on_a_batch(gpu_ctx, w, f, window, 11, serial=name in ("B", "G1"))  # both kernels that leave a Dubins tree
    before = snapshot(b.get_result(0))
    x0, y0, ww, hh = window
    free = int(f.free.sum())
    for H in pfc.headings_of(w.nh):  # the counters, of the call on the whole window
        v, c, h = posefield.batch_pose_field(b, 0, window, H)
        st, ms = posefield.pose_field_stats(b), posefield.pose_field_ms(b)
        print(name, H, st, ms)
        asked = w.nh if H < 0 else 1
        assert st["cells"] == free and st["sweeps"] >= (v >= 0).sum() and st["buckets"] >= free and (v >= 0).sum() <= st["words"] <= free * w.j * asked + free
        if name in pfc.CLUTTERED:
            assert st["words"] < free * w.j * asked  # the pruning is real
        assert len(ms) == 4 and all(t >= 0.0 for t in ms) and ms[1] > 0.0
    assert same_snapshot(before, snapshot(b.get_result(0)))  # the tree arrays are never written
    b.close()


@pytest.mark.parametrize("name", sorted(pfc.WINDOWS))
def test_the_field_through_a_context(name):
    w, window, f = pfc.workload(name)
    _on_a_context(w, f, window, 21, serial=name in ("A", "G256"))


def _planner_answers(p, w, window, f):
    for H in pfc.headings_of(w.nh):
        got = posefield.pose_field(p, window, None if H < 0 else H)
        posefieldref.same(got, posefieldref.answer(f, H))
        cells = pfc.cells_of(window, 31 + H)
        v, c, h = p.connect_poses(np.column_stack([cells, np.full(len(cells), H)]))
        at = (cells[:, 0] - window[0], cells[:, 1] - window[1])
        assert np.array_equal(v, got[0][at]) and np.array_equal(_bits(c), _bits(got[1][at])) and np.array_equal(np.where(v >= 0, h, -1), got[2][at])


@pytest.mark.parametrize("name", sorted(pfc.WINDOWS))
def test_the_field_of_a_star_planner(name):
    """pose_field(planner) of RRTStarDubins: the planner draws the workload's stream, so its tree is the oracle's.  The whole grid of A and
    B, 9600 cells, is a window with runs of two cells."""
    w, window, f = pfc.workload(name)
    p = poseref.planner_of(w)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j
    _planner_answers(p, w, window, f)
    whole = posefield.pose_field(p, None, w.nh - 1)
    assert whole[0].shape == w.og8.shape
    posefieldref.same(posefieldref.cut(whole, (0, 0) + w.og8.shape, window), posefieldref.fixed(f, w.nh - 1))
    p.set_n(w.n)
    with pytest.raises(RuntimeError, match="plan"):
        posefield.pose_field(p, window)
    refused_with_golden_text(GOLDEN, "straight_class", posefield.pose_field, amd.RRTStar(w.og, 50, 8, pbar=False))


def test_the_field_of_an_rrt_dubins_planner():
    """... and of RRTDubins (poseref's workload D): the window lies around the first goal of the workload that connects"""
    w = poseref.workload("D")
    g = w.goals[np.flatnonzero(w.vertex >= 0)[0]]
    W, H = w.og8.shape
    window = (int(np.clip(g[0] - 2, 0, W - 5)), int(np.clip(g[1] - 2, 0, H - 5)), 5, 5)
    f = pfc.reference("D", w, window)
    assert (posefieldref.any_heading(f)[0] >= 0).sum() >= 5
    p = poseref.planner_of(w)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j and type(p).__name__ == "RRTDubins"
    _planner_answers(p, w, window, f)


def test_one_tree_on_a_whole_small_map(gpu_ctx):
    w, window, f = pfc.small_map()
    b, got = _on_a_batch(gpu_ctx, w, f, window, 41)
    assert got[-1][0].shape == (24, 24) and posefield.pose_field_stats(b)["cells"] <= int(f.free.sum())
    b.close()
    _on_a_context(w, f, window, 42)


# ------------------------------------------------------------------------------------------------ window shapes, tree sizes
@pytest.mark.parametrize("k", range(8))
def test_windows_at_the_edges_of_a_grid_no_bucket_edge_divides(gpu_ctx, k):
    w, window, f = pfc.edge_window(k)
    b = planned_batch(gpu_ctx, w)
    for H in pfc.headings_of(w.nh):
        got = posefield.batch_pose_field(b, 0, window, H)
        assert got[0].shape == (window[2], window[3])
        posefieldref.same(got, posefieldref.answer(f, H))
        _spot(lambda p: b.connect_poses(0, p), window, got, H, w.nh, 71 + k)
    b.close()


@pytest.mark.parametrize("j", pfc.SIZES)
def test_trees_around_the_wavefront_and_the_list(gpu_ctx, j):
    """j * headings asked is the number of pairs of a cell that prunes nothing: 1, 2, 63, 64 (one wave), 65, 129, 1025 at one heading,
    16 times as many at any heading (more than the list of 256 survivors holds from j = 129 on)"""
    w = poseref.stride_tree(j, j % 2)
    b = planned_batch(gpu_ctx, w, serial=j in (2, 64))
    for k in range(len(pfc.SIZED_WINDOWS)):
        w, window, f = pfc.sized(j, k)
        for H in pfc.headings_of(w.nh):
            got = posefield.batch_pose_field(b, 0, window, H)
            posefieldref.same(got, posefieldref.answer(f, H))
            _spot(lambda p: b.connect_poses(0, p), window, got, H, w.nh, 81 + k)
    b.close()


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_a_duplicate_of_the_start_pose_never_wins(gpu_ctx, rho, nh):
    for star in (0, 1):
        w, window, f = pfc.tie_duplicate(rho, nh, star)
        b, got = _on_a_batch(gpu_ctx, w, f, window, 51)
        for H, (v, c, h) in got.items():
            assert not np.any(v == w.dup), (rho, nh, star, H)
        assert (got[-1][0] == 0).any()  # the root wins cells of the window, with the duplicate right behind it
        b.close()


@pytest.mark.parametrize("rho,nh", poseref.TIE_PAIRS)
def test_mirror_words_of_equal_cost_go_to_the_lower_index(gpu_ctx, rho, nh):
    for star in (0, 1):
        w, iL, iR, window, f = pfc.tie_mirror(rho, nh, star)
        b = planned_batch(gpu_ctx, w)
        v, c, h = posefield.batch_pose_field(b, 0, window, 0)
        posefieldref.same((v, c, h), posefieldref.fixed(f, 0))
        assert v[90 - window[0], 50 - window[1]] == iL and _bits(c[90 - window[0], 50 - window[1]]) == _bits(w.c[0, iR])
        _spot(lambda p: b.connect_poses(0, p), window, (v, c, h), 0, nh, 91)
        got = posefield.batch_pose_field(b, 0, window, -1)
        posefieldref.same(got, posefieldref.any_heading(f))
        _spot(lambda p: b.connect_poses(0, p), window, got, -1, nh, 92)
        b.close()


def test_headings_of_equal_cost_go_to_the_smaller_heading(gpu_ctx):
    found = pfc.heading_tie()
    assert found is not None  # (test_pose_field_cpu.py shows that it is such a tie)
    w, window, f, (h0, h1) = found
    b = planned_batch(gpu_ctx, w)
    v, c, h = posefield.batch_pose_field(b, 0, window, -1)
    assert (v[0, 0], h[0, 0]) == (f.vertex[0, 0, h0], h0) and _bits(c[0, 0]) == _bits(f.cost[0, 0, h1])
    for H in (h0, h1):
        posefieldref.same(posefield.batch_pose_field(b, 0, window, H), posefieldref.fixed(f, H))
    around = (window[0] - 2, window[1] - 2, 5, 5)
    got = posefield.batch_pose_field(b, 0, around, -1)
    posefieldref.same(got, posefieldref.any_heading(pfc.reference("around the heading tie", w, around)))
    _spot(lambda p: b.connect_poses(0, p), around, got, -1, w.nh, 93)
    b.close()


# ------------------------------------------------------------------------------------------------ kept, grown, relaxed and re-rooted trees
def test_after_keep_pose_tree_the_field_runs_over_the_alive_view_in_the_old_numbers(gpu_ctx):
    k, window, f = pfc.kept()
    w = k.w
    b = planned_batch(gpu_ctx, w)
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive)
    got = _field_window_and_poses(lambda win, H: posefield.batch_pose_field(b, 0, win, H), lambda p: b.connect_poses(0, p), window, f, 61)
    winners = got[-1][0][got[-1][0] >= 0]
    assert np.all(k.alive[winners]) and np.any((np.cumsum(k.alive) - 1)[winners] != winners)  # the old numbers, not the view's
    assert posefield.pose_field_ms(b)[2] > 0.0  # the remap ran
    b.close()


CHANGED_WINDOW = (74, 50, 6, 6)  # of workload B's grid, across an obstacle edge


@pytest.mark.parametrize("op", ["grow_poses", "relax_poses", "reroot_poses"])
def test_after_a_seed_call_the_field_runs_on_the_new_tree(gpu_ctx, op):
    """the restatement is fed with get_result's arrays: the tree the call left on the device"""
    k = pfc.kept()[0]
    w = k.w
    b = planned_logged_batch(gpu_ctx, w, "block")
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive)
    s = posegrowref.more_poses(w, k.og8, min(40, w.n - int(k.alive.sum())), seed=9)
    if op == "grow_poses":
        b.grow_poses(0, s)
    elif op == "relax_poses":
        b.relax_poses(0, pc.R_of(12), s)
    else:
        ids = np.flatnonzero(k.alive)  # the new root: the alive vertex nearest to the window
        near = ids[np.argmin(((w.ro.pts[ids] - np.array(CHANGED_WINDOW[:2]) - 3) ** 2).sum(axis=1))]
        moving.batch_reroot_poses(b, 0, int(near), pc.R_of(12), s)
    b.launch()
    b.sync()
    res = b.get_result(0)
    assert res.j >= 20
    f = posefieldref.field(k.og8, res.pts, res.head, res.vcost, res.j, w.rho, w.nh, CHANGED_WINDOW)
    anyv = posefieldref.any_heading(f)[0]
    assert (anyv >= 0).sum() >= 8 and (~f.free).sum() > 0
    for H in pfc.headings_of(w.nh):
        got = posefield.batch_pose_field(b, 0, CHANGED_WINDOW, H)
        posefieldref.same(got, posefieldref.answer(f, H))
        _spot(lambda p: b.connect_poses(0, p), CHANGED_WINDOW, got, H, w.nh, 94)
    b.close()


def test_the_second_query_of_a_batch_of_three(gpu_ctx):
    """three queries with their own (rho, nh) and trees: the field of each is its own"""
    w = poseref.workload("E")
    gpu_ctx.set_grid(w.og8)
    free = np.argwhere(w.og8 == 0)
    par = [(2.0, 64, 1, 120), (3.0, 8, 0, 200), (1.5, 16, 1, 160)]  # rho, nh, star, n
    b = _ffi.Batch(gpu_ctx, 3, 200, dubins=True)
    keeps, made = [], []
    for q, (rho, nh, star, n) in enumerate(par):
        rng = np.random.default_rng(70 + q)
        samples, heads = hostprep.draw_free_samples(rng, free, n), rng.integers(0, nh, n)
        m = poseref.made(f"three {q}", w.og8, n, star, 12, rho, nh, (w.xs[0], w.xs[1], q % nh), (w.xg[0], w.xg[1], (3 + q) % nh), samples, heads, [w.xg[:2] + (0,)])
        qu, keep = poseref.device_query(m)
        keeps.append(keep)
        made.append(m)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    window = (w.xs[0] - 2 if w.xs[0] >= 2 else 0, w.xs[1] - 2 if w.xs[1] >= 2 else 0, 5, 5)
    for q in (1, 2, 0):
        m = made[q]
        res = b.get_result(q)
        assert res.j == m.j >= 10 and np.array_equal(_bits(res.vcost[:m.j]), _bits(m.ro.vcost[:m.j]))
        f = pfc.reference(("three", q), m, window)
        assert (posefieldref.any_heading(f)[0] >= 0).sum() >= 5
        for H in pfc.headings_of(m.nh):
            got = posefield.batch_pose_field(b, q, window, H)
            posefieldref.same(got, posefieldref.answer(f, H))
            _spot(lambda p: b.connect_poses(q, p), window, got, H, m.nh, 95 + q)
    b.close()
    del keeps


# ------------------------------------------------------------------------------------------------ runs of more than one cell
def _long_runs(b, q, window, nh, probes, seed):
    """A window whose wavefronts decide runs of several cells -- every cell but the first of a run starts from the winner of the cell
    before it and scans all buckets from that bound -- at any heading and at two fixed ones: equal, entry for entry, to the same cells
    taken through tiles that get one cell a wavefront, to the restatement on the probes, and to connect_poses on 16 cells.
    probes: [(small window, posefieldref.Field)]"""
    assert pfc.run_of(window) > 1
    connect = lambda p: b.connect_poses(q, p)  # noqa: E731
    for H in pfc.headings_of(nh):
        got = posefield.batch_pose_field(b, q, window, H)
        for tile in pfc.tiles(window):
            assert pfc.run_of(tile) == 1
            posefieldref.same(posefield.batch_pose_field(b, q, tile, H), posefieldref.cut(got, window, tile))
        for probe, f in probes:
            posefieldref.same(posefieldref.cut(got, window, probe), posefieldref.answer(f, H))
        _spot(connect, window, got, H, nh, seed + H)
        for probe, f in probes:  # ... and 16 cells where the tree is
            _spot(connect, probe, posefieldref.cut(got, window, probe), H, nh, seed + 50 + H)
        assert (got[0] >= 0).sum() > 1000 and (got[0] < 0).sum() > 1000


@pytest.mark.parametrize("k", range(len(pfc.WIDE_WINDOWS)))
def test_runs_of_six_fifteen_and_sixteen_cells(gpu_ctx, k):
    w = pfc.wide()
    window = pfc.WIDE_WINDOWS[k]
    assert pfc.run_of(window) == (16, 6, 15)[k]
    b = planned_batch(gpu_ctx, w, serial=k == 1)
    _long_runs(b, 0, window, w.nh, [(p, pfc.reference("wide", w, p)) for p in pfc.wide_probes(w)], 110)
    assert posefield.pose_field_stats(b)["cells"] > 0
    b.close()


def test_runs_of_sixteen_cells_over_a_kept_view(gpu_ctx):
    w = pfc.wide()
    og2, alive = pfc.wide_kept()
    b = planned_batch(gpu_ctx, w)
    gpu_ctx.set_grid(og2)
    assert np.array_equal(b.keep_pose_tree(0), alive) and 50 < alive.sum() < w.j - 50
    window = pfc.WIDE_WINDOWS[0]
    _long_runs(b, 0, window, w.nh, [(p, pfc.reference("wide kept", w, p, alive=alive, og8=og2)) for p in pfc.wide_probes(w)], 120)
    v = posefield.batch_pose_field(b, 0, window)[0]
    winners = np.unique(v[v >= 0])
    assert np.all(alive[winners]) and np.any((np.cumsum(alive) - 1)[winners] != winners) and posefield.pose_field_ms(b)[2] > 0.0
    b.close()


def test_runs_of_two_cells_on_the_whole_grid_of_a_workload_and_of_its_kept_view(gpu_ctx):
    k, window, f = pfc.kept()
    w = k.w
    whole = (0, 0) + w.og8.shape
    assert pfc.run_of(whole) == 2
    b = planned_batch(gpu_ctx, w)
    _long_runs(b, 0, whole, w.nh, [(window, pfc.workload(pfc.KEPT)[2])], 130)
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive)
    _long_runs(b, 0, whole, w.nh, [(window, f)], 140)
    b.close()


# ------------------------------------------------------------------------------------------------ refusals
def _refused(key, fn, *args, **fmt):
    refused_with_golden_text(GOLDEN, key, fn, *args, **fmt)


def test_refusals():
    w, window, f = pfc.workload("E")
    W, H = w.og8.shape
    nh = w.nh
    want = posefieldref.answer(f, -1)
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    _refused("no_plan", posefield.context_pose_field, ctx, window)
    _refused("no_plan_ms", posefield.pose_field_ms, ctx)
    _refused("no_plan_stats", posefield.pose_field_stats, ctx)
    b = _ffi.Batch(ctx, 2, w.n, dubins=True)
    _refused("unset", posefield.batch_pose_field, b, 0, window)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    _refused("set", posefield.batch_pose_field, b, 0, window)
    _refused("ms_none", posefield.pose_field_ms, b)
    _refused("stats_none", posefield.pose_field_stats, b)
    b.launch()
    b.sync()
    # the refusals of its own, each by code and text; none of them leaves a report behind, and a field call after each still answers
    L = posefield._lib()
    v, c, h = (np.zeros(window[2] * window[3], dtype=t) for t in (np.int32, np.float64, np.int32))

    def null(which):
        ptrs = [a.ctypes.data for a in (v, c, h)]
        ptrs[which] = None
        _ffi._check(ctx.handle, L.rrt_batch_pose_field(b._h, 0, *window, -1, *ptrs))

    first = True
    for key, call, fmt in (("q_high", lambda: posefield.batch_pose_field(b, 2, window), {}), ("q_negative", lambda: posefield.batch_pose_field(b, -1, window), {}),
                           ("w_zero", lambda: posefield.batch_pose_field(b, 0, (0, 0, 0, 5)), {}), ("h_zero", lambda: posefield.batch_pose_field(b, 0, (0, 0, 5, 0)), {}),
                           ("w_negative", lambda: posefield.batch_pose_field(b, 0, (0, 0, -1, 5)), {}),
                           ("past_x", lambda: posefield.batch_pose_field(b, 0, (W - 3, 0, 4, 4)), dict(x=W - 3, W=W, H=H)),
                           ("past_y", lambda: posefield.batch_pose_field(b, 0, (0, H - 3, 4, 4)), dict(y=H - 3, W=W, H=H)),
                           ("before_x", lambda: posefield.batch_pose_field(b, 0, (-1, 0, 4, 4)), dict(W=W, H=H)),
                           ("too_wide", lambda: posefield.batch_pose_field(b, 0, (0, 0, W + 1, H)), dict(w=W + 1, W=W, H=H)),
                           ("far_x", lambda: posefield.batch_pose_field(b, 0, (2 ** 31 - 2, 0, 4, 4)), dict(W=W, H=H)),
                           ("heading_high", lambda: posefield.batch_pose_field(b, 0, window, nh), dict(nh=nh)),
                           ("heading_low", lambda: posefield.batch_pose_field(b, 0, window, -2), dict(nh=nh)),
                           ("null", lambda: null(0), {}), ("null", lambda: null(1), {}), ("null", lambda: null(2), {})):
        _refused(key, call, **fmt)
        if first:  # before any field: a failed call leaves nothing to report on
            _refused("ms_none", posefield.pose_field_ms, b)
            _refused("stats_none", posefield.pose_field_stats, b)
            first = False
        posefieldref.same(posefield.batch_pose_field(b, 0, window), want)
        assert posefield.pose_field_stats(b)["cells"] == f.free.sum()
    assert L.rrt_batch_pose_field(None, 0, *window, -1, v.ctypes.data, c.ctypes.data, h.ctypes.data) == _ffi.RRT_E_ARG
    assert L.rrt_batch_pose_field_stats(b._h, None) == _ffi.RRT_E_ARG and L.rrt_plan_pose_field_ms(None, None) == _ffi.RRT_E_ARG
    # a refusal changes nothing: the reports are still those of the last call that ran
    small = (window[0], window[1], 2, 2)
    posefield.batch_pose_field(b, 0, small, 0)
    cells = posefield.pose_field_stats(b)["cells"]
    _refused("heading_high", posefield.batch_pose_field, b, 0, window, nh, nh=nh)
    assert posefield.pose_field_stats(b)["cells"] == cells == f.free[:2, :2].sum() and len(posefield.pose_field_ms(b)) == 4
    # armed again, and the grid replaced: connect_poses' refusals in the field's name
    before = snapshot(b.get_result(0))
    b.rearm()
    _refused("armed", posefield.batch_pose_field, b, 0, (0, 0, 0, 0))  # the unfinished query comes before the window
    b.launch()
    b.sync()
    assert same_snapshot(before, snapshot(b.get_result(0)))
    then = ctx.grid_generation()
    ctx.set_grid(w.og8)
    _refused("grid_replaced", posefield.batch_pose_field, b, 0, window, then=then, now=ctx.grid_generation())
    b.rearm()
    b.launch()
    b.sync()
    posefieldref.same(posefield.batch_pose_field(b, 0, window), want)
    b.close()
    # a straight-line batch: the field of cells is its call
    b = _ffi.Batch(ctx, 1, w.n)
    _refused("straight_batch", posefield.batch_pose_field, b, 5, window)
    q, keep = _ffi.make_query(1, w.n, w.xs[:2], w.xg[:2], w.samples, r2_rewire=w.r2)
    b.set_query(0, q)
    b.launch()
    b.sync()
    _refused("straight_batch", posefield.batch_pose_field, b, 0, window)
    b.close()
    ctx.close()
