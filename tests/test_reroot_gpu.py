"""GPU: a finished tree re-rooted at one of its vertices (rrt_reroot_*_kernel, rrt_batch_reroot / rrt_plan_reroot, _ffi.Batch.reroot /
Context.reroot, RRT.reroot), then grown on every launch shape a non-Informed query can take, and the tree calls on the result.

Every comparison is exact (==, array_equal, costs bit for bit).  The check is rerootref.py -- the path, the reversed edges walked by the
oracle, alive / depth by every vertex's own walk, the order, the costs summed from the root down -- followed by growref.grow."""
import ctypes

import numpy as np
import pytest

import goalref
import growref
import keepref
import oracle
import rerootref
import routeref
import treecalls as tc
from plannedcases import MAZE, NOISE, one_way_edges, oracle_planned, roots_behind
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd

pytestmark = pytest.mark.gpu


def _planned_tree(b, q, c):
    """query q planned on the device and equal to the oracle's plan; its tree"""
    keep = tc.set_case_query(b, q, c)
    b.launch()
    b.sync()
    res = b.get_result(q)
    ro = c["ro"]
    assert res.j == ro.j and np.array_equal(res.parent[:ro.j], ro.parent[:ro.j]) and np.array_equal(res.vcost[:ro.j].view(np.int64), ro.vcost[:ro.j].view(np.int64))
    return tc.tree_of(res)


def _restate(og8, prev, view, r, samples, c):
    R = rerootref.reroot(og8, prev[0], prev[1], prev[3], r, og8_view=og8 if view else None)
    return R, growref.grow(og8, c["alg"], c["n"], c["xg"], c["r2"], R.pts, R.vcost, R.parent, samples)


def _arm(b, q, r, samples, R):
    j0, old_id, log0 = b.reroot(q, r, samples)
    assert j0 == len(R.ids) == log0 and np.array_equal(old_id, R.ids)
    ms = b.reroot_ms()
    assert len(ms) == 8 and all(t >= 0.0 for t in ms)
    return log0


def _reroot(b, q, og8, prev, view, r, samples, c, shape=None):
    """one reroot of query q on map og8 at vertex r of the tree `prev` = (pts, parent, vcost, j), launched and checked against the
    restatement.  Returns (Rerooted, Grown, result)."""
    R, g = _restate(og8, prev, view, r, samples, c)
    log0 = _arm(b, q, r, samples, R)
    b.launch()
    b.sync()
    res = b.get_result(q)
    tc.same_result(res, g, log0)
    assert np.array_equal(res.pts[0], prev[0][r]) and res.vcost[0] == 0.0 and res.parent[0] == -1
    info = b.team_info()
    assert info["timeouts"] == 0 and b.team()[1] == 0, info
    if shape:
        tc.shape_ran(b, shape)  # (every caller that names its shape has a batch of one query)
    return R, g, res


NONE = np.zeros((0, 2), dtype=np.int32)


def _deepest(prev):
    return int(np.argmax(keepref.depth(prev[1], prev[3])))


def _mid(prev):
    leaf = _deepest(prev)
    way = rerootref.path_to_root(prev[1], prev[3], leaf)
    return way[len(way) // 2]


# ------------------------------------------------------------------------------------------------ 1. m = 0
@pytest.mark.parametrize("inp", [("noise200", 1, 300, 12), ("square100", 0, 200, 14)])
@pytest.mark.parametrize("which", ["root", "leaf", "mid"])
def test_plain_reroot_on_a_clean_tree(gpu_ctx, which, inp):
    c = oracle_planned(*inp)
    assert one_way_edges(c) == []
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    r = dict(root=0, leaf=_deepest(prev), mid=_mid(prev))[which]
    R, g, res = _reroot(b, 0, c["og8"], prev, False, r, NONE, c, "team")
    assert len(R.ids) == prev[3] and all(R.reversed_ok.values()) and R.d == keepref.depth(prev[1], prev[3])[r] and res.i_switch == c["n"]
    b.close()


@pytest.mark.parametrize("inp", [MAZE, NOISE])
def test_a_root_behind_a_one_way_edge_cuts_the_far_side(gpu_ctx, inp):
    c = oracle_planned(*inp)
    edges = one_way_edges(c)
    roots = roots_behind(c, edges)
    assert edges and roots
    ro = c["ro"]
    r = max(roots, key=lambda v: len(rerootref.path_to_root(ro.parent, ro.j, v)))  # the deepest of them
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    R, g, res = _reroot(b, 0, c["og8"], prev, False, r, NONE, c, "team")
    assert not all(R.reversed_ok.values()) and 1 <= len(R.ids) < prev[3] - 1 and res.j == len(R.ids)
    b.close()


# ------------------------------------------------------------------------------------------------ 2. shapes that can break a stage
def test_trees_of_exactly_1_2_63_to_65_and_1023_to_1025_vertices(gpu_ctx):
    cs = []
    for k in tc.SIZES:
        og8, xs, samples, n = tc.sized(k, 100 + k)
        if k != 1:
            cs.append(tc.oracle_case(og8, 0, n, xs, (63, 63), samples, 0))
    b = tc.shaped_batch(gpu_ctx, cs[0], "team", Q=len(cs), n_cap=1040)
    prevs = [None] * len(cs)
    for q, c in enumerate(cs):
        tc.set_case_query(b, q, c)
    b.launch()
    b.sync()
    armed = []
    for q, c in enumerate(cs):
        prev = tc.tree_of(b.get_result(q))
        assert prev[3] == c["ro"].j == tc.SIZES[q + 1]
        r = _deepest(prev)
        R, g = _restate(c["og8"], prev, False, r, NONE, c)
        armed.append((g, _arm(b, q, r, NONE, R)))
    b.launch()
    b.sync()
    for q, (g, log0) in enumerate(armed):
        tc.same_result(b.get_result(q), g, log0)
    b.close()
    # the tree of one vertex: the start boxed in
    og8, xs, samples, n = tc.sized(1, 101)
    c = tc.oracle_case(og8, 0, n, xs, (63, 63) if tuple(xs) != (63, 63) else (0, 0), samples, 0)
    assert c["ro"].j == 1
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    R, g, res = _reroot(b, 0, og8, prev, False, 0, NONE, c)
    assert res.j == 1 and len(R.ids) == 1
    b.close()


def test_a_chain_of_1100_vertices_rerooted_at_its_far_end(gpu_ctx):
    """depth above one workgroup's width: 1099 reversed edges, 1100 levels"""
    og8 = np.zeros((1104, 1104), dtype=np.uint8)
    chain = np.stack([np.arange(1, 1100), np.arange(1, 1100)], axis=1)
    samples = np.concatenate([chain, np.tile(chain[:1], (9, 1))])
    c = tc.oracle_case(og8, 0, 1108, (0, 0), (1103, 0), samples, 0)
    ro = c["ro"]
    assert ro.j == 1100 and np.array_equal(ro.parent[1:1100], np.arange(1099))
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    R, g, res = _reroot(b, 0, og8, prev, False, 1099, NONE, c)
    assert R.d == 1099 and np.array_equal(R.ids, np.arange(1099, -1, -1)) and np.array_equal(res.parent[1:1100], np.arange(1099))
    b.close()


def test_a_star_with_one_level_of_2000_vertices(gpu_ctx):
    """a level wider than the cost kernel's workgroup: every sample hangs on the start; re-rooted at the start and at a leaf"""
    og8 = np.zeros((101, 101), dtype=np.uint8)
    vec = [(dx, dy) for dx in range(-50, 51) for dy in range(-50, 51) if np.gcd(dx, dy) == 1]  # no lattice point between it and the start
    rays = np.array(vec, dtype=np.int64)[np.random.default_rng(7).permutation(len(vec))[:2000]] + 50
    samples = np.concatenate([rays, np.tile(rays[:1], (9, 1))])
    c = tc.oracle_case(og8, 1, 2009, (50, 50), (100, 100), samples, hostprep.radius_threshold(80))
    ro = c["ro"]
    assert ro.j == 2001 and (ro.parent[1:2001] == 0).all()
    b = tc.shaped_batch(gpu_ctx, c, "team", Q=2)
    prevs = [_planned_tree(b, q, c) for q in range(2)]
    out = []
    for q, r in enumerate((0, 1000)):
        R, g = _restate(og8, prevs[q], False, r, NONE, c)
        out.append((R, g, _arm(b, q, r, NONE, R)))
    b.launch()
    b.sync()
    for q, (R, g, log0) in enumerate(out):
        tc.same_result(b.get_result(q), g, log0)
    assert (out[0][0].depth == 1).sum() == 2000 and (out[1][0].depth == 2).sum() == 1999
    b.close()


# ------------------------------------------------------------------------------------------------ 3. after keep_tree
def test_a_kept_view_is_rerooted_in_the_callers_numbers(gpu_ctx):
    c = tc.base()
    w = tc.wall(c)
    og2 = w["og2"]
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    gpu_ctx.set_grid(og2)
    assert np.array_equal(b.keep_tree(0), w["alive"])
    alive = np.flatnonzero(w["alive"])
    dep = keepref.depth(prev[1], prev[3])
    r = int(alive[np.argmax(dep[alive])])
    dead = int(np.flatnonzero(~w["alive"])[0])
    assert r != np.flatnonzero(w["ids"] == r)[0]  # its number in the view is another one: the caller's number is what the call takes
    goals = tc.mixed_goals(og2)
    before = b.connect_goals(0, goals)
    msg = tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, dead))
    assert f"root={dead} is not alive" in msg
    after = b.connect_goals(0, goals)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])  # the view stands
    R, g, res = _reroot(b, 0, og2, prev, True, r, NONE, c, "team")
    assert len(R.ids) <= len(alive) and set(R.ids.tolist()) <= set(alive.tolist()) and R.d == dep[r] > 3
    tc.goals_and_routes(b, 0, og2, res)
    b.close()


# ------------------------------------------------------------------------------------------------ 4. m > 0 on every launch shape
@pytest.mark.parametrize("shape", list(tc.SHAPES))
def test_reroot_then_grow_on_every_launch_shape(gpu_ctx, shape):
    c = tc.base()
    ro = c["ro"]
    m = min(c["n"] - ro.j, 150)
    assert ro.j > 1000 and m >= 100
    more = hostprep.draw_free_samples(np.random.default_rng(33), np.argwhere(c["og8"] == 0), m)
    more[3] = ro.pts[0]  # the old start drawn again: its cell is a vertex's now, so it is refused
    b = tc.shaped_batch(gpu_ctx, c, shape)
    prev = _planned_tree(b, 0, c)
    r = _mid(prev)
    R, g, res = _reroot(b, 0, c["og8"], prev, False, r, more, c, shape)
    assert g.j > g.j0 + 20 and not g.accept_log[3] and R.d >= 3
    b.close()


# ------------------------------------------------------------------------------------------------ 5. afterwards
def test_the_tree_calls_answer_on_the_rerooted_tree(gpu_ctx):
    c = tc.base()
    og8 = c["og8"]
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    r = _mid(prev)
    R, g, res = _reroot(b, 0, og8, prev, False, r, NONE, c)
    cur = tc.tree_of(res)
    tc.goals_and_routes(b, 0, og8, res)  # connect_goals, and routes with shortcuts
    goals = tc.mixed_goals(og8)
    for x, y in zip(b.routes(0, goals), routeref.routes(og8, cur[0], cur[2], cur[1], cur[3], goals, cut=False)):
        assert np.array_equal(x, y)  # raw routes: they begin at the new start
    # rearm + launch plans from the new start
    b.rearm()
    b.launch()
    b.sync()
    st, rn = oracle.plan(og8, c["n"], c["alg"], prev[0][r], c["xg"], c["samples"], r2_rewire=c["r2"])
    again = b.get_result(0)
    live = rn.j + rn.found
    assert again.j == rn.j and again.found == rn.found and np.array_equal(again.pts[:live], rn.pts[:live]) and np.array_equal(again.parent[:live], rn.parent[:live])
    assert np.array_equal(again.vcost[:live].view(np.int64), rn.vcost[:live].view(np.int64)) and np.array_equal(again.pts[0], prev[0][r])
    # a second reroot, a keep_tree on another map, and a grow behind it
    cur = tc.tree_of(again)
    R2, g2, res2 = _reroot(b, 0, og8, cur, False, _deepest(cur), NONE, c)
    cur = tc.tree_of(res2)
    w = tc.wall(c)
    gpu_ctx.set_grid(w["og2"])
    alive = b.keep_tree(0)
    assert np.array_equal(alive, keepref.alive(w["og2"], cur[0], cur[1], cur[3]))
    if alive[0]:
        m = min(c["n"] - int(alive.sum()), 120)
        g3, res3 = tc.grow_checked(b, 0, w["og2"], cur, True, hostprep.draw_free_samples(np.random.default_rng(8), np.argwhere(w["og2"] == 0), m), c, "team")
        tc.goals_and_routes(b, 0, w["og2"], res3, connected=0)
    b.close()


def test_only_the_last_seed_calls_stage_times_answer(gpu_ctx):
    """grow_ms is the last grow's alone: after a reroot or a relax the seed's times are that call's, which reroot_ms / relax_ms report.
    (Every reroot and relax sequence of tests/test_tree_sequences_gpu.py meets it at its first reroot or relax that runs: grow_ms
    answered with that call's seed.)"""
    og8, xs, samples, n = tc.sized(65, 165)
    c = tc.oracle_case(og8, 0, n, xs, (63, 63), samples, 0)
    b = tc.shaped_batch(gpu_ctx, c, "team")
    _planned_tree(b, 0, c)

    def answers():
        out = set()
        for name, call in (("grow", b.grow_ms), ("reroot", b.reroot_ms), ("relax", b.relax_ms), ("stats", b.relax_stats)):
            try:
                call()
                out.add(name)
            except _ffi.RRTError as e:
                assert e.code == _ffi.RRT_E_ARG, e
        return out

    assert answers() == set()
    for call, want in ((lambda: b.grow(0, NONE), {"grow"}), (lambda: b.reroot(0, 7), {"reroot"}), (lambda: b.relax(0, tc.R2), {"relax", "stats"}),
                       (lambda: b.reroot(0, 3), {"reroot"}), (lambda: b.grow(0, NONE), {"grow"})):
        call()
        assert answers() == want
        tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 65))  # a refusal changes nothing
        assert answers() == want
        b.launch()
        b.sync()
        assert answers() == want
    b.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def _stands(answer, goals, before):
    after = answer(goals)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_batch_refusals_change_nothing(gpu_ctx):
    c = tc.base()
    w = tc.wall(c)
    b = tc.shaped_batch(gpu_ctx, c, "pipe1")
    tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 0))  # no query set
    tc.set_case_query(b, 0, c)
    assert "has not finished" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 0))  # not launched
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    goals = tc.mixed_goals(c["og8"])
    ans0 = b.connect_goals(0, goals)
    j0, log0 = ctypes.c_int32(-1), ctypes.c_int32(-1)
    L = _ffi.lib()
    assert L.rrt_batch_reroot(b._h, 0, 0, None, -1, ctypes.byref(j0), None, ctypes.byref(log0)) == _ffi.RRT_E_ARG
    assert (j0.value, log0.value) == (-1, -1) and b"m=-1" in L.rrt_last_error_string(gpu_ctx.handle)
    assert L.rrt_batch_reroot(b._h, 0, 0, None, 0, None, None, ctypes.byref(log0)) == _ffi.RRT_E_ARG  # NULL j0
    room = c["n"] - r0.j
    assert "q=1 of 1" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(1, 0))
    assert f"room for {room}" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 0, c["samples"][:room + 1]))
    for bad in (-1, r0.j, r0.j + 5):
        assert f"root={bad}, query 0 has the vertices [0, {r0.j})" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, bad))
    assert "outside the" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 0, np.array([(5, 5), (200, 5)])))
    _stands(lambda g: b.connect_goals(0, g), goals, ans0)
    # a new grid without keep_tree
    gpu_ctx.set_grid(w["og2"])
    assert "was not kept on it (rrt_batch_keep_tree)" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 0))
    # the root blocked: an empty view
    og3 = w["og2"].copy()
    og3[c["xs"][0], c["xs"][1]] = 1
    gpu_ctx.set_grid(og3)
    assert not b.keep_tree(0).any()
    v0 = b.connect_goals(0, goals)
    assert "root is blocked" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, 0))
    _stands(lambda g: b.connect_goals(0, g), goals, v0)
    # a root that the wall cut
    gpu_ctx.set_grid(w["og2"])
    assert np.array_equal(b.keep_tree(0), w["alive"])
    v1 = b.connect_goals(0, goals)
    dead = int(np.flatnonzero(~w["alive"])[-1])
    assert f"root={dead} is not alive" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.reroot(0, dead))
    _stands(lambda g: b.connect_goals(0, g), goals, v1)
    # after all these refusals the tree is what it was
    gpu_ctx.set_grid(c["og8"])
    assert b.keep_tree(0).all()
    r1 = b.get_result(0)
    assert np.array_equal(r1.pts, r0.pts) and np.array_equal(r1.vcost.view(np.int64), r0.vcost.view(np.int64)) and np.array_equal(r1.parent, r0.parent)
    _stands(lambda g: b.connect_goals(0, g), goals, ans0)
    with pytest.raises(_ffi.RRTError):
        b.reroot_ms()  # no reroot on this batch yet
    b.close()
    # what the batch cannot re-root
    for kw, why in ((dict(rewire=True), "RRT_FLAG_REWIRE"), (dict(dubins=True), "a Dubins word is not reversible"), (dict(large_grid=True), "RRT_FLAG_LARGE_GRID")):
        bb = _ffi.Batch(gpu_ctx, 1, 100, **kw)
        assert why in tc.refused_with_code(_ffi.RRT_E_UNSUPPORTED, lambda: bb.reroot(0, 0))
        bb.close()
    # an Informed query
    b = _ffi.Batch(gpu_ctx, 1, 300, logs=True)
    Cm = hostprep.rotation_to_world_frame(np.asarray(c["xs"], dtype=np.int64), np.asarray(c["xg"], dtype=np.int64))
    qu, keep = _ffi.make_query(2, 300, c["xs"], c["xg"], c["samples"][:300], r2_rewire=c["r2"], goal_d2=0, Cmat=Cm)
    b.set_query(0, qu)
    b.launch()
    b.sync()
    ansi = b.connect_goals(0, goals)
    assert "Informed" in tc.refused_with_code(_ffi.RRT_E_UNSUPPORTED, lambda: b.reroot(0, 0))
    _stands(lambda g: b.connect_goals(0, g), goals, ansi)
    b.close()


def test_plan_refusals_change_nothing():
    c = tc.base()
    w = tc.wall(c)
    ctx = _ffi.Context(0)
    ctx.set_grid(c["og8"])
    n = c["n"]

    def refused(code, root, samples=NONE):
        with pytest.raises(_ffi.RRTError) as e:
            ctx.reroot(root, samples, n)
        assert e.value.code == code and not e.value.seeded, e.value
        return str(e.value)

    assert "no rrt_plan on this context yet" in refused(_ffi.RRT_E_ARG, 0)
    goals = tc.mixed_goals(c["og8"])
    Cm = hostprep.rotation_to_world_frame(np.asarray(c["xs"], dtype=np.int64), np.asarray(c["xg"], dtype=np.int64))
    qi, keepi = _ffi.make_query(2, 300, c["xs"], c["xg"], c["samples"][:300], r2_rewire=c["r2"], goal_d2=0, Cmat=Cm)
    ctx.plan(qi, 300, logs=True)
    assert "Informed" in refused(_ffi.RRT_E_UNSUPPORTED, 0)
    qu, keep = _ffi.make_query(c["alg"], n, c["xs"], c["xg"], c["samples"], r2_rewire=c["r2"])
    ctx.plan(qu, n, rewire=True)
    assert "RRT_FLAG_REWIRE" in refused(_ffi.RRT_E_UNSUPPORTED, 0)
    rc, res = ctx.plan(qu, n)
    ans0 = ctx.connect_goals(goals)
    room = n - res.j
    assert f"room for {room}" in refused(_ffi.RRT_E_ARG, 0, c["samples"][:room + 1])
    assert f"root={res.j}, query 0 has the vertices [0, {res.j})" in refused(_ffi.RRT_E_ARG, res.j)
    assert "root=-1" in refused(_ffi.RRT_E_ARG, -1)
    assert "outside the" in refused(_ffi.RRT_E_ARG, 0, np.array([(5, 5), (200, 5)]))
    j0 = ctypes.c_int32(-1)
    assert _ffi.lib().rrt_plan_reroot(ctx.handle, 0, None, -1, ctypes.byref(j0), None, ctypes.byref(res.c)) == _ffi.RRT_E_ARG and j0.value == -1
    assert _ffi.lib().rrt_plan_reroot(ctx.handle, 0, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    _stands(ctx.connect_goals, goals, ans0)
    ctx.set_grid(w["og2"])
    assert "was not kept on it" in refused(_ffi.RRT_E_ARG, 0)
    assert np.array_equal(ctx.keep_tree(), w["alive"])
    v1 = ctx.connect_goals(goals)
    dead = int(np.flatnonzero(~w["alive"])[0])
    assert f"root={dead} is not alive" in refused(_ffi.RRT_E_ARG, dead)
    _stands(ctx.connect_goals, goals, v1)
    og3 = w["og2"].copy()
    og3[c["xs"][0], c["xs"][1]] = 1
    ctx.set_grid(og3)
    assert not ctx.keep_tree().any()
    assert "root is blocked" in refused(_ffi.RRT_E_ARG, 0)
    # and the call itself, on the kept view, equals the restatement
    ctx.set_grid(w["og2"])
    ctx.keep_tree()
    prev = tc.tree_of(res)
    alive = np.flatnonzero(w["alive"])
    r = int(alive[np.argmax(keepref.depth(prev[1], prev[3])[alive])])
    R, g = _restate(w["og2"], prev, True, r, NONE, c)
    rc, out, j0, old_id = ctx.reroot(r, NONE, n)
    assert j0 == len(R.ids) and np.array_equal(old_id, R.ids) and len(ctx.reroot_ms()) == 8
    tc.same_result(out, g)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. the class
def test_rrtstar_reroot_is_the_restatement_fed_with_the_same_draws():
    c = tc.base()
    og = c["og8"].astype(np.int64)
    N = tc.N
    p = amd.RRTStar(og, N, tc.RR, pbar=False, seed=3)
    with pytest.raises(RuntimeError):
        p.reroot(3)
    T, gv = p.plan(c["xs"], c["xg"])
    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    prev = (np.array(points), np.array(parent), np.array(vcosts), j)
    state = p.rand_gen.bit_generator.state
    with pytest.raises(ValueError, match=f"reroot: root={j}, query 0 has the vertices"):
        p.reroot(j, 5)
    assert p.rand_gen.bit_generator.state == state and p._tree_resident == "device"  # a refused vertex spends no draws and leaves the tree
    with pytest.raises(ValueError, match=f"room for {N - j} more"):
        p.reroot(3, N - j + 1)
    # a vehicle three legs along the route to the goal
    routes, _ = p.routes_to([c["xg"]])
    v0, _ = p.connect_goals([c["xg"]])
    way = rerootref.path_to_root(prev[1], j, int(v0[0]))[::-1]
    assert len(way) > 4 and np.array_equal(routes[0][3], prev[0][way[3]])
    r, m = way[3], min(N - j, 120)
    twin = np.random.default_rng(0)
    twin.bit_generator.state = p.rand_gen.bit_generator.state
    samples = hostprep.draw_free_samples(twin, np.argwhere(og == 0), m)
    R, g = _restate(c["og8"], prev, False, r, samples, c)
    T2, gv2 = p.reroot(r, m)
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state
    assert np.array_equal(p.last_grow_ids, R.ids) and p.last_route == "kernel" and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j
    vg, pts2, par2, vc2 = T2.__dict__["_lazy"]
    live = g.j + g.found
    assert gv2 == vg == g.vgoal and len(pts2) == g.rows and len(par2) == live
    assert np.array_equal(pts2[:live], g.pts[:live]) and np.array_equal(par2, g.parent[:live])
    assert np.array_equal(np.asarray(vc2[:live]).view(np.int64), g.vcost[:live].view(np.int64))
    tc.class_goals_and_routes(p, c["og8"], g, tc.mixed_goals(c["og8"]))
    # a further reroot and a grow on the re-rooted tree
    cur = (g.pts, g.parent, g.vcost, g.j)
    r2 = _deepest(cur)
    R3, g3 = _restate(c["og8"], cur, False, r2, NONE, c)
    T3, gv3 = p.reroot(r2)
    assert np.array_equal(p.last_grow_ids, R3.ids) and np.array_equal(T3.__dict__["_lazy"][2], g3.parent[:g3.j + g3.found])
    T4, gv4 = p.grow(0)
    assert np.array_equal(p.last_grow_ids, np.arange(g3.j)) and np.array_equal(T4.__dict__["_lazy"][2], g3.parent[:g3.j + g3.found])


def test_the_classes_that_do_not_reroot():
    c = tc.base()
    og = c["og8"].astype(np.int64)
    for p in (amd.RRTStarInformed(og, tc.N, tc.RR, 10, pbar=False), amd.RRTStar(og, tc.N, tc.RR, pbar=False, rewire="correct")):
        try:
            p.plan(c["xs"], c["xg"])
        except IndexError:  # (the plan's own goal not reached: the tree is resident all the same)
            pass
        with pytest.raises(ValueError, match="reroot"):
            p.reroot(5)
        assert p._tree_resident == "device"  # the refusal left the tree
