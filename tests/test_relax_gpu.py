"""GPU: a finished tree relaxed to shortest paths over its r-disc (rrt_relax_*_kernel, rrt_batch_relax / rrt_plan_relax,
_ffi.Batch.relax / Context.relax, RRT.relax), then grown, and the tree calls on the result.

Every comparison is exact (==, array_equal, costs bit for bit).  The check is relaxref.py -- the candidate edges walked by the oracle
from u to v, Dijkstra's costs, the parent rule, the order, the costs summed from the root down -- followed by growref.grow; and
relaxref.certify on the arrays the device returned.  The inputs are those of relaxcases.py; test_relax_cpu.py says what each is for."""
import ctypes

import numpy as np
import pytest

import growref
import keepref
import oracle
import relaxcases as rc
import relaxref
import rerootref
import routeref
import treecalls as tc
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd

pytestmark = pytest.mark.gpu

NONE = np.zeros((0, 2), dtype=np.int32)


def _planned_tree(b, q, c):
    """query q planned on the device and equal to the oracle's plan; its tree"""
    tc.set_case_query(b, q, c)
    b.launch()
    b.sync()
    return _same_as_oracle(b.get_result(q), c)


def _same_as_oracle(res, c):
    ro = c["ro"]
    assert res.j == ro.j and np.array_equal(res.parent[:ro.j], ro.parent[:ro.j]) and np.array_equal(res.vcost[:ro.j].view(np.int64), ro.vcost[:ro.j].view(np.int64))
    return tc.tree_of(res)


def _restate(og8, prev, view, r, samples, c, X=None):
    if X is None:
        X = relaxref.relax(og8, prev[0], prev[1], prev[2], prev[3], rc.R_of(r), og8_view=og8 if view else None)
    return X, growref.grow(og8, c["alg"], c["n"], c["xg"], c["r2"], X.pts, X.vcost, X.parent, samples)


def _arm(b, q, r, samples, X):
    j0, old_id, log0 = b.relax(q, rc.R_of(r), samples)
    assert j0 == len(X.ids) == log0 and np.array_equal(old_id, X.ids), (j0, len(X.ids), log0, tc.differ(old_id, X.ids))
    ms, st = b.relax_ms(), b.relax_stats()
    assert len(ms) == 9 and all(t >= 0.0 for t in ms)
    assert st["fell"] == X.fell and 1 <= st["rounds"] <= max(j0, 1) and st["los"] >= 0 and st["priced"] >= 0, (st, X.fell)
    return log0


def _relax(b, q, og8, prev, view, r, samples, c, shape=None, X=None):
    """one relax of query q on map og8 of the tree `prev` = (pts, parent, vcost, j), launched and checked against the restatement
    and by the certificate.  Returns (Relaxed, Grown, result)."""
    X, g = _restate(og8, prev, view, r, samples, c, X)
    log0 = _arm(b, q, r, samples, X)
    b.launch()
    b.sync()
    res = b.get_result(q)
    tc.same_result(res, g, log0)
    info = b.team_info()
    assert info["timeouts"] == 0 and b.team()[1] == 0, info
    if shape:
        tc.shape_ran(b, shape)  # (every caller that names its shape has a batch of one query)
    if len(samples) == 0:  # the device's own arrays, by rules of their own
        j0 = len(X.ids)
        assert relaxref.certify(og8, res.pts[:j0], res.parent[:j0], res.vcost[:j0], rc.R_of(r), relaxref.old_edges_of(X.in_parent, X.order)) == []
    return X, g, res


# ------------------------------------------------------------------------------------------------ 1. sizes and crafted inputs
def test_trees_of_exactly_1_2_63_to_65_and_1023_to_1025_vertices(gpu_ctx):
    cs = [rc.sized(k) for k in tc.SIZES if k != 1]
    b = tc.shaped_batch(gpu_ctx, cs[0], "team", Q=len(cs), n_cap=1040)
    for q, c in enumerate(cs):
        tc.set_case_query(b, q, c)
    b.launch()
    b.sync()
    armed = []
    for q, c in enumerate(cs):
        prev = _same_as_oracle(b.get_result(q), c)
        assert prev[3] == tc.SIZES[q + 1]
        X, g = _restate(c["og8"], prev, False, tc.RR, NONE, c, rc.relaxed(c, tc.RR))
        armed.append((g, _arm(b, q, tc.RR, NONE, X)))
    b.launch()
    b.sync()
    for q, (g, log0) in enumerate(armed):
        tc.same_result(b.get_result(q), g, log0)
    b.close()
    c = rc.sized(1)  # the tree of one vertex: the start boxed in
    assert c["ro"].j == 1
    b = tc.shaped_batch(gpu_ctx, c, "team")
    X, g, res = _relax(b, 0, c["og8"], _planned_tree(b, 0, c), False, tc.RR, NONE, c)
    assert res.j == 1 and X.fell == 0 and b.relax_stats()["rounds"] == 1
    b.close()


@pytest.mark.parametrize("name", list(rc.FIXTURES))
def test_the_crafted_inputs(gpu_ctx, name):
    c, r, X = rc.fixture(name)
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    _relax(b, 0, c["og8"], prev, False, r, NONE, c, X=X)
    print(name, b.relax_stats(), b.relax_ms())  # (the rounds are the implementation's: only 1 <= rounds <= j is asserted, in _arm)
    b.close()


@pytest.mark.parametrize("alg", [0, 1])
def test_the_noise_map_for_rrtstandard_and_rrtstar(gpu_ctx, alg):
    c = rc.base(alg)
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    X, g, res = _relax(b, 0, c["og8"], prev, False, tc.RR, NONE, c, "team", X=rc.relaxed(c, tc.RR))
    assert X.fell > prev[3] // 2 and X.ties >= 1 and res.i_switch == c["n"]
    b.close()


# ------------------------------------------------------------------------------------------------ 2. after keep_tree
def test_a_kept_view_is_relaxed_among_its_alive_vertices(gpu_ctx):
    c = tc.base()
    w = tc.wall(c)
    og2 = w["og2"]
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    gpu_ctx.set_grid(og2)
    assert np.array_equal(b.keep_tree(0), w["alive"]) and not w["alive"].all()
    X, g, res = _relax(b, 0, og2, prev, True, tc.RR, NONE, c, "team", X=rc.relaxed(c, tc.RR, og2, True))
    assert set(X.ids.tolist()) == set(np.flatnonzero(w["alive"]).tolist()) and not np.array_equal(X.ids, np.arange(len(X.ids)))
    tc.goals_and_routes(b, 0, og2, res)
    b.close()


# ------------------------------------------------------------------------------------------------ 3. with reroot
def test_reroot_then_relax_and_relax_then_reroot(gpu_ctx):
    c = tc.base()
    og8 = c["og8"]
    b = tc.shaped_batch(gpu_ctx, c, "team", Q=2)
    prevs = [_planned_tree(b, q, c) for q in range(2)]
    r = prevs[0][3] // 2
    # query 0: reroot, then relax
    Z = rerootref.reroot(og8, prevs[0][0], prevs[0][1], prevs[0][3], r)
    gz = growref.grow(og8, c["alg"], c["n"], c["xg"], c["r2"], Z.pts, Z.vcost, Z.parent, NONE)
    j0, old_id, log0 = b.reroot(0, r)
    assert j0 == len(Z.ids) and np.array_equal(old_id, Z.ids)
    b.launch()
    b.sync()
    res = b.get_result(0)
    tc.same_result(res, gz, log0)
    X, g, res = _relax(b, 0, og8, tc.tree_of(res), False, tc.RR, NONE, c)
    assert X.vcost.mean() < Z.vcost[:len(X.ids)].mean() and np.array_equal(res.pts[0], prevs[0][0][r]) and res.vcost[0] == 0.0
    with pytest.raises(_ffi.RRTError):
        b.reroot_ms()  # the stage times are the relax call's now
    # query 1: relax, then reroot
    X1, g1, res1 = _relax(b, 1, og8, prevs[1], False, tc.RR, NONE, c, X=rc.relaxed(c, tc.RR))
    cur = tc.tree_of(res1)
    r1 = int(np.argmax(keepref.depth(cur[1], cur[3])))
    Z1 = rerootref.reroot(og8, cur[0], cur[1], cur[3], r1)
    g2 = growref.grow(og8, c["alg"], c["n"], c["xg"], c["r2"], Z1.pts, Z1.vcost, Z1.parent, NONE)
    j0, old_id, log0 = b.reroot(1, r1)
    assert j0 == len(Z1.ids) and np.array_equal(old_id, Z1.ids)
    b.launch()
    b.sync()
    tc.same_result(b.get_result(1), g2, log0)
    with pytest.raises(_ffi.RRTError):
        b.relax_ms()
    with pytest.raises(_ffi.RRTError):
        b.relax_stats()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. m > 0
@pytest.mark.parametrize("shape", ["team", "pipe1"])
def test_relax_then_grow_on_a_team_and_on_one_cu(gpu_ctx, shape):
    c = tc.base()
    ro = c["ro"]
    m = min(c["n"] - ro.j, 120)
    assert m >= 100
    more = hostprep.draw_free_samples(np.random.default_rng(34), np.argwhere(c["og8"] == 0), m)
    more[3] = ro.pts[5]  # a vertex's cell drawn again: refused
    b = tc.shaped_batch(gpu_ctx, c, shape)
    prev = _planned_tree(b, 0, c)
    X, g, res = _relax(b, 0, c["og8"], prev, False, tc.RR, more, c, shape, X=rc.relaxed(c, tc.RR))
    assert g.j > g.j0 + 20 and not g.accept_log[3] and b.team()[1] == 0
    b.close()


# ------------------------------------------------------------------------------------------------ 5. afterwards
def test_the_tree_calls_answer_on_the_relaxed_tree(gpu_ctx):
    c = tc.base()
    og8 = c["og8"]
    b = tc.shaped_batch(gpu_ctx, c, "team")
    prev = _planned_tree(b, 0, c)
    X, g, res = _relax(b, 0, og8, prev, False, tc.RR, NONE, c, X=rc.relaxed(c, tc.RR))
    cur = tc.tree_of(res)
    tc.goals_and_routes(b, 0, og8, res)  # connect_goals, and routes with shortcuts
    goals = tc.mixed_goals(og8)
    for x, y in zip(b.routes(0, goals), routeref.routes(og8, cur[0], cur[2], cur[1], cur[3], goals, cut=False)):
        assert np.array_equal(x, y)  # raw routes
    # a second relax finds nothing to lower
    X2, g2, res2 = _relax(b, 0, og8, cur, False, tc.RR, NONE, c)
    assert X2.fell == 0 and b.relax_stats()["fell"] == 0 and b.relax_stats()["rounds"] == 1
    assert np.array_equal(np.sort(res2.vcost[:cur[3]]).view(np.int64), np.sort(cur[2][:cur[3]]).view(np.int64))
    # rearm + launch still plans from xstart
    b.rearm()
    b.launch()
    b.sync()
    cur = _same_as_oracle(b.get_result(0), c)
    assert np.array_equal(cur[0][0], c["xs"])
    # relax, a keep_tree on another map, and a grow behind it
    X3, g3, res3 = _relax(b, 0, og8, cur, False, tc.RR, NONE, c, X=rc.relaxed(c, tc.RR))
    cur = tc.tree_of(res3)
    w = tc.wall(c)
    gpu_ctx.set_grid(w["og2"])
    alive = b.keep_tree(0)
    assert np.array_equal(alive, keepref.alive(w["og2"], cur[0], cur[1], cur[3])) and alive[0]
    m = min(c["n"] - int(alive.sum()), 120)
    g4, res4 = tc.grow_checked(b, 0, w["og2"], cur, True, hostprep.draw_free_samples(np.random.default_rng(8), np.argwhere(w["og2"] == 0), m), c, "team")
    tc.goals_and_routes(b, 0, w["og2"], res4, connected=0)
    b.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def _stands(answer, goals, before):
    after = answer(goals)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_batch_refusals_change_nothing(gpu_ctx):
    c = tc.base()
    w = tc.wall(c)
    R = tc.R2
    b = tc.shaped_batch(gpu_ctx, c, "pipe1")
    tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, R))  # no query set
    tc.set_case_query(b, 0, c)
    assert "has not finished" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, R))  # not launched
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    goals = tc.mixed_goals(c["og8"])
    ans0 = b.connect_goals(0, goals)
    j0, log0 = ctypes.c_int32(-1), ctypes.c_int32(-1)
    L = _ffi.lib()
    assert L.rrt_batch_relax(b._h, 0, R, None, -1, ctypes.byref(j0), None, ctypes.byref(log0)) == _ffi.RRT_E_ARG
    assert (j0.value, log0.value) == (-1, -1) and b"m=-1" in L.rrt_last_error_string(gpu_ctx.handle)
    assert L.rrt_batch_relax(b._h, 0, R, None, 0, None, None, ctypes.byref(log0)) == _ffi.RRT_E_ARG  # NULL j0
    room = c["n"] - r0.j
    assert "q=1 of 1" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(1, R))
    assert f"room for {room}" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, R, c["samples"][:room + 1]))
    for bad in (0, -5):
        assert f"r2={bad}" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, bad))
    assert f"room for {room}" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, 0, c["samples"][:room + 1]))  # the room comes first
    assert "outside the" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, R, np.array([(5, 5), (200, 5)])))
    _stands(lambda g: b.connect_goals(0, g), goals, ans0)
    # a new grid without keep_tree
    gpu_ctx.set_grid(w["og2"])
    assert "was not kept on it (rrt_batch_keep_tree)" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, R))
    # the root blocked: an empty view
    og3 = w["og2"].copy()
    og3[c["xs"][0], c["xs"][1]] = 1
    gpu_ctx.set_grid(og3)
    assert not b.keep_tree(0).any()
    v0 = b.connect_goals(0, goals)
    assert "root is blocked" in tc.refused_with_code(_ffi.RRT_E_ARG, lambda: b.relax(0, R))
    _stands(lambda g: b.connect_goals(0, g), goals, v0)
    # after all these refusals the tree is what it was
    gpu_ctx.set_grid(c["og8"])
    assert b.keep_tree(0).all()
    r1 = b.get_result(0)
    assert np.array_equal(r1.pts, r0.pts) and np.array_equal(r1.vcost.view(np.int64), r0.vcost.view(np.int64)) and np.array_equal(r1.parent, r0.parent)
    _stands(lambda g: b.connect_goals(0, g), goals, ans0)
    with pytest.raises(_ffi.RRTError):
        b.relax_ms()  # no relax on this batch yet
    with pytest.raises(_ffi.RRTError):
        b.relax_stats()
    b.close()
    # what the batch cannot relax
    for kw, why in ((dict(rewire=True), "RRT_FLAG_REWIRE"), (dict(dubins=True), "depends on the headings"), (dict(large_grid=True), "RRT_FLAG_LARGE_GRID")):
        bb = _ffi.Batch(gpu_ctx, 1, 100, **kw)
        assert why in tc.refused_with_code(_ffi.RRT_E_UNSUPPORTED, lambda: bb.relax(0, R))
        bb.close()
    # an Informed query
    b = _ffi.Batch(gpu_ctx, 1, 300, logs=True)
    Cm = hostprep.rotation_to_world_frame(np.asarray(c["xs"], dtype=np.int64), np.asarray(c["xg"], dtype=np.int64))
    qu, keep = _ffi.make_query(2, 300, c["xs"], c["xg"], c["samples"][:300], r2_rewire=c["r2"], goal_d2=0, Cmat=Cm)
    b.set_query(0, qu)
    b.launch()
    b.sync()
    ansi = b.connect_goals(0, goals)
    assert "Informed" in tc.refused_with_code(_ffi.RRT_E_UNSUPPORTED, lambda: b.relax(0, R))
    _stands(lambda g: b.connect_goals(0, g), goals, ansi)
    b.close()


def test_plan_refusals_change_nothing():
    c = tc.base()
    w = tc.wall(c)
    R = tc.R2
    ctx = _ffi.Context(0)
    ctx.set_grid(c["og8"])
    n = c["n"]

    def refused(code, r2=R, samples=NONE):
        with pytest.raises(_ffi.RRTError) as e:
            ctx.relax(r2, samples, n)
        assert e.value.code == code and not e.value.seeded, e.value
        return str(e.value)

    assert "no rrt_plan on this context yet" in refused(_ffi.RRT_E_ARG)
    goals = tc.mixed_goals(c["og8"])
    Cm = hostprep.rotation_to_world_frame(np.asarray(c["xs"], dtype=np.int64), np.asarray(c["xg"], dtype=np.int64))
    qi, keepi = _ffi.make_query(2, 300, c["xs"], c["xg"], c["samples"][:300], r2_rewire=c["r2"], goal_d2=0, Cmat=Cm)
    ctx.plan(qi, 300, logs=True)
    assert "Informed" in refused(_ffi.RRT_E_UNSUPPORTED)
    qu, keep = _ffi.make_query(c["alg"], n, c["xs"], c["xg"], c["samples"], r2_rewire=c["r2"])
    ctx.plan(qu, n, rewire=True)
    assert "RRT_FLAG_REWIRE" in refused(_ffi.RRT_E_UNSUPPORTED)
    rc_, res = ctx.plan(qu, n)
    ans0 = ctx.connect_goals(goals)
    room = n - res.j
    assert f"room for {room}" in refused(_ffi.RRT_E_ARG, R, c["samples"][:room + 1])
    assert "r2=0" in refused(_ffi.RRT_E_ARG, 0)
    assert "outside the" in refused(_ffi.RRT_E_ARG, R, np.array([(5, 5), (200, 5)]))
    j0 = ctypes.c_int32(-1)
    assert _ffi.lib().rrt_plan_relax(ctx.handle, R, None, -1, ctypes.byref(j0), None, ctypes.byref(res.c)) == _ffi.RRT_E_ARG and j0.value == -1
    assert _ffi.lib().rrt_plan_relax(ctx.handle, R, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    _stands(ctx.connect_goals, goals, ans0)
    ctx.set_grid(w["og2"])
    assert "was not kept on it" in refused(_ffi.RRT_E_ARG)
    og3 = w["og2"].copy()
    og3[c["xs"][0], c["xs"][1]] = 1
    ctx.set_grid(og3)
    assert not ctx.keep_tree().any()
    assert "root is blocked" in refused(_ffi.RRT_E_ARG)
    # and the call itself, on the kept view, equals the restatement
    ctx.set_grid(w["og2"])
    assert np.array_equal(ctx.keep_tree(), w["alive"])
    v1 = ctx.connect_goals(goals)
    _stands(ctx.connect_goals, goals, v1)
    X, g = _restate(w["og2"], _same_as_oracle(res, c), True, tc.RR, NONE, c, rc.relaxed(c, tc.RR, w["og2"], True))
    rc_, out, j0, old_id = ctx.relax(R, NONE, n)
    assert j0 == len(X.ids) and np.array_equal(old_id, X.ids) and len(ctx.relax_ms()) == 9 and ctx.relax_stats()["fell"] == X.fell
    tc.same_result(out, g)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 7. the classes
def test_rrtstar_relax_is_the_restatement_fed_with_the_same_draws():
    c = tc.base()
    og = c["og8"].astype(np.int64)
    N = tc.N
    p = amd.RRTStar(og, N, tc.RR, pbar=False, seed=3)
    with pytest.raises(RuntimeError):
        p.relax()
    T, gv = p.plan(c["xs"], c["xg"])
    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    prev = (np.array(points), np.array(parent), np.array(vcosts), j)
    state = p.rand_gen.bit_generator.state
    with pytest.raises(ValueError, match=f"room for {N - j} more"):
        p.relax(m=N - j + 1)
    assert p.rand_gen.bit_generator.state == state and p._tree_resident == "device"
    m = min(N - j, 100)
    twin = np.random.default_rng(0)
    twin.bit_generator.state = p.rand_gen.bit_generator.state
    samples = hostprep.draw_free_samples(twin, np.argwhere(og == 0), m)
    X, g = _restate(c["og8"], prev, False, tc.RR, samples, c)
    T2, gv2 = p.relax(m=m)  # r defaults to r_rewire
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state
    assert np.array_equal(p.last_grow_ids, X.ids) and p.last_route == "kernel" and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j
    assert p.last_relax["fell"] == X.fell and 1 <= p.last_relax["rounds"] <= j
    vg, pts2, par2, vc2 = T2.__dict__["_lazy"]
    live = g.j + g.found
    assert gv2 == vg == g.vgoal and len(pts2) == g.rows and len(par2) == live
    assert np.array_equal(pts2[:live], g.pts[:live]) and np.array_equal(par2, g.parent[:live])
    assert np.array_equal(np.asarray(vc2[:live]).view(np.int64), g.vcost[:live].view(np.int64))
    tc.class_goals_and_routes(p, c["og8"], g, tc.mixed_goals(c["og8"]))
    # reroot, then relax with a radius of its own
    cur = (g.pts, g.parent, g.vcost, g.j)
    r = int(np.argmax(keepref.depth(cur[1], cur[3])))
    Z = rerootref.reroot(c["og8"], cur[0], cur[1], cur[3], r)
    T3, gv3 = p.reroot(r)
    assert np.array_equal(p.last_grow_ids, Z.ids)
    X4, g4 = _restate(c["og8"], (Z.pts, Z.parent, Z.vcost, len(Z.ids)), False, 12, NONE, c)
    T4, gv4 = p.relax(12)
    assert np.array_equal(p.last_grow_ids, X4.ids) and np.array_equal(T4.__dict__["_lazy"][2], g4.parent[:g4.j + g4.found]) and p.last_relax["fell"] == X4.fell


def test_rrtstandard_must_pass_r_and_the_classes_that_do_not_relax():
    c = tc.base(alg=0)
    og = c["og8"].astype(np.int64)
    p = amd.RRTStandard(og, tc.N, pbar=False, seed=3)
    try:
        T, gv = p.plan(c["xs"], c["xg"])
    except IndexError:
        pass
    j = p.last_stats["j"]
    state = p.rand_gen.bit_generator.state
    with pytest.raises(ValueError, match="pass r"):
        p.relax()
    assert p._tree_resident == "device" and p.rand_gen.bit_generator.state == state
    try:
        p.relax(tc.RR)
    except IndexError:  # (the plan's own goal not reached: the relaxed tree is resident all the same)
        pass
    assert p.last_relax["fell"] > j // 2 and p.last_stats["j"] == j and sorted(p.last_grow_ids.tolist()) == list(range(j))
    for q in (amd.RRTStarInformed(og, tc.N, tc.RR, 10, pbar=False), amd.RRTStar(og, tc.N, tc.RR, pbar=False, rewire="correct")):
        try:
            q.plan(c["xs"], c["xg"])
        except IndexError:
            pass
        with pytest.raises(ValueError, match="relax"):
            q.relax()
        assert q._tree_resident == "device"  # the refusal left the tree
