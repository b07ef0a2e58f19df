"""GPU: a finished tree grown with new samples (rrt_seed_*_kernel, rrt_batch_grow / rrt_plan_grow, _ffi.Batch.grow / Context.grow,
RRT.grow), on every launch shape a non-Informed query can take, and the goals and routes calls on the grown tree.

Every comparison is exact (==, array_equal, costs bit for bit).  The check is growref.py -- keepref's seed, the loop over the oracle's
primitives, goalref's go2goal -- and, where nothing was cut, oracle.plan over all samples as well."""
import ctypes

import numpy as np
import pytest

import growref
import keepref
import oracle
import slabs
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from treecalls import (N, R2, RR, SHAPES, base, class_goals_and_routes, goals_and_routes, grow_checked, mixed_goals, refused_with_code, set_case_query,
                       shaped_batch, tree_of, wall)

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------ 1. nothing cut
@pytest.mark.parametrize("shape", list(SHAPES))
def test_nothing_cut_is_the_longer_plan(gpu_ctx, shape):
    c = base()
    ro = c["ro"]
    m = c["n"] - ro.j
    assert ro.j > 1000 and m >= 100 and (ro.accept_log == 0).any()  # room to grow: the plan rejected samples
    more = hostprep.draw_free_samples(np.random.default_rng(31), np.argwhere(c["og8"] == 0), m)
    b = shaped_batch(gpu_ctx, c, shape)
    set_case_query(b, 0, c)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    assert r0.j == ro.j and np.array_equal(r0.vcost[:ro.j], ro.vcost[:ro.j])
    g, res = grow_checked(b, 0, c["og8"], tree_of(r0), False, more, c, shape)
    st, rl = oracle.plan(c["og8"], c["n"] + m, c["alg"], c["xs"], c["xg"], np.concatenate([c["samples"], more]), r2_rewire=c["r2"])
    live = rl.j + rl.found
    assert g.j < c["n"] and res.j == rl.j > ro.j + 50 and res.found == rl.found
    assert np.array_equal(res.pts[:live], rl.pts[:live]) and np.array_equal(res.parent[:live], rl.parent[:live])
    assert np.array_equal(res.vcost[:live].view(np.int64), rl.vcost[:live].view(np.int64))
    goals_and_routes(b, 0, c["og8"], res)
    b.close()


# ------------------------------------------------------------------------------------------------ 2. a wall stamped in
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_kept_tree_grows_back_behind_the_wall(gpu_ctx, shape):
    c = base()
    w = wall(c)
    og2, ro = w["og2"], c["ro"]
    assert (~w["alive"]).sum() >= 100 and len(w["ids"]) >= 100 and len(w["ids"]) > 64  # above PP_TINY
    assert len(w["cut_free"]) >= 20 and len(w["samples"]) == c["n"] - len(w["ids"])
    b = shaped_batch(gpu_ctx, c, shape)
    set_case_query(b, 0, c)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    gpu_ctx.set_grid(og2)
    assert np.array_equal(b.keep_tree(0), w["alive"])
    g, res = grow_checked(b, 0, og2, tree_of(r0), True, w["samples"], c, shape)
    acc = g.accept_log[w["where"]]
    assert acc[:-2].any() and not acc[-1]  # a cut vertex's cell is a vertex again; the obstacle cell is not
    assert g.j - g.j0 >= 100
    goals_and_routes(b, 0, og2, res)
    # the grown tree is an ordinary finished query: kept again on the first map, every edge that crosses no new obstacle survives
    gpu_ctx.set_grid(c["og8"])
    pts, parent, vcost, j = tree_of(res)
    assert np.array_equal(b.keep_tree(0), keepref.alive(c["og8"], pts, parent, j))
    b.close()


@pytest.mark.parametrize("shape", ["team", "pipe1", "serial"])
def test_a_kept_rrtstandard_tree_grows_back(gpu_ctx, shape):
    """alg = 0: no near set, no cost comparison -- the same seed, the loop of rrt.py:418-437"""
    c = base(seed=25, alg=0, r2=0)
    w = wall(c)
    assert (~w["alive"]).sum() >= 100 and len(w["ids"]) > 64 and len(w["samples"]) == c["n"] - len(w["ids"])
    b = shaped_batch(gpu_ctx, c, shape)
    set_case_query(b, 0, c)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    assert r0.j == c["ro"].j
    gpu_ctx.set_grid(w["og2"])
    assert np.array_equal(b.keep_tree(0), w["alive"])
    g, res = grow_checked(b, 0, w["og2"], tree_of(r0), True, w["samples"], c, shape)
    assert g.j - g.j0 >= 100 and g.sum_near == 0
    goals_and_routes(b, 0, w["og2"], res)
    b.close()


# ------------------------------------------------------------------------------------------------ 3. only the root alive
@pytest.mark.parametrize("shape", ["team", "pipe1", "block1", "serial"])
def test_only_the_root_alive_is_the_tiny_tree_path(gpu_ctx, shape):
    c = base()
    xs = c["xs"]
    og2 = c["og8"].copy()
    og2[max(xs[0] - 3, 0):xs[0] + 4, max(xs[1] - 3, 0):xs[1] + 4] = 1
    og2[xs[0], xs[1]] = 0  # xstart alone in a filled block: every edge out of it is cut
    b = shaped_batch(gpu_ctx, c, shape)
    set_case_query(b, 0, c)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    gpu_ctx.set_grid(og2)
    alive = b.keep_tree(0)
    assert alive.sum() == 1 and alive[0]
    samples = np.concatenate([[xs], hostprep.draw_free_samples(np.random.default_rng(5), np.argwhere(og2 == 0), 40), [xs]])
    g, res = grow_checked(b, 0, og2, tree_of(r0), True, samples, c, shape)
    # xstart drawn once becomes vertex 1 (rrt.py:425: it is never in `sampled`), the second time it is refused; nothing else is visible
    assert g.j0 == 1 and g.j == 2 and g.accept_log[0] == 1 and g.accept_log[-1] == 0 and not g.found and res.status == _ffi.RRT_E_GOAL_UNREACHABLE
    goals_and_routes(b, 0, og2, res, connected=0)  # (two vertices on xstart inside a filled block: no goal has to see them)
    b.close()


# ------------------------------------------------------------------------------------------------ 4. a seed across a scan chunk
def test_a_seed_of_more_than_4096_vertices_grown_twice(gpu_ctx):
    c = base(W=512, gseed=4, pair=6, n=6000, seed=22)
    ro = c["ro"]
    room = c["n"] - ro.j
    assert ro.j > 4096 + 64 and room >= 100, (ro.j, room)
    b = shaped_batch(gpu_ctx, c, "team")
    set_case_query(b, 0, c)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    free = np.argwhere(c["og8"] == 0)
    g1, r1 = grow_checked(b, 0, c["og8"], tree_of(r0), False, hostprep.draw_free_samples(np.random.default_rng(41), free, room // 2), c, "team")
    assert g1.j0 > 4096 and g1.j > g1.j0
    goals_and_routes(b, 0, c["og8"], r1)
    og2 = c["og8"].copy()
    far = np.argmax(np.abs(np.asarray(g1.pts[:g1.j]) - c["xs"]).sum(axis=1))
    fx, fy = (int(v) for v in g1.pts[far])
    og2[max(fx - 80, 0):fx + 80, max(fy - 80, 0):fy + 80] = 1  # a block far from the start: cuts some 200 vertices
    og2[c["xs"][0], c["xs"][1]] = 0
    gpu_ctx.set_grid(og2)
    pts, parent, vcost, j = tree_of(r1)
    alive = b.keep_tree(0)
    assert np.array_equal(alive, keepref.alive(og2, pts, parent, j)) and 4096 < alive.sum() < j - 20
    m2 = min(c["n"] - int(alive.sum()), 600)
    g2, r2 = grow_checked(b, 0, og2, (pts, parent, vcost, j), True, hostprep.draw_free_samples(np.random.default_rng(42), np.argwhere(og2 == 0), m2), c, "team")
    assert g2.j0 > 4096 and g2.j > g2.j0 + 100
    goals_and_routes(b, 0, og2, r2)
    b.close()


# ------------------------------------------------------------------------------------------------ 5. a ball of more than 64 cells
def test_a_radius_whose_ball_takes_a_second_slab_of_cells(gpu_ctx):
    r2 = hostprep.radius_threshold(120)
    c = base(r2=r2, seed=23)
    w = wall(c)
    shift = slabs.cell_shift(200, 200, r2, slabs.DIV_PIPE)
    assert slabs.largest_box(200, 200, r2, shift) > 64
    b = shaped_batch(gpu_ctx, c, "pipe1")
    set_case_query(b, 0, c)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    gpu_ctx.set_grid(w["og2"])
    b.keep_tree(0)
    g, res = grow_checked(b, 0, w["og2"], tree_of(r0), True, w["samples"], c, "pipe1")
    cov = slabs.coverage(200, 200, r2, shift, w["samples"], np.ones(len(w["samples"]), dtype=bool), g.jlog, g.pts, g.nearest_log, g.accept_log, g.parent)
    assert cov["reach"] >= 1 and cov["max_box"] > 64, cov  # a grown iteration needs a record of the SEED from a later slab
    goals_and_routes(b, 0, w["og2"], res)
    b.close()


# ------------------------------------------------------------------------------------------------ 6. a batch of three
def test_one_query_of_three_grown_the_others_unchanged(gpu_ctx):
    c = base()
    w = wall(c)
    cs = [c, base(seed=24, pair=7), base(seed=25, alg=0, r2=0)]
    b = shaped_batch(gpu_ctx, c, "team", Q=3)
    for q, cq in enumerate(cs):
        set_case_query(b, q, cq)
    b.launch()
    b.sync()
    before = [b.get_result(q) for q in range(3)]
    for q, cq in enumerate(cs):
        assert before[q].j == cq["ro"].j
    gpu_ctx.set_grid(w["og2"])
    b.keep_tree(0)
    b.keep_tree(2)
    g, res = grow_checked(b, 0, w["og2"], tree_of(before[0]), True, w["samples"], c, "team", Q=3)
    for q in (1, 2):
        r = b.get_result(q)
        assert (r.status, r.j, r.found, r.vgoal) == (before[q].status, before[q].j, before[q].found, before[q].vgoal)
        live = r.j + r.found
        assert np.array_equal(r.pts[:live], before[q].pts[:live]) and np.array_equal(r.parent[:live], before[q].parent[:live])
        assert np.array_equal(r.vcost[:live].view(np.int64), before[q].vcost[:live].view(np.int64))
        with pytest.raises(_ffi.RRTError):  # the launch dropped the view of query 2; query 1 never had one for this grid
            b.connect_goals(q, [(5, 5)])
    goals_and_routes(b, 0, w["og2"], res)
    b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals and m == 0
def test_refusals_change_nothing_and_m_zero_only_connects_the_goal(gpu_ctx):
    c = base()
    w = wall(c)
    b = shaped_batch(gpu_ctx, c, "pipe1")
    refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(0, c["samples"][:5]))  # no query set
    set_case_query(b, 0, c)
    refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(0, c["samples"][:5]))  # not launched
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    goals = mixed_goals(c["og8"])
    ans0 = b.connect_goals(0, goals)
    j0, log0 = ctypes.c_int32(-1), ctypes.c_int32(-1)  # m < 0: below what _ffi.Batch.grow can pass
    assert _ffi.lib().rrt_batch_grow(b._h, 0, None, -1, ctypes.byref(j0), None, ctypes.byref(log0)) == _ffi.RRT_E_ARG
    assert (j0.value, log0.value) == (-1, -1) and b"m=-1" in _ffi.lib().rrt_last_error_string(gpu_ctx.handle)
    room = c["n"] - r0.j
    refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(1, c["samples"][:5]))
    assert f"room for {room}" in refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(0, c["samples"][:room + 1]))  # one more than the room
    refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(0, np.array([(5, 5), (200, 5)])))  # outside the grid
    # a new grid without keep_tree
    gpu_ctx.set_grid(w["og2"])
    refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(0, c["samples"][:5]))
    # the root blocked: refused, the view and its answers stay
    og3 = w["og2"].copy()
    og3[c["xs"][0], c["xs"][1]] = 1
    gpu_ctx.set_grid(og3)
    assert not b.keep_tree(0).any()
    v0, c0 = b.connect_goals(0, goals)
    assert "root is blocked" in refused_with_code(_ffi.RRT_E_ARG, lambda: b.grow(0, c["samples"][:5]))
    v1, c1 = b.connect_goals(0, goals)
    assert np.array_equal(v0, v1) and np.array_equal(c0, c1) and (v1 == -1).all()
    # after all these refusals the tree is what it was
    gpu_ctx.set_grid(c["og8"])
    assert b.keep_tree(0).all()
    r1 = b.get_result(0)
    assert np.array_equal(r1.pts, r0.pts) and np.array_equal(r1.vcost.view(np.int64), r0.vcost.view(np.int64)) and np.array_equal(r1.parent, r0.parent)
    ans1 = b.connect_goals(0, goals)
    assert np.array_equal(ans0[0], ans1[0]) and np.array_equal(ans0[1], ans1[1])
    # m == 0 on the wall map: the seed, then go2goal
    gpu_ctx.set_grid(w["og2"])
    b.keep_tree(0)
    g, res = grow_checked(b, 0, w["og2"], tree_of(r0), True, np.zeros((0, 2), dtype=np.int32), c, "pipe1")
    assert g.j == g.j0 == len(w["ids"]) and res.i_switch == c["n"]
    goals_and_routes(b, 0, w["og2"], res)
    b.close()
    # what the batch cannot grow
    for kw in (dict(rewire=True), dict(dubins=True), dict(large_grid=True)):
        bb = _ffi.Batch(gpu_ctx, 1, 100, **kw)
        refused_with_code(_ffi.RRT_E_UNSUPPORTED, lambda: bb.grow(0, c["samples"][:5]))
        bb.close()


def test_an_informed_query_is_refused(gpu_ctx):
    c = base()
    gpu_ctx.set_grid(c["og8"])
    b = _ffi.Batch(gpu_ctx, 1, 300, logs=True)
    Cm = hostprep.rotation_to_world_frame(np.asarray(c["xs"], dtype=np.int64), np.asarray(c["xg"], dtype=np.int64))
    qu, keep = _ffi.make_query(2, 300, c["xs"], c["xg"], c["samples"][:300], r2_rewire=c["r2"], goal_d2=0, Cmat=Cm)
    b.set_query(0, qu)
    b.launch()
    b.sync()
    assert b.get_result(0).j > 10
    refused_with_code(_ffi.RRT_E_UNSUPPORTED, lambda: b.grow(0, c["samples"][:5]))
    b.close()


# ------------------------------------------------------------------------------------------------ 8. the class
def test_grow_after_a_plan_that_did_not_reach_its_goal():
    """plan() raises IndexError (the goal boxed in): the tree is resident, and this is the case grow is for.  grow on the same map
    raises the same way and still leaves the grown tree; after keep_tree on the map without the box a further grow reaches the goal,
    and row n of T is the goal of that plan()."""
    c = base()
    og8, xs, xg = c["og8"], c["xs"], c["xg"]
    boxed = og8.copy()
    boxed[max(xg[0] - 4, 0):xg[0] + 5, max(xg[1] - 4, 0):xg[1] + 5] = 1
    boxed[xg[0], xg[1]] = 0
    p = amd.RRTStar(boxed.astype(np.int64), N, RR, pbar=False, seed=3)
    twin = np.random.default_rng(0)
    twin.bit_generator.state = p.rand_gen.bit_generator.state
    st, ro = oracle.plan(boxed, N, 1, xs, xg, hostprep.draw_free_samples(twin, np.argwhere(boxed == 0), N), r2_rewire=R2)
    assert st == growref.ST_UNREACHABLE and not ro.found and N - ro.j >= 100
    with pytest.raises(IndexError):
        p.plan(xs, xg)
    assert p._tree_resident == "device" and p.last_route == "kernel"
    # 1. grow straight after the failed plan: the first plan of this planner
    m1 = 80
    ids, sp, sc, spar = growref.seed(ro.pts, ro.parent, ro.vcost, ro.j)
    g1 = growref.grow(boxed, 1, N, xg, R2, sp, sc, spar, hostprep.draw_free_samples(twin, np.argwhere(boxed == 0), m1))
    assert g1.status == growref.ST_UNREACHABLE and g1.j > g1.j0 == ro.j
    with pytest.raises(ValueError, match=f"room for {N - ro.j} more"):
        p.grow(N - ro.j + 1)
    with pytest.raises(IndexError):
        p.grow(m1)
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state and p._tree_resident == "device"
    assert np.array_equal(p.last_grow_ids, ids) and p.last_stats["j"] == g1.j and p.last_stats["sum_j"] == g1.sum_j
    goals = mixed_goals(boxed)
    class_goals_and_routes(p, boxed, g1, goals)
    # 2. the box gone: keep_tree, then grow into the room that is left
    alive = p.keep_tree(og8.astype(np.int64))
    assert np.array_equal(alive, keepref.alive(og8, g1.pts, g1.parent, g1.j)) and alive.all()
    m2 = N - g1.j
    ids, sp, sc, spar = growref.seed(g1.pts, g1.parent, g1.vcost, g1.j, og8_view=og8)
    g2 = growref.grow(og8, 1, N, xg, R2, sp, sc, spar, hostprep.draw_free_samples(twin, np.argwhere(og8 == 0), m2))
    assert g2.found and g2.status == growref.ST_OK
    T, gv = p.grow(m2)
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state and np.array_equal(p.last_grow_ids, ids)
    vg, pts, par, vc = T.__dict__["_lazy"]
    live = g2.j + 1
    assert gv == vg == g2.vgoal and len(pts) == g2.rows == N + 1 and np.array_equal(pts[N], xg) and vc[N] == g2.vcost[g2.j]
    assert np.array_equal(pts[:live], g2.pts[:live]) and np.array_equal(par, g2.parent[:live])
    assert np.array_equal(np.asarray(vc[:live]).view(np.int64), g2.vcost[:live].view(np.int64))
    class_goals_and_routes(p, og8, g2, mixed_goals(og8))


def test_rrtstar_grow_is_the_restatement_fed_with_the_same_draws():
    c = base()
    w = wall(c)
    og = c["og8"].astype(np.int64)
    og2 = w["og2"].astype(np.int64)
    p = amd.RRTStar(og, N, RR, pbar=False, seed=3)
    with pytest.raises(RuntimeError):
        p.grow(10)
    T, gv = p.plan(c["xs"], c["xg"])
    _, points, parent, vcosts = T.__dict__["_lazy"]
    j = p.last_stats["j"]
    with pytest.raises(ValueError, match=f"room for {N - j} more"):
        p.grow(N - j + 1)
    alive = p.keep_tree(og2)
    j0 = int(alive.sum())
    m = min(N - j0, 500)
    twin = np.random.default_rng(0)
    twin.bit_generator.state = p.rand_gen.bit_generator.state
    samples = hostprep.draw_free_samples(twin, np.argwhere(og2 == 0), m)
    ids, sp, sc, spar = growref.seed(np.array(points), np.array(parent), np.array(vcosts), j, og8_view=w["og2"])
    g = growref.grow(w["og2"], 1, N, c["xg"], R2, sp, sc, spar, samples)
    T2, gv2 = p.grow(m)
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state
    assert np.array_equal(p.last_grow_ids, ids) and p.last_route == "kernel" and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j
    vg, pts2, par2, vc2 = T2.__dict__["_lazy"]
    assert gv2 == vg == g.vgoal and len(pts2) == g.rows and len(par2) == g.j + g.found
    assert np.array_equal(pts2[:g.j + g.found], g.pts[:g.j + g.found]) and np.array_equal(par2, g.parent[:g.j + g.found])
    assert np.array_equal(np.asarray(vc2[:g.j + g.found]).view(np.int64), g.vcost[:g.j + g.found].view(np.int64))
    if g.found:
        assert np.array_equal(pts2[N], c["xg"]) and vc2[N] == g.vcost[g.j]
    goals = mixed_goals(w["og2"])
    class_goals_and_routes(p, w["og2"], g, goals)
    T3, gv3 = p.grow(0)  # a further grow on the grown tree: nothing new, the same tree
    assert np.array_equal(p.last_grow_ids, np.arange(g.j)) and np.array_equal(T3.__dict__["_lazy"][2], par2)


def test_the_classes_that_do_not_grow():
    """with a tree on the device (tests/test_grow_cpu.py has the same refusals, and the Dubins planner's, before any plan)"""
    c = base()
    og = c["og8"].astype(np.int64)
    for p in (amd.RRTStarInformed(og, N, RR, 10, pbar=False), amd.RRTStar(og, N, RR, pbar=False, rewire="correct")):
        try:
            p.plan(c["xs"], c["xg"])
        except IndexError:  # (the plan's own goal not reached: the tree is resident all the same)
            pass
        assert p._tree_resident == "device"
        with pytest.raises(ValueError, match="grow"):
            p.grow(5)
        assert p._tree_resident == "device"  # the refusal left the tree
    p = amd.RRTStandard(og, 300, pbar=False)
    try:
        p.plan(c["xs"], c["xg"])
    except IndexError:
        pass
    p.set_og(og.copy())
    with pytest.raises(RuntimeError):
        p.grow(5)
