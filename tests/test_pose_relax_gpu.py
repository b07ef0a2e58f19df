"""GPU: a finished Dubins tree relaxed to shortest paths over its own poses (rrt_pose_relax_*_kernel, rrt_batch_relax_poses /
rrt_plan_relax_poses, _ffi.Batch.relax_poses / Context.relax_poses, RRTDubins / RRTStarDubins .relax_poses), then grown, and the pose
tree calls on the result.

Every comparison is exact (==, array_equal, costs as raw bits).  The check is poserelaxref.py -- the candidate edges swept with the
oracle's words from u to v, Dijkstra's costs, the parent rule, the order, the costs summed from the root down -- followed by
posegrowref.grow; and poserelaxref.certify on the arrays the device returned.  The inputs are those of poserelaxcases.py;
test_pose_relax_cpu.py says what each is for.  Of the statistics only `fell` is exact: the rounds depend on the order the wavefronts ran in."""
import ctypes
import json
import os

import numpy as np
import pytest

import oracle
import posegrowref
import posekeepref
import poserelaxcases as pc
import poserelaxref
import poseref
import poseroutesref
import poseshortref
from posecalls import GROW_KERNELS, planned_logged_batch, refused_with_golden_text
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins
from treecalls import same_result, tree_of

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_relax_refusals.json")) as f:
    GOLDEN = json.load(f)

NONE = np.zeros((0, 3), dtype=np.int32)


def _restate(w, og8, prev, view, r, samples, X=None, n=None):
    if X is None:
        X = poserelaxref.relax(og8, *prev, pc.R_of(r), w.rho, w.nh, og8_view=og8 if view else None)
    return X, posegrowref.grow(og8, w.star, w.n if n is None else n, w.xg, w.r2, w.rho, w.nh, X.pts, X.head, X.vcost, X.parent, samples)


def _held(st, X, j0):
    """the statistics of a call against the restatement X: fell exactly, the others within what any order of the wavefronts allows"""
    print("device", st, "restatement", dict(fell=X.fell, words=X.words, sweeps=X.sweeps, pairs=X.pairs))
    assert st["fell"] == X.fell, (st, X.fell)
    assert 1 <= st["rounds"] <= max(j0, 1), st
    assert X.sweeps <= st["sweeps"] <= st["rounds"] * X.pairs, (st, X.sweeps, X.pairs)
    assert X.words <= st["words"] <= st["rounds"] * X.pairs, (st, X.words, X.pairs)


def _arm(b, q, r, samples, X):
    j0, old_id, log0 = b.relax_poses(q, pc.R_of(r), samples)
    assert j0 == len(X.ids) == log0 and np.array_equal(old_id, X.ids), (j0, len(X.ids), log0)
    ms = b.relax_poses_ms()
    assert len(ms) == 9 and all(t >= 0.0 for t in ms)
    _held(b.relax_poses_stats(), X, j0)
    return log0


def _relax(b, q, w, og8, prev, view, r, samples, X=None, kernel=None, n=None):
    """one relax_poses of query q on map og8 of the tree `prev` = (pts, head, parent, vcost, j), launched and checked against the
    restatement and by the certificate.  Returns (Relaxed, Grown, result)."""
    X, g = _restate(w, og8, prev, view, r, samples, X, n)
    log0 = _arm(b, q, r, samples, X)
    b.launch()
    b.sync()
    res = b.get_result(q)
    same_result(res, g, log0)
    assert b.team()[1] == 0
    if kernel:
        assert b.kernel_name() == GROW_KERNELS[kernel][1], b.kernel_name()
    if len(samples) == 0:  # the device's own arrays, by rules of their own
        j0 = len(X.ids)
        assert poserelaxref.certify(og8, res.pts[:j0], res.head[:j0], res.parent[:j0], res.vcost[:j0], pc.R_of(r), w.rho, w.nh,
                                    poserelaxref.old_edges_of(X.in_parent, X.order), prev=X.order) == []
    return X, g, res


# ------------------------------------------------------------------------------------------------ 1. the workloads, the crafted inputs, the sizes
@pytest.mark.parametrize("name", list(pc.WORKLOADS) + list(pc.FIXTURES))
def test_the_workloads_and_the_crafted_inputs(gpu_ctx, name):
    w, r, X = pc.fixture(name)
    b = planned_logged_batch(gpu_ctx, w, "block")
    _relax(b, 0, w, w.og8, pc.tree(w), False, r, NONE, X=X)
    print(name, b.relax_poses_stats(), b.relax_poses_ms())
    b.close()


def test_trees_of_exactly_1_2_63_to_65_and_1023_to_1025_vertices(gpu_ctx):
    for j in pc.SIZES:
        w, r, X = pc.fixture(f"sized{j}")
        assert w.j == j
        b = planned_logged_batch(gpu_ctx, w, "block")
        _, _, res = _relax(b, 0, w, w.og8, pc.tree(w), False, r, NONE, X=X)
        assert res.j == j
        b.close()


# ------------------------------------------------------------------------------------------------ 2. m > 0 on both Dubins kernels
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_relax_then_grow_on_both_dubins_kernels(gpu_ctx, kernel):
    w, r, X = pc.fixture("E")
    m = 100
    assert w.j + m <= w.n
    s = posegrowref.more_poses(w, w.og8, m, seed=34)
    s[3, :2] = w.ro.pts[5]  # a vertex's cell drawn again: refused
    b = planned_logged_batch(gpu_ctx, w, kernel)
    X, g, res = _relax(b, 0, w, w.og8, pc.tree(w), False, r, s, X=X, kernel=kernel)
    assert g.j > g.j0 + 20 and not g.accept_log[3]
    b.close()


# ------------------------------------------------------------------------------------------------ 3. after keep_pose_tree on a changed map
def test_a_kept_view_is_relaxed_among_its_alive_vertices(gpu_ctx):
    k = posekeepref.changed("A")
    w, r = k.w, pc.WORKLOADS["A"]
    b = planned_logged_batch(gpu_ctx, w, "block")
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive) and not k.alive.all()
    X, g, res = _relax(b, 0, w, k.og8, pc.tree(w), True, r, NONE, X=pc.relaxed(w, r, k.og8, True))
    assert set(X.ids.tolist()) == set(np.flatnonzero(k.alive).tolist()) and not np.array_equal(X.ids, np.arange(len(X.ids))) and X.fell > len(X.ids) // 2
    v, c, _ = poseref.connect(k.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    got = b.connect_poses(0, w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1].view(np.int64), c.view(np.int64))
    b.close()


# ------------------------------------------------------------------------------------------------ 4. afterwards
def test_the_pose_tree_calls_answer_on_the_relaxed_tree(gpu_ctx):
    w, r, X = pc.fixture("E")
    og8 = w.og8
    b = planned_logged_batch(gpu_ctx, w, "block")
    X, g, res = _relax(b, 0, w, og8, pc.tree(w), False, r, NONE, X=X)
    cur = tree_of(res)
    # connect_poses, and routes with points and shortcuts, in the new numbering
    v, c, _ = poseref.connect(og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    got = b.connect_poses(0, w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1].view(np.int64), c.view(np.int64)) and (v >= 0).sum() >= 4
    assert c[v >= 0].mean() < w.cost[w.vertex >= 0].mean()  # (the goals that connect are the same ones: the vertices did not move)
    poseroutesref.same(b.pose_routes(0, w.goals, points=True), poseroutesref.routes(g.pts, g.head, g.parent, g.j, w.goals, v, c, w.rho, w.nh))
    poseroutesref.same(b.pose_routes(0, w.goals, points=True, shortcut=True),
                       poseshortref.routes(g.pts, g.head, g.parent, g.j, w.goals, v, c, w.rho, w.nh, og8, shortcut=True))
    # a second relax_poses lowers nothing
    X2, g2, res2 = _relax(b, 0, w, og8, cur, False, r, NONE)
    st = b.relax_poses_stats()
    assert X2.fell == 0 and st["fell"] == 0 and st["rounds"] == 1
    assert np.array_equal(np.sort(res2.vcost[:cur[4]]).view(np.int64), np.sort(cur[3][:cur[4]]).view(np.int64))
    # keep_pose_tree on a changed map and grow_poses behind it
    cur = tree_of(res2)
    og2 = posekeepref.blocks_map(og8, w.xs)
    alive = posekeepref.alive(og2, cur[0], cur[1], cur[2], cur[4], w.rho, w.nh)
    gpu_ctx.set_grid(og2)
    assert np.array_equal(b.keep_pose_tree(0), alive) and alive[0] and not alive.all()
    ids, sp, sh, sc, spar = posegrowref.seed(cur[0], cur[1], cur[2], cur[3], cur[4], alive)
    s = posegrowref.more_poses(w, og2, min(w.n - len(ids), 60), seed=8)
    g3 = posegrowref.grow(og2, w.star, w.n, w.xg, w.r2, w.rho, w.nh, sp, sh, sc, spar, s)
    j0, old_id, log0 = b.grow_poses(0, s)
    assert j0 == len(ids) and np.array_equal(old_id, ids)
    b.launch()
    b.sync()
    same_result(b.get_result(0), g3, log0)
    with pytest.raises(_ffi.RRTError):
        b.relax_poses_ms()  # the stage times are the grow's now
    # rearm + launch still plans the query's own stream from xstart
    gpu_ctx.set_grid(og8)
    b.rearm()
    b.launch()
    b.sync()
    res = b.get_result(0)
    samples, heads = np.array(w.samples), np.array(w.heads)
    samples[j0:j0 + len(s)], heads[j0:j0 + len(s)] = s[:, :2], s[:, 2]  # (rows [j0, j0 + m) of the sample buffer hold the grow's samples)
    st, ro = oracle.dubins_plan(og8, w.n, w.star, w.xs, w.xg, samples, heads, r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    assert res.status == st and res.j == ro.j and np.array_equal(res.parent[:ro.j], ro.parent[:ro.j]) and np.array_equal(res.head[:ro.j], ro.head[:ro.j])
    assert np.array_equal(res.vcost[:ro.j].view(np.int64), ro.vcost[:ro.j].view(np.int64)) and tuple(res.pts[0]) == w.xs[:2]
    b.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def _raw(call, h, r2, s, m, null_j0=False):
    j0, log0 = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc = call(h, 0, int(r2), s.ctypes.data if s is not None else None, m, None if null_j0 else ctypes.byref(j0), None, ctypes.byref(log0))
    assert (j0.value, log0.value) == (-1, -1)
    return rc


def test_batch_refusals_have_the_golden_texts_and_change_nothing(gpu_ctx):
    w = poseref.workload("E")
    W, H = w.og8.shape
    R = pc.R_of(12)
    who = "rrt_batch_relax_poses"
    L = _ffi.lib()
    u = _ffi.Batch(gpu_ctx, 1, w.n, dubins=True)
    refused_with_golden_text(GOLDEN, "unfinished_query", u.relax_poses, 0, R)
    refused_with_golden_text(GOLDEN, "ms_none", u.relax_poses_ms)
    refused_with_golden_text(GOLDEN, "stats_none", u.relax_poses_stats)
    u.close()
    p = _ffi.Batch(gpu_ctx, 1, 100)
    refused_with_golden_text(GOLDEN, "non_dubins_batch", p.relax_poses, 0, R)
    p.close()
    b = planned_logged_batch(gpu_ctx, w, "block")
    before = b.get_result(0)
    ok = posegrowref.more_poses(w, w.og8, 4)
    refused_with_golden_text(GOLDEN, "dubins_batch_relax", b.relax, 0, R)  # the straight-line call keeps its answer for a Dubins batch
    refused_with_golden_text(GOLDEN, "q_out_of_range", b.relax_poses, 1, R)
    s32 = np.ascontiguousarray(ok, dtype=np.int32)
    assert _raw(L.rrt_batch_relax_poses, b._h, R, s32, -1) == _ffi.RRT_E_ARG
    assert L.rrt_last_error_string(gpu_ctx.handle).decode() == GOLDEN["m_negative"][1].format(who=who)
    assert _raw(L.rrt_batch_relax_poses, b._h, R, None, 0, null_j0=True) == _ffi.RRT_E_ARG
    assert L.rrt_last_error_string(gpu_ctx.handle).decode() == GOLDEN["null"][1].format(who=who)
    assert _raw(L.rrt_batch_relax_poses, b._h, R, None, 2) == _ffi.RRT_E_ARG  # samples announced and none given
    room = w.n - w.j
    fmt = dict(who=who, j=w.j, m=room + 1, n=w.n, room=room)
    refused_with_golden_text(GOLDEN, "room", b.relax_poses, 0, R, posegrowref.more_poses(w, w.og8, room + 1), **fmt)
    refused_with_golden_text(GOLDEN, "room", b.relax_poses, 0, 0, posegrowref.more_poses(w, w.og8, room + 1), **fmt)  # the room comes first
    for bad in (0, -5):
        refused_with_golden_text(GOLDEN, "r2_not_positive", b.relax_poses, 0, bad, ok, who=who, r2=bad)
    bad = ok.copy()
    bad[2, 2] = w.nh
    refused_with_golden_text(GOLDEN, "heading_out_of_range", b.relax_poses, 0, R, bad, who=who, nh=w.nh)
    refused_with_golden_text(GOLDEN, "r2_not_positive", b.relax_poses, 0, 0, bad, who=who, r2=0)  # the radius comes before the samples
    bad = ok.copy()
    bad[1, 0] = W
    refused_with_golden_text(GOLDEN, "cell_outside", b.relax_poses, 0, R, bad, who=who, x=W, y=int(bad[1, 1]), W=W, H=H)
    gpu_ctx.set_grid(np.zeros((W + 1, H), dtype=np.uint8))
    refused_with_golden_text(GOLDEN, "grid_shape", b.relax_poses, 0, R, who=who, W=W, H=H)
    gpu_ctx.set_grid(w.og8)  # the same cells, another generation
    with pytest.raises(_ffi.RRTError) as e:
        b.relax_poses(0, R)
    assert e.value.code == _ffi.RRT_E_ARG and str(e.value).endswith(GOLDEN["grid_not_kept"][1].split("now)")[1]) and f"{who}: the context's grid was replaced" in str(e.value)
    k = posekeepref.root_blocked(w)
    gpu_ctx.set_grid(k.og8)
    assert not b.keep_pose_tree(0).any()
    refused_with_golden_text(GOLDEN, "root_blocked", b.relax_poses, 0, R, who=who)
    gpu_ctx.set_grid(w.og8)
    assert b.keep_pose_tree(0).all()
    after = b.get_result(0)
    for name in ("pts", "vcost", "parent", "head"):
        assert np.array_equal(getattr(before, name), getattr(after, name))
    assert (after.status, after.j, after.found, after.vgoal) == (before.status, before.j, before.found, before.vgoal)
    v, c = b.connect_poses(0, w.goals)  # ... and the tree still answers as it did
    assert np.array_equal(v, w.vertex) and np.array_equal(c, w.cost)
    refused_with_golden_text(GOLDEN, "ms_none", b.relax_poses_ms)
    b.close()


def test_plan_refusals_and_the_call_through_rrt_plan():
    w = poseref.workload("D")  # RRTDubins: the planner without a near set
    r = pc.WORKLOADS["D"]
    R = pc.R_of(r)
    who = "rrt_plan_relax_poses"
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    refused_with_golden_text(GOLDEN, "no_plan", ctx.relax_poses, R, NONE, w.n)
    refused_with_golden_text(GOLDEN, "plan_ms_none", ctx.relax_poses_ms)
    qu, keep = poseref.device_query(w)
    rc, res = ctx.plan(qu, w.n)
    assert rc == w.status and res.j == w.j
    ans0 = ctx.connect_poses(w.goals)

    def refused(key, threshold, samples, **fmt):
        code, text = GOLDEN[key]
        with pytest.raises(_ffi.RRTError) as e:
            ctx.relax_poses(threshold, samples, w.n)
        assert e.value.code == code and not e.value.seeded and str(e.value) == f"librrt_hip error {code}: {text.format(who=who, **fmt)}", str(e.value)

    room = w.n - w.j
    refused("room", R, posegrowref.more_poses(w, w.og8, room + 1), j=w.j, m=room + 1, n=w.n, room=room)
    refused("r2_not_positive", 0, NONE, r2=0)
    bad = posegrowref.more_poses(w, w.og8, 3)
    bad[2, 2] = w.nh
    refused("heading_out_of_range", R, bad, nh=w.nh)
    j0 = ctypes.c_int32(-1)
    L = _ffi.lib()
    assert L.rrt_plan_relax_poses(ctx.handle, R, None, -1, ctypes.byref(j0), None, ctypes.byref(res.c)) == _ffi.RRT_E_ARG and j0.value == -1
    assert L.rrt_plan_relax_poses(ctx.handle, R, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    got = ctx.connect_poses(w.goals)
    assert np.array_equal(got[0], ans0[0]) and np.array_equal(got[1], ans0[1])
    with pytest.raises(_ffi.RRTError) as e:
        ctx.relax(R, np.zeros((0, 2), dtype=np.int32), w.n)
    assert str(e.value) == f"librrt_hip error {GOLDEN['dubins_batch_relax'][0]}: " + GOLDEN["dubins_batch_relax"][1].replace("rrt_batch_relax", "rrt_plan_relax")
    # and the call itself equals the restatement
    X, g = _restate(w, w.og8, pc.tree(w), False, r, NONE, pc.relaxed(w, r))
    rc, out, j0, old_id = ctx.relax_poses(R, NONE, w.n)
    assert rc == g.status and j0 == len(X.ids) and np.array_equal(old_id, X.ids) and len(ctx.relax_poses_ms()) == 9
    _held(ctx.relax_poses_stats(), X, j0)
    same_result(out, g)
    v, c, _ = poseref.connect(w.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    got = ctx.connect_poses(w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1], c)
    ctx.close()


# ------------------------------------------------------------------------------------------------ 6. the classes
def _class_golden(key, fn, *args, **fmt):
    code, text = GOLDEN[key]
    assert code == "ValueError"
    with pytest.raises(ValueError) as e:
        fn(*args)
    assert str(e.value) == text.format(**fmt), str(e.value)


def test_rrtstardubins_relax_poses_is_the_restatement_fed_with_the_same_draws():
    w = poseref.workload("E")
    r, seed = poseref.SPECS["E"][4], poseref.SPECS["E"][7]
    p = RRTStarDubins(w.og, w.n, r, w.rho, n_headings=w.nh, pbar=False, seed=seed)
    with pytest.raises(RuntimeError):
        p.relax_poses()
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j and p._grow_j0 == w.j
    _class_golden("dubins_planner_relax", p.relax)
    _class_golden("radius_not_positive", p.relax_poses, 0)
    _class_golden("room_class", lambda: p.relax_poses(m=w.n - w.j + 1), j=w.j, n=w.n, room=w.n - w.j, m=w.n - w.j + 1)
    _class_golden("m_negative_class", lambda: p.relax_poses(m=-1))
    assert p._tree_resident == "device"
    m = 60
    twin = np.random.default_rng(0)
    twin.bit_generator.state = p.rand_gen.bit_generator.state
    cells = hostprep.draw_free_samples(twin, np.argwhere(w.og8 == 0), m)
    s = np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), twin.integers(0, w.nh, m)])
    X, g = _restate(w, w.og8, pc.tree(w), False, r, s, pc.relaxed(w, r))
    T2, gv2 = p.relax_poses(m=m)  # r defaults to r_rewire
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state
    assert np.array_equal(p.last_grow_ids, X.ids) and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j and p._grow_j0 == g.j
    assert set(p.last_relax) == {"rounds", "fell", "sweeps", "words"}
    _held(p.last_relax, X, len(X.ids))
    vg, pts2, par2, vc2 = T2.__dict__["_lazy"]
    live = g.j + g.found
    assert gv2 == vg == g.vgoal and len(pts2) == g.rows and len(par2) == live
    assert np.array_equal(pts2[:live], g.pts[:live]) and np.array_equal(par2, g.parent[:live])
    assert np.array_equal(np.asarray(vc2[:live]).view(np.int64), g.vcost[:live].view(np.int64))
    assert np.array_equal(T2.__dict__["_dub"][0][:live], g.head[:live])
    # the pose calls of the class on the relaxed and grown tree
    v, c, _ = poseref.connect(w.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    pv, pcost, ph = p.connect_poses(w.goals)
    assert np.array_equal(pv, v) and np.array_equal(pcost, c)
    routes, length = p.routes_to_poses(w.goals)
    paths = p.paths_to_poses(T2, w.goals)
    for e in range(len(w.goals)):
        assert (routes[e] is None) == (v[e] < 0) == (paths[e] is None)
        if v[e] >= 0:
            assert np.array_equal(routes[e], paths[e]) and length[e] == c[e]
    cut, cut_len = p.routes_to_poses(w.goals, shortcut=True)
    assert all((a is None) == (b is None) for a, b in zip(cut, routes)) and np.all(cut_len[v >= 0] <= length[v >= 0] + 1e-9)
    # the grown vertices may carry cheaper paths: relax_poses again with the radius passed, and then a third one lowers nothing
    T3, gv3 = p.relax_poses(r)
    T4, gv4 = p.relax_poses(r)
    assert p.last_relax["fell"] == 0 and p.last_relax["rounds"] == 1 and sorted(p.last_grow_ids.tolist()) == list(range(g.j))


def test_rrtdubins_must_pass_r_and_the_straight_line_classes_name_relax():
    w = poseref.workload("D")
    p = RRTDubins(w.og, w.n, w.rho, n_headings=w.nh, pbar=False, seed=poseref.SPECS["D"][7])
    try:
        p.plan(np.array(w.xs), np.array(w.xg))
    except IndexError:
        pass
    j = p.last_stats["j"]
    assert j == w.j
    state = p.rand_gen.bit_generator.state
    _class_golden("no_radius", p.relax_poses)
    assert p._tree_resident == "device" and p.rand_gen.bit_generator.state == state
    X = pc.relaxed(w, pc.WORKLOADS["D"])
    try:
        p.relax_poses(pc.WORKLOADS["D"])
    except IndexError:  # (the plan's own goal not reached: the relaxed tree is resident all the same)
        pass
    assert p.last_relax["fell"] == X.fell and p.last_stats["j"] == j and np.array_equal(p.last_grow_ids, X.ids)
    og = w.og
    q = amd.RRTStar(og, 300, 12, pbar=False)
    _class_golden("straight_line_planner", q.relax_poses, 12)
