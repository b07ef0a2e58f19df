"""GPU: a finished Dubins tree re-rooted at one of its poses (rrt_pose_reroot_*_kernel, rrt_batch_reroot_poses / rrt_plan_reroot_poses,
rrtplanner_amd.moving), then grown, and the pose tree calls on the result.

Every comparison is exact (==, array_equal, costs as raw bits).  The check is poserootref.py -- the root-first dense input, the edges
swept with the oracle's words, Dijkstra's costs, the cut, the parent rule, the order, the costs summed from the root down -- followed
by posegrowref.grow; and poserelaxref.certify on the arrays the device returned.  The inputs are those of poserootcases.py;
test_pose_reroot_cpu.py says what each is for.  Of the statistics `reached` is exact; the rounds, sweeps and words depend on the order
the wavefronts ran in and are held between Dijkstra's counts and what the rounds could at most do."""
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
import poserootcases as rc
import poserootref
import poseroutesref
import poseshortref
from posecalls import GROW_KERNELS, planned_logged_batch, refused_with_golden_text
from rrtplanner_amd import _ffi, hostprep, moving
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins
from treecalls import same_result, tree_of

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_reroot_refusals.json")) as f:
    GOLDEN = json.load(f)

NONE = np.zeros((0, 3), dtype=np.int32)


def _R(r):
    return pc.R_of(r) if r else 0


def _restate(w, og8, prev, view, root, r, samples, X=None, n=None):
    if X is None:
        X = poserootref.reroot(og8, *prev, root, _R(r), w.rho, w.nh, og8_view=og8 if view else None)
    return X, posegrowref.grow(og8, w.star, w.n if n is None else n, w.xg, w.r2, w.rho, w.nh, X.pts, X.head, X.vcost, X.parent, samples)


def _held(st, X):
    """the statistics of a call against the restatement X: reached exactly, the others within what any order of the wavefronts allows"""
    print("device", st, "restatement", dict(reached=X.reached, cut=X.cut, words=X.words, sweeps=X.sweeps, pairs=X.pairs))
    assert set(st) == {"rounds", "reached", "sweeps", "words"}
    assert st["reached"] == X.reached, (st, X.reached)
    assert 1 <= st["rounds"] <= max(X.G.j, 1), st
    assert X.sweeps <= st["sweeps"] <= st["rounds"] * X.pairs, (st, X.sweeps, X.pairs)
    assert X.words <= st["words"] <= st["rounds"] * X.pairs, (st, X.words, X.pairs)


def _arm(b, q, root, r, samples, X):
    j0, old_id, log0 = moving.batch_reroot_poses(b, q, root, _R(r), samples)
    assert j0 == len(X.ids) == log0 and old_id.dtype == np.int32 and np.array_equal(old_id, X.ids), (j0, len(X.ids), log0)
    ms = moving.reroot_poses_ms(b)
    assert len(ms) == 10 and all(t >= 0.0 for t in ms)
    _held(moving.reroot_poses_stats(b), X)
    return log0


def _reroot(b, q, w, og8, prev, view, root, r, samples, X=None, kernel=None, n=None):
    """one reroot_poses of query q on map og8 of the tree `prev` = (pts, head, parent, vcost, j), launched and checked against the
    restatement and by the certificate.  Returns (Rerooted, Grown, result)."""
    X, g = _restate(w, og8, prev, view, root, r, samples, X, n)
    log0 = _arm(b, q, root, r, samples, X)
    b.launch()
    b.sync()
    res = b.get_result(q)
    same_result(res, g, log0)
    assert b.team()[1] == 0
    assert tuple(res.pts[0]) == tuple(int(c) for c in prev[0][root]) and res.head[0] == prev[1][root] and res.vcost[0] == 0.0
    if kernel:
        assert b.kernel_name() == GROW_KERNELS[kernel][1], b.kernel_name()
    if len(samples) == 0:  # the device's own arrays, by rules of their own
        j0 = len(X.ids)
        assert poserelaxref.certify(og8, res.pts[:j0], res.head[:j0], res.parent[:j0], res.vcost[:j0], _R(r), w.rho, w.nh, poserootref.old_edges_of(X),
                                    prev=X.order) == []
    return X, g, res


# ------------------------------------------------------------------------------------------------ 1. the workloads, the crafted inputs, the sizes
@pytest.mark.parametrize("name", list(pc.WORKLOADS) + list(pc.FIXTURES))
def test_the_workloads_and_the_crafted_inputs_at_four_roots(gpu_ctx, name):
    w, r = rc.workload(name)
    for root in rc.roots_of(w):
        b = planned_logged_batch(gpu_ctx, w, "block")
        _reroot(b, 0, w, w.og8, pc.tree(w), False, root, r, NONE, X=rc.rerooted(w, root, r))
        print(name, root, moving.reroot_poses_stats(b), moving.reroot_poses_ms(b))
        b.close()


def test_trees_of_exactly_1_2_63_to_65_and_1023_to_1025_vertices(gpu_ctx):
    for j in pc.SIZES:
        w, r = rc.workload(f"sized{j}")
        assert w.j == j
        for root in sorted({j - 1, j // 2}):
            b = planned_logged_batch(gpu_ctx, w, "block")
            X, _, res = _reroot(b, 0, w, w.og8, pc.tree(w), False, root, r, NONE, X=rc.rerooted(w, root, r))
            assert res.j == X.reached
            b.close()


@pytest.mark.parametrize("name", ["E", "D"])
def test_r2_0_keeps_exactly_what_hangs_below_the_root(gpu_ctx, name):
    w, r = rc.workload(name)
    for root in rc.roots_of(w):
        b = planned_logged_batch(gpu_ctx, w, "block")
        X, _, res = _reroot(b, 0, w, w.og8, pc.tree(w), False, root, 0, NONE, X=rc.rerooted(w, root, 0))
        st = moving.reroot_poses_stats(b)
        assert (st["rounds"], st["sweeps"], st["words"]) == (1, 0, 0) and res.j == X.reached
        b.close()
    assert rc.rerooted(w, rc.midway(w), 0).reached > 1


# ------------------------------------------------------------------------------------------------ 2. m > 0 on both Dubins kernels
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_reroot_then_grow_on_both_dubins_kernels(gpu_ctx, kernel):
    w, r = rc.workload("D")  # the root cuts a third of the tree: the samples grow it back
    root, m = w.j - 1, 60
    assert rc.rerooted(w, root, r).cut > 20 and w.j + m <= w.n
    s = posegrowref.more_poses(w, w.og8, m, seed=34)
    s[3, :2] = w.ro.pts[root - 1]  # a vertex's cell drawn again
    b = planned_logged_batch(gpu_ctx, w, kernel)
    X, g, res = _reroot(b, 0, w, w.og8, pc.tree(w), False, root, r, s, X=rc.rerooted(w, root, r), kernel=kernel)
    assert g.j >= g.j0 + 5 and g.accept_log.sum() == g.j - g.j0  # (the restatement's own: the samples put vertices back)
    b.close()


# ------------------------------------------------------------------------------------------------ 3. after keep_pose_tree on a changed map
def test_a_kept_view_is_rerooted_among_its_alive_vertices(gpu_ctx):
    k = posekeepref.changed("A")
    w, r = k.w, pc.WORKLOADS["A"]
    root = int(np.flatnonzero(k.alive)[-1])
    b = planned_logged_batch(gpu_ctx, w, "block")
    gpu_ctx.set_grid(k.og8)
    assert np.array_equal(b.keep_pose_tree(0), k.alive) and not k.alive.all()
    X, g, res = _reroot(b, 0, w, k.og8, pc.tree(w), True, root, r, NONE, X=rc.rerooted(w, root, r, k.og8, True))
    assert X.ids[0] == root and set(X.ids.tolist()) <= set(np.flatnonzero(k.alive).tolist())
    v, c, _ = poseref.connect(k.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    got = b.connect_poses(0, w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1].view(np.int64), c.view(np.int64))
    b.close()


# ------------------------------------------------------------------------------------------------ 4. afterwards
def test_the_pose_tree_calls_answer_on_the_rerooted_tree(gpu_ctx):
    w, r = rc.workload("E")
    og8 = w.og8
    root = rc.midway(w)
    b = planned_logged_batch(gpu_ctx, w, "block")
    X, g, res = _reroot(b, 0, w, og8, pc.tree(w), False, root, r, NONE, X=rc.rerooted(w, root, r))
    cur = tree_of(res)
    start = (int(res.pts[0][0]), int(res.pts[0][1]), int(res.head[0]))
    assert start == (int(w.ro.pts[root][0]), int(w.ro.pts[root][1]), int(w.ro.head[root]))
    # connect_poses, and routes with points and shortcuts, in the new numbering
    v, c, _ = poseref.connect(og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    got = b.connect_poses(0, w.goals)
    assert np.array_equal(got[0], v) and np.array_equal(got[1].view(np.int64), c.view(np.int64)) and (v >= 0).sum() >= 1
    poseroutesref.same(b.pose_routes(0, w.goals, points=True), poseroutesref.routes(g.pts, g.head, g.parent, g.j, w.goals, v, c, w.rho, w.nh))
    poseroutesref.same(b.pose_routes(0, w.goals, points=True, shortcut=True),
                       poseshortref.routes(g.pts, g.head, g.parent, g.j, w.goals, v, c, w.rho, w.nh, og8, shortcut=True))
    # relax_poses on the re-rooted tree lowers nothing: it is the shortest-path tree already
    Y = poserelaxref.relax(og8, *cur, pc.R_of(r), w.rho, w.nh)
    gy = posegrowref.grow(og8, w.star, w.n, w.xg, w.r2, w.rho, w.nh, Y.pts, Y.head, Y.vcost, Y.parent, NONE)
    j0, old_id, log0 = b.relax_poses(0, pc.R_of(r))
    assert Y.fell == 0 and b.relax_poses_stats()["fell"] == 0 and np.array_equal(old_id, Y.ids)
    with pytest.raises(_ffi.RRTError):
        moving.reroot_poses_ms(b)  # the stage times are the relax's now
    b.launch()
    b.sync()
    res2 = b.get_result(0)
    same_result(res2, gy, log0)
    # a second reroot_poses, from the new numbers
    cur = tree_of(res2)
    root2 = cur[4] // 2
    X2, g2, res3 = _reroot(b, 0, w, og8, cur, False, root2, r, NONE)
    with pytest.raises(_ffi.RRTError):
        b.relax_poses_ms()
    # keep_pose_tree on a changed map and grow_poses behind it
    cur = tree_of(res3)
    og2 = posekeepref.blocks_map(og8, tuple(int(c) for c in cur[0][0]) + (int(cur[1][0]),))
    alive = posekeepref.alive(og2, cur[0], cur[1], cur[2], cur[4], w.rho, w.nh)
    gpu_ctx.set_grid(og2)
    assert np.array_equal(b.keep_pose_tree(0), alive) and alive[0]
    ids, sp, sh, sc, spar = posegrowref.seed(cur[0], cur[1], cur[2], cur[3], cur[4], alive)
    s = posegrowref.more_poses(w, og2, min(w.n - len(ids), 40), seed=8)
    g3 = posegrowref.grow(og2, w.star, w.n, w.xg, w.r2, w.rho, w.nh, sp, sh, sc, spar, s)
    j0, old_id, log0 = b.grow_poses(0, s)
    assert j0 == len(ids) and np.array_equal(old_id, ids)
    b.launch()
    b.sync()
    same_result(b.get_result(0), g3, log0)
    with pytest.raises(_ffi.RRTError):
        moving.reroot_poses_ms(b)  # the stage times are the grow's now
    # rearm + launch plans the query's own stream from the new start pose
    gpu_ctx.set_grid(og8)
    b.rearm()
    b.launch()
    b.sync()
    res = b.get_result(0)
    xs2 = tuple(int(c) for c in cur[0][0]) + (int(cur[1][0]),)
    samples, heads = np.array(w.samples), np.array(w.heads)
    samples[j0:j0 + len(s)], heads[j0:j0 + len(s)] = s[:, :2], s[:, 2]  # (rows [j0, j0 + m) of the sample buffer hold the grow's samples)
    st, ro = oracle.dubins_plan(og8, w.n, w.star, xs2, w.xg, samples, heads, r2_rewire=w.r2, rho=w.rho, nh=w.nh)
    live = ro.j + (1 if ro.found else 0)
    assert res.status == st and res.j == ro.j and np.array_equal(res.parent[:live], ro.parent[:live]) and np.array_equal(res.head[:live], ro.head[:live])
    assert np.array_equal(res.vcost[:live].view(np.int64), ro.vcost[:live].view(np.int64)) and tuple(res.pts[0]) == xs2[:2] and xs2 != tuple(w.xs)
    b.close()


# ------------------------------------------------------------------------------------------------ 5. refusals
def _raw(call, h, root, r2, s, m, null_j0=False):
    j0, log0 = ctypes.c_int32(-1), ctypes.c_int32(-1)
    rc_ = call(h, 0, int(root), int(r2), s.ctypes.data if s is not None else None, m, None if null_j0 else ctypes.byref(j0), None, ctypes.byref(log0))
    assert (j0.value, log0.value) == (-1, -1)
    return rc_


def test_batch_refusals_have_the_golden_texts_and_change_nothing(gpu_ctx):
    w = poseref.workload("E")
    W, H = w.og8.shape
    R = pc.R_of(12)
    who = "rrt_batch_reroot_poses"
    L = moving._lib()
    call = moving.batch_reroot_poses
    u = _ffi.Batch(gpu_ctx, 1, w.n, dubins=True)
    refused_with_golden_text(GOLDEN, "unfinished_query", call, u, 0, 0, R)
    refused_with_golden_text(GOLDEN, "ms_none", moving.reroot_poses_ms, u)
    refused_with_golden_text(GOLDEN, "stats_none", moving.reroot_poses_stats, u)
    u.close()
    p = _ffi.Batch(gpu_ctx, 1, 100)
    refused_with_golden_text(GOLDEN, "non_dubins_batch", call, p, 0, 0, R)
    p.close()
    b = planned_logged_batch(gpu_ctx, w, "block")
    before = b.get_result(0)
    ok = posegrowref.more_poses(w, w.og8, 4)
    refused_with_golden_text(GOLDEN, "dubins_batch_reroot", b.reroot, 0, 3)  # the straight-line call keeps its answer for a Dubins batch
    refused_with_golden_text(GOLDEN, "q_out_of_range", call, b, 1, 0, R)
    s32 = np.ascontiguousarray(ok, dtype=np.int32)
    assert _raw(L.rrt_batch_reroot_poses, b._h, 3, R, s32, -1) == _ffi.RRT_E_ARG
    assert L.rrt_last_error_string(gpu_ctx.handle).decode() == GOLDEN["m_negative"][1].format(who=who)
    assert _raw(L.rrt_batch_reroot_poses, b._h, 3, R, None, 0, null_j0=True) == _ffi.RRT_E_ARG
    assert L.rrt_last_error_string(gpu_ctx.handle).decode() == GOLDEN["null"][1].format(who=who)
    assert _raw(L.rrt_batch_reroot_poses, b._h, 3, R, None, 2) == _ffi.RRT_E_ARG  # samples announced and none given
    room = w.n - w.j
    fmt = dict(who=who, j=w.j, m=room + 1, n=w.n, room=room)
    refused_with_golden_text(GOLDEN, "room", call, b, 0, 3, R, posegrowref.more_poses(w, w.og8, room + 1), **fmt)
    refused_with_golden_text(GOLDEN, "room", call, b, 0, w.j, -1, posegrowref.more_poses(w, w.og8, room + 1), **fmt)  # the room comes first
    for bad in (-1, w.j, w.j + 7):
        refused_with_golden_text(GOLDEN, "root_outside", call, b, 0, bad, R, ok, who=who, root=bad, j=w.j)
    refused_with_golden_text(GOLDEN, "root_outside", call, b, 0, w.j, -5, ok, who=who, root=w.j, j=w.j)  # the root comes before the radius
    for bad in (-1, -5):
        refused_with_golden_text(GOLDEN, "r2_negative", call, b, 0, 3, bad, ok, who=who, r2=bad)
    bad = ok.copy()
    bad[2, 2] = w.nh
    refused_with_golden_text(GOLDEN, "heading_out_of_range", call, b, 0, 3, R, bad, who=who, nh=w.nh)
    refused_with_golden_text(GOLDEN, "r2_negative", call, b, 0, 3, -1, bad, who=who, r2=-1)  # the radius comes before the samples
    bad = ok.copy()
    bad[1, 0] = W
    refused_with_golden_text(GOLDEN, "cell_outside", call, b, 0, 3, R, bad, who=who, x=W, y=int(bad[1, 1]), W=W, H=H)
    gpu_ctx.set_grid(np.zeros((W + 1, H), dtype=np.uint8))
    refused_with_golden_text(GOLDEN, "grid_shape", call, b, 0, 3, R, who=who, W=W, H=H)
    gpu_ctx.set_grid(w.og8)  # the same cells, another generation
    with pytest.raises(_ffi.RRTError) as e:
        call(b, 0, 3, R)
    assert e.value.code == _ffi.RRT_E_ARG and str(e.value).endswith(GOLDEN["grid_not_kept"][1].split("now)")[1]) and f"{who}: the context's grid was replaced" in str(e.value)
    k = posekeepref.root_blocked(w)
    gpu_ctx.set_grid(k.og8)
    assert not b.keep_pose_tree(0).any()
    refused_with_golden_text(GOLDEN, "root_blocked", call, b, 0, 3, R, who=who)
    # a root that is not alive in the kept view: the view stays
    k2 = posekeepref.changed("E")
    assert k2.w.j == w.j and not k2.alive.all() and k2.alive[0]
    gpu_ctx.set_grid(k2.og8)
    assert np.array_equal(b.keep_pose_tree(0), k2.alive)
    dead = int(np.flatnonzero(~k2.alive)[0])
    refused_with_golden_text(GOLDEN, "root_not_alive", call, b, 0, dead, R, ok, who=who, root=dead, alive=int(k2.alive.sum()), j=w.j)
    refused_with_golden_text(GOLDEN, "root_not_alive", call, b, 0, dead, -1, ok, who=who, root=dead, alive=int(k2.alive.sum()), j=w.j)
    gpu_ctx.set_grid(w.og8)
    assert b.keep_pose_tree(0).all()
    after = b.get_result(0)
    for name in ("pts", "vcost", "parent", "head"):
        assert np.array_equal(getattr(before, name), getattr(after, name))
    assert (after.status, after.j, after.found, after.vgoal) == (before.status, before.j, before.found, before.vgoal)
    v, c = b.connect_poses(0, w.goals)  # ... and the tree still answers as it did
    assert np.array_equal(v, w.vertex) and np.array_equal(c, w.cost)
    refused_with_golden_text(GOLDEN, "ms_none", moving.reroot_poses_ms, b)
    b.close()


def test_plan_refusals_and_the_call_through_rrt_plan():
    w = poseref.workload("D")  # RRTDubins: the planner without a near set
    r = pc.WORKLOADS["D"]
    R = pc.R_of(r)
    root = w.j - 1
    who = "rrt_plan_reroot_poses"
    ctx = _ffi.Context(0)
    ctx.set_grid(w.og8)
    refused_with_golden_text(GOLDEN, "no_plan", moving.context_reroot_poses, ctx, root, R, NONE, w.n)
    refused_with_golden_text(GOLDEN, "plan_ms_none", moving.reroot_poses_ms, ctx)
    qu, keep = poseref.device_query(w)
    rc_, res = ctx.plan(qu, w.n)
    assert rc_ == w.status and res.j == w.j
    ans0 = ctx.connect_poses(w.goals)

    def refused(key, vertex, threshold, samples, **fmt):
        code, text = GOLDEN[key]
        with pytest.raises(_ffi.RRTError) as e:
            moving.context_reroot_poses(ctx, vertex, threshold, samples, w.n)
        assert e.value.code == code and not e.value.seeded and str(e.value) == f"librrt_hip error {code}: {text.format(who=who, **fmt)}", str(e.value)

    room = w.n - w.j
    refused("room", root, R, posegrowref.more_poses(w, w.og8, room + 1), j=w.j, m=room + 1, n=w.n, room=room)
    refused("root_outside", w.j, R, NONE, root=w.j, j=w.j)
    refused("r2_negative", root, -1, NONE, r2=-1)
    bad = posegrowref.more_poses(w, w.og8, 3)
    bad[2, 2] = w.nh
    refused("heading_out_of_range", root, R, bad, nh=w.nh)
    j0 = ctypes.c_int32(-1)
    L = moving._lib()
    assert L.rrt_plan_reroot_poses(ctx.handle, root, R, None, -1, ctypes.byref(j0), None, ctypes.byref(res.c)) == _ffi.RRT_E_ARG and j0.value == -1
    assert L.rrt_plan_reroot_poses(ctx.handle, root, R, None, 0, ctypes.byref(j0), None, None) == _ffi.RRT_E_ARG
    got = ctx.connect_poses(w.goals)
    assert np.array_equal(got[0], ans0[0]) and np.array_equal(got[1], ans0[1])
    # and the call itself equals the restatement
    s = posegrowref.more_poses(w, w.og8, min(30, room), seed=5)
    assert len(s) >= 10
    X, g = _restate(w, w.og8, pc.tree(w), False, root, r, s, rc.rerooted(w, root, r))
    assert g.accept_log.sum() >= 1  # (the samples put vertices on the re-rooted tree)
    rc_, out, j0, old_id = moving.context_reroot_poses(ctx, root, R, s, w.n)
    assert rc_ == g.status and j0 == len(X.ids) and np.array_equal(old_id, X.ids) and len(moving.reroot_poses_ms(ctx)) == 10
    _held(moving.reroot_poses_stats(ctx), X)
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


def test_rrtstardubins_reroot_poses_is_the_restatement_fed_with_the_same_draws():
    w = poseref.workload("E")
    r, seed = poseref.SPECS["E"][4], poseref.SPECS["E"][7]
    p = RRTStarDubins(w.og, w.n, r, w.rho, n_headings=w.nh, pbar=False, seed=seed)
    with pytest.raises(RuntimeError):
        moving.reroot_poses(p, 3)
    T, gv = p.plan(np.array(w.xs), np.array(w.xg))
    assert p.last_stats["j"] == w.j and p._grow_j0 == w.j
    root = rc.midway(w)
    _class_golden("dubins_planner_reroot", p.reroot, root)
    _class_golden("radius_negative", moving.reroot_poses, p, root, -1)
    _class_golden("vertex_negative_class", moving.reroot_poses, p, -1)
    _class_golden("room_class", lambda: moving.reroot_poses(p, root, m=w.n - w.j + 1), j=w.j, n=w.n, room=w.n - w.j, m=w.n - w.j + 1)
    _class_golden("m_negative_class", lambda: moving.reroot_poses(p, root, m=-1))
    state = p.rand_gen.bit_generator.state
    _class_golden("root_class", lambda: moving.reroot_poses(p, w.j, m=5), root=w.j, j=w.j)
    assert p._tree_resident == "device" and p.rand_gen.bit_generator.state == state  # a refused vertex spends no draws
    m = 40
    twin = np.random.default_rng(0)
    twin.bit_generator.state = p.rand_gen.bit_generator.state
    cells = hostprep.draw_free_samples(twin, np.argwhere(w.og8 == 0), m)
    s = np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), twin.integers(0, w.nh, m)])
    X, g = _restate(w, w.og8, pc.tree(w), False, root, r, s, rc.rerooted(w, root, r))
    T2, gv2 = moving.reroot_poses(p, root, m=m)  # r defaults to r_rewire
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state
    assert np.array_equal(p.last_grow_ids, X.ids) and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j and p._grow_j0 == g.j
    _held(p.last_relax, X)
    vg, pts2, par2, vc2 = T2.__dict__["_lazy"]
    live = g.j + g.found
    assert gv2 == vg == g.vgoal and len(pts2) == g.rows and len(par2) == live
    assert np.array_equal(pts2[:live], g.pts[:live]) and np.array_equal(par2, g.parent[:live])
    assert np.array_equal(np.asarray(vc2[:live]).view(np.int64), g.vcost[:live].view(np.int64))
    assert np.array_equal(T2.__dict__["_dub"][0][:live], g.head[:live])
    # the pose calls of the class on the re-rooted and grown tree
    v, c, _ = poseref.connect(w.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    pv, pcost, ph = p.connect_poses(w.goals)
    assert np.array_equal(pv, v) and np.array_equal(pcost, c)
    # again with the radius passed, at r = 0: what hangs below the vertex
    cur = (g.pts[:g.j], g.head[:g.j], g.parent[:g.j], g.vcost[:g.j], g.j)
    X0 = poserootref.reroot(w.og8, *cur, 1, 0, w.rho, w.nh)
    try:
        moving.reroot_poses(p, 1, 0)
    except IndexError:  # (the plan's own goal not reached from there: the tree is resident all the same)
        pass
    assert np.array_equal(p.last_grow_ids, X0.ids) and p.last_relax["reached"] == X0.reached and p.last_stats["j"] == X0.reached


def test_rrtdubins_must_pass_r_and_the_straight_line_classes_name_reroot():
    w = poseref.workload("D")
    p = RRTDubins(w.og, w.n, w.rho, n_headings=w.nh, pbar=False, seed=poseref.SPECS["D"][7])
    try:
        p.plan(np.array(w.xs), np.array(w.xg))
    except IndexError:
        pass
    j = p.last_stats["j"]
    assert j == w.j
    state = p.rand_gen.bit_generator.state
    _class_golden("no_radius", moving.reroot_poses, p, w.j - 1)
    assert p._tree_resident == "device" and p.rand_gen.bit_generator.state == state
    # m > 0 on the planner without a near set, fed with the same draws: m free cells, then m heading indices
    r, root = pc.WORKLOADS["D"], w.j - 1
    m = min(30, w.n - w.j)
    assert m >= 10
    twin = np.random.default_rng(0)
    twin.bit_generator.state = state
    cells = hostprep.draw_free_samples(twin, np.argwhere(w.og8 == 0), m)
    s = np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), twin.integers(0, w.nh, m)])
    X, g = _restate(w, w.og8, pc.tree(w), False, root, r, s, rc.rerooted(w, root, r))
    assert g.accept_log.sum() >= 1
    try:
        moving.reroot_poses(p, root, r, m)
    except IndexError:  # (the plan's own goal not reached: the re-rooted tree is resident all the same)
        assert not g.found
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state and p._tree_resident == "device"
    assert np.array_equal(p.last_grow_ids, X.ids) and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j and p._grow_j0 == g.j
    _held(p.last_relax, X)
    v, c, _ = poseref.connect(w.og8, g.pts, g.head, g.vcost, g.j, w.goals, w.rho, w.nh)
    pv, pcost, ph = p.connect_poses(w.goals)
    assert np.array_equal(pv, v) and np.array_equal(pcost, c)
    q = amd.RRTStar(w.og, 300, 12, pbar=False)
    _class_golden("straight_line_planner", moving.reroot_poses, q, 3, 12)


def test_the_class_after_keep_pose_tree_refuses_a_dead_vertex_and_reroots_at_an_alive_one():
    k = posekeepref.changed("E")
    w = k.w
    r, seed = poseref.SPECS["E"][4], poseref.SPECS["E"][7]
    p = RRTStarDubins(w.og, w.n, r, w.rho, n_headings=w.nh, pbar=False, seed=seed)
    p.plan(np.array(w.xs), np.array(w.xg))
    alive = p.keep_pose_tree(k.og8.astype(np.asarray(w.og).dtype))
    assert np.array_equal(alive, k.alive) and not k.alive.all() and k.alive[0]
    dead, root = int(np.flatnonzero(~k.alive)[0]), int(np.flatnonzero(k.alive)[-1])
    state = p.rand_gen.bit_generator.state
    _class_golden("root_dead_class", lambda: moving.reroot_poses(p, dead, m=5), root=dead, alive=int(k.alive.sum()), j=w.j)
    assert p._tree_resident == "device" and p.rand_gen.bit_generator.state == state and p._grow_j0 == int(k.alive.sum())  # no draw spent, the view stays
    m = 20
    twin = np.random.default_rng(0)
    twin.bit_generator.state = state
    cells = hostprep.draw_free_samples(twin, np.argwhere(k.og8 == 0), m)
    s = np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), twin.integers(0, w.nh, m)])
    X, g = _restate(w, k.og8, pc.tree(w), True, root, r, s, rc.rerooted(w, root, r, k.og8, True))
    try:
        moving.reroot_poses(p, root, m=m)
    except IndexError:
        assert not g.found
    assert p.rand_gen.bit_generator.state == twin.bit_generator.state
    assert np.array_equal(p.last_grow_ids, X.ids) and p.last_stats["j"] == g.j and p.last_stats["sum_j"] == g.sum_j and p._grow_j0 == g.j
    _held(p.last_relax, X)
