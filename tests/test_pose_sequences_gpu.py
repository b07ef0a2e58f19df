"""GPU: mixed histories of keep_pose_tree / grow_poses / relax_poses / connect_poses / pose_routes / rearm / set_query / set_grid on a
Dubins batch of three queries with three (rho, nh), replayed against the host model of tests/posetreemodel.py -- the orders nobody
scripted, as tests/test_tree_sequences_gpu.py has them for the straight-line calls.

After every operation the answer (or the refusal: code and one word of the message) is compared exactly, costs and points bit for
bit; after every grow-like call the batch is asked which stage times answer; and then EVERY query of every batch is asked for its
result (headings included) and for a fixed connect_poses of 8 poses.  The first mismatch ends the sequence; its message names the
sequence and the operation, and posetreemodel.replay(seed, upto) rebuilds that prefix on the CPU."""
import numpy as np
import pytest

import poseroutesref
import posetreemodel as pm
import treemodel as tm
from orchelp import bits
from posecalls import GROW_KERNELS
from rrtplanner_amd import _ffi

pytestmark = pytest.mark.gpu


def _call(f):
    try:
        return f()
    except _ffi.RRTError as e:
        return e


def _answered(got, want):
    if isinstance(want, tm.Refusal):
        assert isinstance(got, _ffi.RRTError), f"expected the refusal {want}, the call answered"
        assert got.code == want.code and want.word in str(got), f"expected the refusal {want}, got {got.code}: {got}"
        return True
    assert not isinstance(got, _ffi.RRTError), f"expected an answer, refused with {getattr(got, 'code', None)}: {got}"
    return False


def _same_tree(res, t):
    assert (res.status, res.j, res.found, res.vgoal, res.rows) == (t.status, t.j, t.found, t.vgoal, t.rows)
    assert np.array_equal(res.pts[:t.live], t.pts[:t.live]) and np.array_equal(res.parent[:t.live], t.parent[:t.live])
    assert np.array_equal(res.head[:t.live], t.head[:t.live])
    assert np.array_equal(bits(res.vcost[:t.live]), bits(t.vcost[:t.live]))
    assert res.sum_j == t.sum_j and res.sum_near == t.sum_near
    if t.log0 is not None:
        lo, hi = t.log0, t.log0 + len(t.accept_log)
        assert np.array_equal(res.nearest_log[lo:hi], t.nearest_log) and np.array_equal(res.accept_log[lo:hi], t.accept_log)
        assert np.array_equal(res.j_log[lo:hi], t.jlog) and res.sum_cells_nn == t.sum_cells_nn


def _same_poses(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def _timers(b, timed):
    how = timed[0] if timed else None
    for name, call, stages in (("grow", b.grow_ms, 3), ("relax", b.relax_poses_ms, 9)):
        got = _call(call)
        if name == how:
            assert not isinstance(got, _ffi.RRTError) and len(got) == stages and all(t >= 0.0 for t in got), f"{name}: {got}"
        else:
            assert isinstance(got, _ffi.RRTError) and got.code == _ffi.RRT_E_ARG, f"the {name} times answer after a {how}: {got}"
    st = _call(b.relax_poses_stats)
    if how == "relax":
        X, j0 = timed[1], timed[2]
        assert not isinstance(st, _ffi.RRTError) and st["fell"] == X["fell"] and 1 <= st["rounds"] <= max(j0, 1), (st, X)
        assert X["sweeps"] <= st["sweeps"] <= st["rounds"] * X["pairs"] and X["words"] <= st["words"] <= st["rounds"] * X["pairs"], (st, X)
    else:
        assert isinstance(st, _ffi.RRTError) and st.code == _ffi.RRT_E_ARG, f"relax_poses_stats answers after a {how}: {st}"


POSE = np.array([(5, 5, 0)], dtype=np.int32)


class PoseBatchDriver:
    def __init__(self, ctx, nbatches, kernel):
        self.ctx, self.kernel = ctx, kernel
        self.maps, _, _ = pm.workload()
        ctx.set_grid(self.maps[0])
        n_cap = max(q[1] for q in pm.QUERIES)
        self.b = [_ffi.Batch(ctx, len(pm.QUERIES), n_cap, logs=True, dubins=True, serial=GROW_KERNELS[kernel][0]) for _ in range(nbatches)]
        self.lines = _ffi.Batch(ctx, 1, 64)  # a straight-line batch of the same context, for the Dubins calls it refuses
        self.keepalive = {}

    def close(self):
        for b in self.b + [self.lines]:
            b.close()

    def _launch(self, b):
        b.launch()
        b.sync()

    def _launched(self, b, ran):
        assert b.team()[1] == 0 and b.team_info()["timeouts"] == 0
        if ran:
            assert b.kernel_name() == GROW_KERNELS[self.kernel][1], b.kernel_name()

    def step(self, op, want):
        kind = op[0]
        if kind == "set_grid":
            self.ctx.set_grid(self.maps[op[1]])
            return
        b = self.b[op[1]]
        if kind == "launch":
            if not _answered(_call(lambda: self._launch(b)), want):
                self._launched(b, want)
        elif kind == "rearm":
            b.rearm()
        elif kind == "rows":
            got = _call(lambda: b.pose_routes_rows(0 if isinstance(want, tm.Refusal) else len(want[1])))
            if not _answered(got, want):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        elif kind == "points":
            got = _call(lambda: b.pose_routes_points(0 if isinstance(want, tm.Refusal) else len(want)))
            if not _answered(got, want):
                assert np.array_equal(bits(got), bits(want))
        elif kind == "pose_calls":
            _answered(_call(lambda: self.lines.relax_poses(0, tm.R2, POSE)), want)
            _answered(_call(lambda: self.lines.connect_poses(0, POSE)), want)
        elif kind == "line_calls":
            _answered(_call(lambda: b.reroot(op[2], 0)), want)
            _answered(_call(lambda: b.relax(op[2], tm.R2)), want)
        elif kind == "set_query":
            s = op[3]
            qu, self.keepalive[op[1:3]] = _ffi.make_query(_ffi.ALG_DUBINS_STAR if s["star"] else _ffi.ALG_DUBINS, s["n"], s["xs"], s["xg"], s["samples"],
                                                          r2_rewire=s["r2"], headings=s["heads"], rho=s["rho"], nh=s["nh"])
            b.set_query(op[2], qu)
        elif kind == "result":
            got = _call(lambda: b.get_result(op[2]))
            if not _answered(got, want):
                _same_tree(got, want)
        elif kind == "keep":
            got = _call(lambda: b.keep_pose_tree(op[2]))
            if not _answered(got, want):
                assert got.dtype == bool and np.array_equal(got, want)
        elif kind in ("grow", "arm", "relax", "relax_arm"):
            got = _call((lambda: b.grow_poses(op[2], op[3])) if kind in ("grow", "arm") else (lambda: b.relax_poses(op[2], op[3], op[4])))
            if not _answered(got, want):
                assert got[0] == want["j0"] and got[2] == want["log0"] and np.array_equal(got[1], want["old_id"])
                if kind in ("grow", "relax"):
                    self._launch(b)
                    self._launched(b, True)
                    _same_tree(b.get_result(op[2]), want["tree"])
        elif kind == "poses":
            got = _call(lambda: b.connect_poses(op[2], op[3]))
            if not _answered(got, want):
                _same_poses(got, want)
        elif kind == "routes":
            got = _call(lambda: b.pose_routes(op[2], op[3], points=op[4], shortcut=op[5]))
            if not _answered(got, want):
                poseroutesref.same(got, want, points=op[4])
        else:
            raise ValueError(kind)

    def timers(self, op, timed):
        if op[0] in ("grow", "arm", "relax", "relax_arm"):
            _timers(self.b[op[1]], timed[op[1]])

    def everyone(self, after):
        for bi, (b, row) in enumerate(zip(self.b, after)):
            for q, (tree, answer) in enumerate(row):
                try:
                    got = _call(lambda: b.get_result(q))
                    if not _answered(got, tree):
                        _same_tree(got, tree)
                    got = _call(lambda: b.connect_poses(q, pm.probe_of(pm.QUERIES[q][4])))
                    if not _answered(got, answer):
                        _same_poses(got, answer)
                    assert b.team_info()["timeouts"] == 0
                except AssertionError as e:
                    raise AssertionError(f"afterwards, query {q} of batch {bi}: {e}") from None


def _replay(driver, steps, label):
    try:
        for k, st in enumerate(steps):
            try:
                driver.step(st.op, st.expect)
                driver.timers(st.op, st.timed)
                driver.everyone(st.after)
            except AssertionError as e:
                raise AssertionError(f"{label}, operation {k} {st.op[:3]!r}: {e}") from None
    finally:
        driver.close()


@pytest.mark.parametrize("seed", pm.POSE_SEEDS)
@pytest.mark.parametrize("kernel", list(GROW_KERNELS))
def test_a_pose_sequence_on_one_batch(gpu_ctx, kernel, seed):
    steps, _ = pm.trace(seed)
    _replay(PoseBatchDriver(gpu_ctx, 1, kernel), steps, f"pose sequence {seed} on the {kernel} kernel (posetreemodel.replay({seed}, k + 1))")


def test_two_pose_batches_on_one_context_take_turns(gpu_ctx):
    a, b = pm.POSE_PAIR
    steps, _ = pm.interleaved(a, b, pm.POSE_PAIR_OPS)
    _replay(PoseBatchDriver(gpu_ctx, 2, "block"), steps,
            f"pose sequences {a} and {b} in turns on two batches (posetreemodel.interleaved({a}, {b}, {pm.POSE_PAIR_OPS}))")


class PoseContextDriver:
    """the single-query operations of posetreemodel._GenPoseOne on Context.plan / keep_pose_tree / grow_poses / relax_poses / connect_poses /
    pose_routes"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.maps, _, _ = pm.workload()
        self.n = pm.ONE[1]
        self.seeded = False  # (the context's own batch outlives a test: its timers are asked once a seed call of this sequence has run)

    def close(self):
        pass

    def _grown(self, got, want):
        if not _answered(got, want):
            rc, res, j0, old_id = got
            assert rc == want["tree"].status and j0 == want["j0"] and np.array_equal(old_id, want["old_id"])
            _same_tree(res, want["tree"])
            self.seeded = True

    def step(self, op, want):
        kind, ctx = op[0], self.ctx
        if kind == "set_grid":
            ctx.set_grid(self.maps[op[1]])
        elif kind == "plan":
            s = op[2]
            ctx.set_grid(self.maps[op[1]])
            qu, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR if s["star"] else _ffi.ALG_DUBINS, s["n"], s["xs"], s["xg"], s["samples"], r2_rewire=s["r2"],
                                       headings=s["heads"], rho=s["rho"], nh=s["nh"])
            rc, res = ctx.plan(qu, s["n"], logs=True)
            assert rc == want.status
            _same_tree(res, want)
        elif kind == "keep1":
            ctx.set_grid(self.maps[op[1]])
            got = ctx.keep_pose_tree()
            assert got.dtype == bool and np.array_equal(got, want)
        elif kind == "grow1":
            self._grown(_call(lambda: ctx.grow_poses(op[1], self.n, logs=True)), want)
        elif kind == "relax1":
            self._grown(_call(lambda: ctx.relax_poses(op[1], op[2], self.n, logs=True)), want)
        elif kind == "poses1":
            got = _call(lambda: ctx.connect_poses(op[1]))
            if not _answered(got, want):
                _same_poses(got, want)
        elif kind == "routes1":
            got = _call(lambda: ctx.pose_routes(op[1], points=op[2], shortcut=op[3]))
            if not _answered(got, want):
                poseroutesref.same(got, want, points=op[2])
        else:
            raise ValueError(kind)

    def timers(self, op, timed):
        if op[0] in ("grow1", "relax1") and self.seeded:
            _timers(self.ctx, timed[0])

    def everyone(self, after):
        got = _call(lambda: self.ctx.connect_poses(pm.probe_of(pm.ONE[4])))
        if not _answered(got, after[0][0][1]):
            _same_poses(got, after[0][0][1])


def test_a_pose_sequence_on_the_contexts_own_batch(gpu_ctx):
    seed = pm.POSE_ONE_SEED
    steps, _ = pm.trace_one(seed)
    _replay(PoseContextDriver(gpu_ctx), steps, f"single-query pose sequence {seed} through Context (posetreemodel.trace_one({seed}))")
