"""GPU: long mixed histories of keep_tree / grow / reroot / relax / connect_goals / routes / rearm / set_query / set_grid on one batch, replayed against
the host model of tests/treemodel.py -- the orders nobody scripted.

After every operation the answer (or the refusal: code and one word of the message) is compared exactly, and then EVERY query of
every batch is asked for its result and for a fixed goals call, which have to be what the model says: an operation must not change a
query it did not name, whether it succeeded or was refused.  The first mismatch ends the sequence; its message names the sequence, the
driver and the operation, and treemodel.replay(seed, upto) rebuilds that prefix on the CPU.  tests/test_tree_sequences_cpu.py holds the
same seeds to the conditions that make the sequences worth running.  After every grow, reroot or relax, refused or not, the batch is
also asked for the stage times of all three and for the relax counters: only those of the last such call that ran answer."""
import itertools

import numpy as np
import pytest

import growref
import oracle
import treemodel as tm
from orchelp import bits
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.oggen import DeviceGrids
from treecalls import SHAPES, shape_ran, tree_of

pytestmark = pytest.mark.gpu


def _call(f):
    try:
        return f()
    except _ffi.RRTError as e:
        return e


def _answered(got, want):
    """`got` is what the call gave or the RRTError it raised; want a Refusal: the same refusal.  Returns True for a refusal."""
    if isinstance(want, tm.Refusal):
        assert isinstance(got, _ffi.RRTError), f"expected the refusal {want}, the call answered"
        assert got.code == want.code and want.word in str(got), f"expected the refusal {want}, got {got.code}: {got}"
        return True
    assert not isinstance(got, _ffi.RRTError), f"expected an answer, refused with {getattr(got, 'code', None)}: {got}"
    return False


def _same_tree(res, t, logs=True):
    assert (res.status, res.j, res.found, res.vgoal, res.rows) == (t.status, t.j, t.found, t.vgoal, t.rows)
    assert np.array_equal(res.pts[:t.live], t.pts[:t.live]) and np.array_equal(res.parent[:t.live], t.parent[:t.live])
    assert np.array_equal(bits(res.vcost[:t.live]), bits(t.vcost[:t.live]))
    assert res.sum_j == t.sum_j and res.sum_near == t.sum_near  # the statistics of the last run: a grow counts its own iterations alone
    if logs and t.log0 is not None:
        lo, hi = t.log0, t.log0 + len(t.accept_log)
        assert np.array_equal(res.nearest_log[lo:hi], t.nearest_log) and np.array_equal(res.accept_log[lo:hi], t.accept_log)
        assert np.array_equal(res.j_log[lo:hi], t.jlog)


def _same_goals(got, want):
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))


def _same_routes(got, want):
    assert len(got) == len(want) == 6
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(bits(x), bits(y)) if k in (1, 2) else np.array_equal(x, y), k


def _seeded(got, want):
    """what a grow, a reroot or a relax call answered: (j0, old_id, log0)"""
    assert got[0] == want["j0"] and got[2] == want["log0"] and np.array_equal(got[1], want["old_id"])


def _timers(o, timed):
    """`o` (a Batch or a Context) is asked for the stage times of all three seed calls and for the relax counters: only those of the
    last seed call that ran answer -- timed = (call, the relax's fell, its j0), None: no seed call has run --, the others are refused"""
    how = timed[0] if timed else None
    for name, stages in (("grow", 3), ("reroot", 8), ("relax", 9)):
        got = _call(getattr(o, name + "_ms"))
        if name == how:
            assert not isinstance(got, _ffi.RRTError) and len(got) == stages and all(t >= 0.0 for t in got), f"{name}_ms after a {how}: {got}"
        else:
            assert isinstance(got, _ffi.RRTError) and got.code == _ffi.RRT_E_ARG, f"{name}_ms answers after a {how}: {got}"
    st = _call(o.relax_stats)
    if how == "relax":
        assert not isinstance(st, _ffi.RRTError) and st["fell"] == timed[1] and 1 <= st["rounds"] <= max(timed[2], 1), (st, timed)
    else:
        assert isinstance(st, _ffi.RRTError) and st.code == _ffi.RRT_E_ARG, f"relax_stats answers after a {how}: {st}"


POSE = np.array([(5, 5, 0)], dtype=np.int32)  # a pose for the Dubins calls that a straight-line batch refuses
RADIUS = {hostprep.radius_threshold(r): r for r in tm.RELAX_R}  # the planner classes take the radius, the calls its threshold


class BatchDriver:
    """the operations of treemodel on _ffi.Batch objects of one context"""

    def __init__(self, ctx, nbatches=1, shape="team"):
        self.ctx, self.shape = ctx, shape
        self.maps, self.xs, _ = tm.workload()
        ctx.set_grid(self.maps[0])  # (a batch takes its shape from the context's grid)
        self.b = [_ffi.Batch(ctx, len(tm.NS), max(tm.NS), logs=True, **SHAPES[shape][0]) for _ in range(nbatches)]
        self.keepalive = {}

    def close(self):
        for b in self.b:
            b.close()

    def _launched(self, b, ran):
        info = b.team_info()
        assert info["timeouts"] == 0 and b.team()[1] == 0, info
        if ran:
            shape_ran(b, self.shape, Q=len(tm.NS))  # (three queries: "team" and "team64" are held to the launch plan's name for three)

    def _launch(self, b):
        b.launch()
        b.sync()

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
            rows = 0 if isinstance(want, tm.Refusal) else len(want[1])
            got = _call(lambda: b.routes_rows(rows))
            if not _answered(got, want):
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        elif kind == "set_query":
            s = op[3]
            qu, self.keepalive[op[1:3]] = _ffi.make_query(s["alg"], s["n"], self.xs, s["xg"], s["samples"], r2_rewire=tm.R2 if s["alg"] else 0)
            b.set_query(op[2], qu)
        elif kind == "result":
            got = _call(lambda: b.get_result(op[2]))
            if not _answered(got, want):
                _same_tree(got, want)
        elif kind == "keep":
            got = _call(lambda: b.keep_tree(op[2]))
            if not _answered(got, want):
                assert got.dtype == bool and np.array_equal(got, want)
        elif kind in tm.SEED_OPS:
            call = tm.ARMS.get(kind, kind)
            got = _call(lambda: getattr(b, call)(*op[2:]))  # grow(q, samples), reroot(q, root, samples), relax(q, r2, samples)
            if not _answered(got, want):
                _seeded(got, want)
                if kind not in tm.ARMS:
                    self._launch(b)
                    self._launched(b, True)
                    _same_tree(b.get_result(op[2]), want["tree"])
        elif kind == "pose_calls":
            _answered(_call(lambda: b.relax_poses(op[2], tm.R2, POSE)), want)
            _answered(_call(lambda: b.connect_poses(op[2], POSE)), want)
        elif kind == "goals":
            got = _call(lambda: b.connect_goals(op[2], op[3]))
            if not _answered(got, want):
                _same_goals(got, want)
        elif kind == "routes":
            got = _call(lambda: b.routes(op[2], op[3], shortcut=op[4]))
            if not _answered(got, want):
                _same_routes(got, want)
        else:
            raise ValueError(kind)

    def timers(self, op, timed):
        if op[0] in tm.SEED_OPS:
            _timers(self.b[op[1]], timed[op[1]])

    def everyone(self, after, probe):
        """every query of every batch: its result and the probe goals call, as the model has them after the operation"""
        for bi, (b, row) in enumerate(zip(self.b, after)):
            for q, (tree, answer) in enumerate(row):
                try:
                    got = _call(lambda: b.get_result(q))
                    if not _answered(got, tree):
                        _same_tree(got, tree)
                    got = _call(lambda: b.connect_goals(q, probe))
                    if not _answered(got, answer):
                        _same_goals(got, answer)
                    assert b.team_info()["timeouts"] == 0
                except AssertionError as e:
                    raise AssertionError(f"afterwards, query {q} of batch {bi}: {e}") from None


def _replay(driver, steps, label):
    try:
        for k, st in enumerate(steps):
            try:
                driver.step(st.op, st.expect)
                driver.timers(st.op, st.timed)
                driver.everyone(st.after, tm.PROBE)
            except AssertionError as e:
                raise AssertionError(f"{label}, operation {k} {st.op[:3]!r}: {e}") from None
    finally:
        driver.close()


# ------------------------------------------------------------------------------------------------ 1. one batch, every launch shape
@pytest.mark.parametrize("shape, seed", list(zip(SHAPES, tm.SEEDS)))
def test_a_sequence_on_one_batch(gpu_ctx, shape, seed):
    steps, _ = tm.trace(seed)
    _replay(BatchDriver(gpu_ctx, 1, shape), steps, f"sequence {seed} on a batch of shape {shape} (treemodel.replay({seed}, k + 1))")


# ------------------------------------------------------------------------------------------------ 2. two batches, one context
def test_two_batches_on_one_context_take_turns(gpu_ctx):
    a, b = tm.PAIR
    steps, _ = tm.interleaved(a, b)
    _replay(BatchDriver(gpu_ctx, 2, "team"), steps, f"sequences {a} and {b} in turns on two batches (treemodel.interleaved({a}, {b}))")


# ------------------------------------------------------------------------------------------------ 3. the context's own batch
class ContextDriver:
    """the single-query operations of treemodel._GenOne on Context.plan / keep_tree / grow / connect_goals / routes"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.maps, self.xs, _ = tm.workload()

    def close(self):
        pass

    def step(self, op, want):
        kind, ctx = op[0], self.ctx
        if kind == "set_grid":
            ctx.set_grid(self.maps[op[1]])
        elif kind == "plan":
            s = op[2]
            ctx.set_grid(self.maps[op[1]])
            qu, keep = _ffi.make_query(s["alg"], s["n"], self.xs, s["xg"], s["samples"], r2_rewire=tm.R2 if s["alg"] else 0)
            self.n = s["n"]  # (the tree calls of the context take the n of its plan)
            rc, res = ctx.plan(qu, s["n"], logs=True)
            assert rc == want.status
            _same_tree(res, want)
        elif kind == "keep1":
            ctx.set_grid(self.maps[op[1]])
            got = ctx.keep_tree()
            assert got.dtype == bool and np.array_equal(got, want)
        elif kind == "grow1":
            got = _call(lambda: ctx.grow(op[1], self.n, logs=True))
            if not _answered(got, want):
                rc, res, j0, old_id = got
                assert rc == want["tree"].status and j0 == want["j0"] and np.array_equal(old_id, want["old_id"])
                _same_tree(res, want["tree"])
        elif kind in ("reroot1", "relax1"):
            got = _call(lambda: getattr(ctx, kind[:-1])(op[1], op[2], self.n, logs=True))
            if not _answered(got, want):
                rc, res, j0, old_id = got
                assert rc == want["tree"].status and j0 == want["j0"] and np.array_equal(old_id, want["old_id"])
                _same_tree(res, want["tree"])
        elif kind == "pose_calls1":
            _answered(_call(lambda: ctx.relax_poses(tm.R2, POSE, self.n)), want)
            _answered(_call(lambda: ctx.connect_poses(POSE)), want)
        elif kind == "goals1":
            got = _call(lambda: ctx.connect_goals(op[1]))
            if not _answered(got, want):
                _same_goals(got, want)
        elif kind == "routes1":
            got = _call(lambda: ctx.routes(op[1], shortcut=op[2]))
            if not _answered(got, want):
                _same_routes(got, want)
        else:
            raise ValueError(kind)

    def timers(self, op, timed):
        """(the context's own batch outlives a test: what it answers before the sequence's first seed call has run is another test's)"""
        if op[0] in ("grow1", "reroot1", "relax1") and timed[0]:
            _timers(self.ctx, timed[0])

    def everyone(self, after, probe):
        got = _call(lambda: self.ctx.connect_goals(probe))
        if not _answered(got, after[0][0][1]):
            _same_goals(got, after[0][0][1])


@pytest.mark.parametrize("seed", tm.ONE_SEEDS[:2])
def test_a_sequence_on_the_contexts_own_batch(gpu_ctx, seed):
    steps, _ = tm.trace_one(seed)
    _replay(ContextDriver(gpu_ctx), steps, f"single-query sequence {seed} through Context (treemodel.trace_one({seed}))")


# ------------------------------------------------------------------------------------------------ 4. the planner classes
class PlannerDriver:
    """the same operations on RRTStandard / RRTStar: plan / keep_tree / grow / connect_goals / routes_to / set_og / set_n.  The planner
    draws its own samples: its stream starts where the sequence's draw stream stood and has to stand where that one stands after every
    operation.  What the engine refuses the classes refuse on the host, with ValueError or RuntimeError."""

    def __init__(self):
        self.maps, self.xs, _ = tm.workload()
        self.p = None
        self.draws_state = None
        self.seeded = False

    def close(self):
        self.p = None

    def _og(self, k):
        return self.maps[k].astype(np.int64)

    def _tree(self, out, t):
        T, gv = out
        vg, pts, par, vc = T.__dict__["_lazy"]
        assert gv == vg == t.vgoal and len(pts) == t.rows and len(par) == t.live
        assert np.array_equal(pts[:t.live], t.pts[:t.live]) and np.array_equal(par, t.parent[:t.live])
        assert np.array_equal(bits(np.asarray(vc[:t.live])), bits(t.vcost[:t.live]))

    def _run(self, call, t):
        """plan() and grow() raise IndexError where the reference does (no vertex sees the goal and rows are left); the tree is there all the same"""
        if t.status == growref.ST_UNREACHABLE:
            with pytest.raises(IndexError):
                call()
        else:
            self._tree(call(), t)
        st = self.p.last_stats
        assert (st["j"], st["sum_j"], st["sum_near"]) == (t.j, t.sum_j, t.sum_near) and self.p.last_route == "kernel" and self.p._tree_resident == "device"

    def _refused_by_class(self, call, want):
        with pytest.raises((ValueError, RuntimeError)) as e:
            call()
        if want.word in ("room for", "nothing to grow from", "is not alive", "has the vertices [0,"):
            assert want.word in str(e.value), e.value

    def step(self, op, want):
        kind = op[0]
        if kind == "set_grid":
            self.p.set_og(self._og(op[1]))
        elif kind == "plan":
            s = op[2]
            cls = amd.RRTStar if s["alg"] else amd.RRTStandard
            if type(self.p) is not cls:
                self.p = cls(self._og(op[1]), s["n"], tm.RR, pbar=False) if s["alg"] else cls(self._og(op[1]), s["n"], pbar=False)
                self.p.rand_gen.bit_generator.state = s["draws_state"]
                self.seeded = False  # (a new planner has a context of its own: no seed call has run on it)
            else:
                self.p.set_og(self._og(op[1]))
                self.p.set_n(s["n"])
            self._run(lambda: self.p.plan(self.xs, s["xg"]), want)
        elif kind == "keep1":
            got = self.p.keep_tree(self._og(op[1]))
            assert got.dtype == bool and np.array_equal(got, want)
        elif kind == "grow1":
            if isinstance(want, tm.Refusal):
                self._refused_by_class(lambda: self.p.grow(len(op[1])), want)
            else:
                self._run(lambda: self.p.grow(len(op[1])), want["tree"])
                assert np.array_equal(self.p.last_grow_ids, want["old_id"])
        elif kind in ("reroot1", "relax1"):
            call = (lambda: self.p.reroot(op[1], len(op[2]))) if kind == "reroot1" else (lambda: self.p.relax(RADIUS[op[1]], len(op[2])))
            if isinstance(want, tm.Refusal):
                self._refused_by_class(call, want)
            else:
                self._run(call, want["tree"])
                assert np.array_equal(self.p.last_grow_ids, want["old_id"])
                if kind == "relax1":
                    assert self.p.last_relax["fell"] == want["fell"] and 1 <= self.p.last_relax["rounds"] <= max(want["j0"], 1)
        elif kind == "pose_calls1":
            for call in (lambda: self.p.relax_poses(tm.RR, 1), lambda: self.p.connect_poses(POSE)):
                with pytest.raises(ValueError):
                    call()
        elif kind == "goals1":
            if isinstance(want, tm.Refusal):
                self._refused_by_class(lambda: self.p.connect_goals(op[1]), want)
            else:
                _same_goals(self.p.connect_goals(op[1]), want)
        elif kind == "routes1":
            if isinstance(want, tm.Refusal):
                self._refused_by_class(lambda: self.p.routes_to(op[1], shortcut=op[2]), want)
            else:
                routes, length = self.p.routes_to(op[1], shortcut=op[2])
                assert np.array_equal(bits(length), bits(want[2])) and len(routes) == len(op[1])
                for k, r in enumerate(routes):
                    lo, hi = want[3][k], want[3][k + 1]
                    assert (r is None and lo == hi) or np.array_equal(r, want[4][lo:hi]), k
        else:
            raise ValueError(kind)

    def timers(self, op, timed, ran):
        self.seeded = self.seeded or ran
        if op[0] in ("grow1", "reroot1", "relax1") and self.seeded:
            _timers(self.p.device_context(), timed[0])

    def everyone(self, after, probe):
        want = after[0][0][1]
        if isinstance(want, tm.Refusal):
            self._refused_by_class(lambda: self.p.connect_goals(probe), want)
        else:
            _same_goals(self.p.connect_goals(probe), want)
        assert self.p.rand_gen.bit_generator.state == self.draws_state, "the planner's stream is not where the sequence's draws stand"


def _replay_on_the_planner_classes(seed):
    steps, _ = tm.trace_one(seed)
    d = PlannerDriver()
    for k, st in enumerate(steps):
        try:
            d.draws_state = st.draws_state
            d.step(st.op, st.expect)
            d.timers(st.op, st.timed, st.op[0] in ("grow1", "reroot1", "relax1") and not isinstance(st.expect, tm.Refusal))
            d.everyone(st.after, tm.PROBE)
        except AssertionError as e:
            raise AssertionError(f"single-query sequence {seed} through the planner classes (treemodel.trace_one({seed})), operation {k} {st.op[:2]!r}: {e}") from None


@pytest.mark.parametrize("seed", tm.ONE_SEEDS[2:])
def test_a_sequence_on_the_planner_classes(seed):
    _replay_on_the_planner_classes(seed)


# ------------------------------------------------------------------------------------------------ 5. the sequences with reroot and relax
@pytest.mark.parametrize("shape, seed", list(zip(SHAPES, itertools.cycle(tm.ROOT_SEEDS))))
def test_a_reroot_and_relax_sequence_on_one_batch(gpu_ctx, shape, seed):
    steps, _ = tm.trace(seed)
    _replay(BatchDriver(gpu_ctx, 1, shape), steps, f"sequence {seed} on a batch of shape {shape} (treemodel.replay({seed}, k + 1))")


def test_two_batches_take_turns_with_reroot_and_relax(gpu_ctx):
    a, b = tm.ROOT_PAIR
    steps, _ = tm.interleaved(a, b, tm.ROOT_PAIR_OPS)
    _replay(BatchDriver(gpu_ctx, 2, "team"), steps, f"sequences {a} and {b} in turns on two batches (treemodel.interleaved({a}, {b}, {tm.ROOT_PAIR_OPS}))")


@pytest.mark.parametrize("seed", tm.ROOT_ONE_SEEDS)
def test_a_reroot_and_relax_sequence_on_the_contexts_own_batch(gpu_ctx, seed):
    steps, _ = tm.trace_one(seed)
    _replay(ContextDriver(gpu_ctx), steps, f"single-query sequence {seed} through Context (treemodel.trace_one({seed}))")


@pytest.mark.parametrize("seed", tm.ROOT_ONE_SEEDS)
def test_a_reroot_and_relax_sequence_on_the_planner_classes(seed):
    _replay_on_the_planner_classes(seed)


# ------------------------------------------------------------------------------------------------ 6. armed on one map, launched on another
def _grown(n, g, j0):
    return tm.Tree(n, g.pts, g.parent, g.vcost, g.j, g.found, g.vgoal, g.status, g.sum_j, g.sum_near, j0, g.nearest_log, g.accept_log, g.jlog)


def _refused_arg(call, word=""):
    with pytest.raises(_ffi.RRTError) as e:
        call()
    assert e.value.code == _ffi.RRT_E_ARG and word in str(e.value), e.value
    return str(e.value)


@pytest.mark.parametrize("shape", ["team", "pipe1"])
def test_a_grow_armed_on_one_map_is_not_launched_on_another(gpu_ctx, shape):
    """The seed's edges were tested on the map of the grow call; a launch on another map would stamp that map on all of them.  The
    launch is refused and the query stays armed; a set_grid of the first map's cells is a new generation all the same, so it stays
    refused; rearm lifts the refusal as it undoes an armed grow, and the query runs again from its sample buffer as it stands."""
    maps, xs, xgs = tm.workload()
    n = tm.NS[1]
    gpu_ctx.set_grid(maps[tm.MAP_A])
    b = _ffi.Batch(gpu_ctx, 1, n, logs=True, **SHAPES[shape][0])
    rng = np.random.default_rng(3)
    samples = hostprep.draw_free_samples(rng, np.argwhere(maps[tm.MAP_A] == 0), n)
    qu, keep = _ffi.make_query(1, n, xs, xgs[1], samples, r2_rewire=tm.R2)
    b.set_query(0, qu)
    b.launch()
    b.sync()
    gpu_ctx.set_grid(maps[tm.MAP_WALL])
    alive = b.keep_tree(0)
    assert 0.05 <= (~alive).mean() <= 0.95
    more = hostprep.draw_free_samples(rng, np.argwhere(maps[tm.MAP_WALL] == 0), 40)
    gen_seed = gpu_ctx.grid_generation()
    j0, old_id, log0 = b.grow(0, more)
    assert j0 == alive.sum() and np.array_equal(old_id, np.flatnonzero(alive))
    gpu_ctx.set_grid(maps[tm.MAP_B])  # same shape, other obstacles across the seed
    msg = _refused_arg(b.launch, "seeded")
    assert "query 0" in msg and f"generation {gen_seed} then, {gpu_ctx.grid_generation()} now" in msg
    for call in (lambda: b.get_result(0), lambda: b.connect_goals(0, [(5, 5)]), lambda: b.grow(0, more), lambda: b.keep_tree(0)):
        _refused_arg(call)  # query 0 is armed and not launched, as it was
    gpu_ctx.set_grid(maps[tm.MAP_WALL])  # the same cells, a new generation
    _refused_arg(b.launch, "seeded")
    b.rearm()
    b.launch()
    b.sync()
    buf = samples.copy()
    buf[j0:j0 + len(more)] = more
    st, ro = oracle.plan(maps[tm.MAP_WALL], n, 1, xs, xgs[1], buf, r2_rewire=tm.R2)
    _same_tree(b.get_result(0), tm.Tree(n, ro.pts, ro.parent, ro.vcost, ro.j, ro.found, ro.vgoal, st, ro.sum_j, ro.sum_near, None, None, None, None))
    shape_ran(b, shape)  # (one query: "team" is two shifts)
    assert b.team_info()["timeouts"] == 0
    b.close()


def test_a_grow_armed_on_a_resident_frame_runs_when_that_frame_is_back(gpu_ctx):
    """Resident frames share one generation and differ in the grid: select_frame to another frame refuses the launch and drops
    nothing -- the view and the route rows of the other query are still there --, select_frame back runs the grow, which is growref's."""
    grids = DeviceGrids(gpu_ctx, tm.W, tm.H, thresh=0.33, frames=2, seed=5)
    og = [np.ascontiguousarray(f != 0, dtype=np.uint8) for f in grids.host]
    free = np.argwhere((og[0] == 0) & (og[1] == 0))
    rng = np.random.default_rng(8)
    xs, xg = free[rng.integers(0, len(free))], free[rng.integers(0, len(free))]
    n = 600
    grids.select(0)
    b = _ffi.Batch(gpu_ctx, 2, n, logs=True)
    keepalive = []
    for q in range(2):
        samples = hostprep.draw_free_samples(rng, np.argwhere(og[0] == 0), n)
        qu, keep = _ffi.make_query(1, n, xs, xg, samples, r2_rewire=tm.R2)
        keepalive.append(keep)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    r0 = b.get_result(0)
    more = hostprep.draw_free_samples(rng, np.argwhere(og[0] == 0), min(50, n - r0.j))
    assert len(more) >= 10
    ids, sp, sc, spar = growref.seed(*tree_of(r0))
    want = growref.grow(og[0], 1, n, xg, tm.R2, sp, sc, spar, more)
    goals = free[rng.integers(0, len(free), size=16)]
    assert b.keep_tree(1).all()
    j0, old_id, log0 = b.grow(0, more)
    ans1 = b.routes(1, goals)
    grids.select(1)
    _refused_arg(b.launch, "seeded")
    _refused_arg(lambda: b.connect_goals(1, goals), "replaced")
    grids.select(0)
    _same_goals(b.connect_goals(1, goals), ans1[:2])  # (after a launch query 1 would be refused: it lost its view)
    xy, ids1 = b.routes_rows(len(ans1[5]))
    assert np.array_equal(xy, ans1[4]) and np.array_equal(ids1, ans1[5])
    b.launch()
    b.sync()
    res = b.get_result(0)
    _same_tree(res, _grown(n, want, j0))
    assert res.j > r0.j and b.team_info()["timeouts"] == 0
    _refused_arg(lambda: b.connect_goals(1, goals), "replaced")  # the launch that ran dropped the view
    b.close()
