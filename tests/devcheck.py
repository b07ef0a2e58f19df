"""Oracle-versus-device drivers that more than one test module (and tools/fuzz_more.py) uses: the table of launch shapes of the
straight-line kernels, one query through rrt_plan on a named shape against oracle.plan, and the properties of a rewired tree.

Asserts here are not rewritten by pytest: an exact comparison of arrays names the first indices that differ (orchelp.differ)."""
import numpy as np

import oracle
from orchelp import differ
from rrtplanner_amd import _ffi, hostprep

# teams of up to 64 workers per query (default: pipelined, one more CU that only commits), the same without the pipeline, capped
# teams (2, 3 and 4 workers: 16 samples per member, pipelined and -- 4 -- not; 16: 4 samples per member, 4 waves per sample), one CU,
# one sample per iteration, and a team that loses a member (must finish on one CU per query).
# For a single RRTStandard / RRT* query, which is what every test of this table runs: "team" (no cap) is the committer + worker pair
# of 64 in TWO SHIFTS, 128 workers (treecalls.TWO_SHIFTS); "team64" (the cap of 64) is the same pair in ONE SHIFT, 64 workers
# (treecalls.ONE_SHIFT), which is also what every batch of 2 or 3 queries and every second batch in flight runs.  An Informed query
# runs the one-body kernel on 64 + 1 under both names.
KERNELS = ["team", "team64", "teamnp", "team2", "team3", "team4", "team4np", "team16", "block", "block16", "serial", "teamfault"]
KERNEL_ARGS = {"team": {}, "team64": {"team": 64}, "teamnp": {"pipe": False}, "team2": {"team": 2}, "team3": {"team": 3}, "team4": {"team": 4},
               "team4np": {"team": 4, "pipe": False}, "team16": {"team": 16},
               # one CU per query: the barrier-free pipeline (rrt_pipe.h; Informed queries run the block kernel), and the block kernel
               "block": {"team": 1}, "block16": {"team": 1, "pipe1": False},
               "serial": {"serial": True}, "teamfault": {"team": 8, "team_fault": True}}
KERNELS_NOFAULT = [k for k in KERNELS if k != "teamfault"]


def same_as_oracle_with_logs(rc, res, st, ro):
    """every array, per-iteration log and sum of a result against the oracle's run of the same streams"""
    assert rc == st
    assert res.j == ro.j and res.found == ro.found and res.vgoal == ro.vgoal and res.i_switch == ro.i_switch
    live = ro.j + (1 if ro.found else 0)
    assert np.array_equal(res.nearest_log, ro.nearest_log), differ(res.nearest_log, ro.nearest_log)
    assert np.array_equal(res.accept_log, ro.accept_log), differ(res.accept_log, ro.accept_log)
    assert np.array_equal(res.j_log, ro.jlog), differ(res.j_log, ro.jlog)
    assert np.array_equal(res.pts[:live], ro.pts[:live]), differ(res.pts[:live], ro.pts[:live])
    assert np.array_equal(res.parent[:live], ro.parent[:live]), differ(res.parent[:live], ro.parent[:live])
    assert np.array_equal(res.vcost[:live], ro.vcost[:live]), differ(res.vcost[:live], ro.vcost[:live])  # bit-exact f64 (tolerance stated by the north star: 1e-6)
    assert np.array_equal(res.cbest_log, ro.cbest_log, equal_nan=True), differ(res.cbest_log, ro.cbest_log)
    assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near


def oracle_vs_device(ctx, og8, alg, n, seed, xs, xg, r_rewire=None, r_goal=None, kernel="team"):
    rng = np.random.default_rng(seed)
    free = np.argwhere(og8 == 0)
    samples = hostprep.draw_free_samples(rng, free, n)
    r2 = hostprep.radius_threshold(r_rewire) if r_rewire is not None else 0
    gd2 = hostprep.goal_threshold(r_goal) if r_goal is not None else 0
    Cm = hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64)) if alg == 2 else None
    q, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2, goal_d2=gd2, Cmat=Cm)
    rc, res = ctx.plan(q, n, logs=True, **KERNEL_ARGS[kernel])
    st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, r_goal=r_goal or 0.0, Cmat=Cm)
    ub = None
    if rc == _ffi.RRT_NEED_UNITBALL:
        assert st == oracle.ORC_NEED_UNITBALL and res.i_switch == ro.i_switch
        ub = hostprep.draw_unitball(rng, n - res.i_switch)
        rc = ctx.plan_resume(ub, res)
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, r_goal=r_goal, unitball=ub, ub_offset=res.i_switch, Cmat=Cm)
    same_as_oracle_with_logs(rc, res, st, ro)
    return res, ro


def oracle_vs_batch(ctx, og8, alg, n, seed, xs, xg, r_rewire=None, r_goal=None, kernel="team", cache=None):
    """oracle_vs_device through a Batch of one query, which can say what ran: the same draws, the same comparisons (every log and
    sum), an Informed query through the unit-ball hand-over.  Returns (result, oracle's run, kernel_name(), team_info() with team()
    under "team") of the last launch.  cache: a dict that keeps the oracle's runs for a second call with the same query on another shape."""
    cache = {} if cache is None else cache
    rng = np.random.default_rng(seed)
    free = np.argwhere(og8 == 0)
    samples = hostprep.draw_free_samples(rng, free, n)
    r2 = hostprep.radius_threshold(r_rewire) if r_rewire is not None else 0
    gd2 = hostprep.goal_threshold(r_goal) if r_goal is not None else 0
    Cm = hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64)) if alg == 2 else None
    q, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2, goal_d2=gd2, Cmat=Cm)
    b = _ffi.Batch(ctx, 1, n, logs=True, **KERNEL_ARGS[kernel])
    try:
        b.set_query(0, q)
        b.launch()
        b.sync()
        res = b.get_result(0)
        rc = res.status
        if "first" not in cache:
            cache["first"] = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, r_goal=r_goal or 0.0, Cmat=Cm)
        st, ro = cache["first"]
        if rc == _ffi.RRT_NEED_UNITBALL:
            assert st == oracle.ORC_NEED_UNITBALL and res.i_switch == ro.i_switch
            ub = hostprep.draw_unitball(rng, n - res.i_switch)
            b.set_unitball(0, ub, res.i_switch)
            b.launch()
            b.sync()
            res = b.get_result(0)
            rc = res.status
            if "resumed" not in cache:
                cache["resumed"] = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2, r_goal=r_goal, unitball=ub, ub_offset=ro.i_switch, Cmat=Cm)
            st, ro = cache["resumed"]
        same_as_oracle_with_logs(rc, res, st, ro)
        return res, ro, b.kernel_name(), dict(b.team_info(), team=b.team())
    finally:
        b.close()
        del keep


def check_rewired_tree(og8, r, xs):
    """Every property a rewired tree must have: rooted and acyclic, costs exactly parent cost + edge length, every edge free
    in the direction the rewire / choose-parent tested it (child-side endpoint last), costs non-decreasing along root paths."""
    live = r.j + (1 if r.found else 0)
    par = r.parent[:live].astype(np.int64)
    pts = r.pts[:live].astype(np.int64)
    assert par[0] == -1 and np.all(par[1:] >= 0) and np.all(par[1:] < r.j) and pts[0].tolist() == [int(xs[0]), int(xs[1])]
    depth = np.zeros(live, dtype=np.int64)
    order = np.argsort(r.vcost[:live], kind="stable")
    hops = np.full(live, -1)
    hops[0] = 0
    for _ in range(live):  # relax until every vertex has its hop count: terminates iff the parent map is a tree
        todo = hops < 0
        if not todo.any():
            break
        ok = todo & (hops[np.where(par >= 0, par, 0)] >= 0)
        assert ok.any(), "cycle or orphan in the parent map"
        hops[ok] = hops[par[ok]] + 1
    d = pts[1:] - pts[par[1:]]
    dist = np.sqrt((d * d).sum(1).astype(np.float64))
    assert np.array_equal(r.vcost[1:live], r.vcost[par[1:]] + dist), "a cost is not its parent's cost + the edge length"
    assert np.all(r.vcost[1:live] >= r.vcost[par[1:]])
    for c in range(1, live, max(1, live // 400)):
        assert oracle.collisionfree(og8, pts[par[c]], pts[c])[0] or oracle.collisionfree(og8, pts[c], pts[par[c]])[0]
    del depth, order
