"""The near-set record stream past its first 64 cells, kernels on the other kernel's cell size, and batches of more than one
query on the one-CU kernels.

tests/slabs.py says which iterations of a query make the stream of the ball's cells take a second slab of 64 cells
(r_rewire = 60, 120, 127.5, 255 on divisor 2 cells; every radius from 64 on where a divisor 2 kernel runs on divisor 4 cells).
CPU: the oracle's runs of every case below reach what the case claims, against a floor stated in slabs.meets_floor.
GPU: every kernel against the oracle, every array and per-iteration log bit for bit.

That these tests can fail was checked once with a library whose slab loop stopped after the first 64 cells (`cbase < 64` in
rrt_block_nearset.inc): all six `test_slab_radii_on_every_kernel[*-block16]` cases failed (parents, nearest logs or tree sizes
off the oracle's) while `test_device_vs_oracle_1024_n6000[*-64-*-block16]` of tests/test_gpu_parity.py still passed."""
import numpy as np
import pytest

import oracle
import slabs
from devcheck import KERNEL_ARGS, KERNELS_NOFAULT, check_rewired_tree
from posecalls import assert_audit_clean, check_dubins_tree, device_vs_oracle_dubins, independent_collision_witness
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import random_connected_pair
from slabs import fill_batch, hand_over_unitballs, query_of, same_as_oracle
from treecalls import ONE_SHIFT, TWO_SHIFTS


def _id(c):
    return c["id"]


# ------------------------------------------------------------------------------------------------------------ CPU
def test_geometry_pins():
    """Every r_rewire the older GPU tests pass to the team and block kernels stays within one slab of 64 cells on divisor 2
    cells; 60, 120, 127 and 255 give boxes of 81.  Should RRT_CELL_DIV change, this says that the slab cases need re-aiming."""
    assert (slabs.DIV_TEAM, slabs.DIV_PIPE, slabs.SLAB) == (2.0, 4.0, 64)
    table = {}
    for grid, r in slabs.OLD_RADII + slabs.LATE_RADII:
        r2 = hostprep.radius_threshold(r)
        shift = slabs.cell_shift(grid, grid, r2, slabs.DIV_TEAM)
        table[(grid, r)] = (shift, slabs.largest_box(grid, grid, r2, shift))
    print(table)
    assert table[(2048, 200.5)] == (6, 64) and table[(1024, 48)] == (4, 49) and table[(300, 70)] == (5, 36)
    assert table[(512, 40)] == (4, 36) and table[(1024, 64)] == table[(2048, 64)] == (5, 25)
    assert table[(512, 30)] == table[(96, 30)] == (4, 25)
    assert all(table[k][1] <= slabs.SLAB for k in slabs.OLD_RADII)
    assert [table[k] for k in slabs.LATE_RADII] == [(4, 81), (5, 81), (5, 81), (6, 81)]
    # the other radii of the older tests: one cell, or a grid of at most 25 cells
    for grid, r in ((256, 1e6), (69, 500), (64, 9), (1024, 24), (300, 20), (300, 200)):
        r2 = hostprep.radius_threshold(r)
        assert slabs.largest_box(grid, grid, r2, slabs.cell_shift(grid, grid, r2, slabs.DIV_TEAM)) <= slabs.SLAB
    # the two divisors give different cells from r = 64 on (below, and on 2048^2 at r = 64, they do not)
    assert slabs.shift_pair(1024, 1024, hostprep.radius_threshold(24)) == (4, 4)
    assert slabs.shift_pair(2048, 2048, hostprep.radius_threshold(64)) == (5, 5)
    assert slabs.shift_pair(1024, 1024, hostprep.radius_threshold(64)) == (5, 4)
    assert slabs.shift_pair(300, 260, hostprep.radius_threshold(70)) == (5, 4)
    # a box, by hand: r = 60 around (500, 20) on 1024^2, 16-pixel cells: columns 27 .. 34, rows 0 .. 4 (clamped at y = 0)
    assert [int(v) for v in slabs.box_cells(1024, 1024, 3600, 4, 500, 20)] == [27, 34, 0, 4]


@pytest.mark.parametrize("c", slabs.SLAB_CASES, ids=_id)
def test_slab_cases_reach_a_later_slab(c):
    d = slabs.slab_case(c)
    print(f"{c['id']}: j={d['ro'].j} shift={d['shift']} shifts(div 2, div 4)={slabs.shift_pair(c['W'], c['H'], d['r2'])} {d['cov']}")
    assert d["st"] == 0 and d["cov"]["max_box"] > slabs.SLAB
    assert slabs.meets_floor(d["cov"]), d["cov"]
    if c["alg"] == 2:
        assert d["ub"] is not None and d["ro"].i_switch < c["n"]  # the ellipse phase was reached


@pytest.mark.parametrize("c", slabs.DUBINS_SLAB_CASES, ids=_id)
def test_dubins_slab_cases_reach_a_later_slab(c):
    d = slabs.dubins_slab_case(c)
    print(f"{c['id']}: j={d['ro'].j} shift={d['shift']} {d['cov']}")
    assert d["cov"]["max_box"] > slabs.SLAB and slabs.meets_floor(d["cov"]), d["cov"]


def _xgeo(name, div):
    X = getattr(slabs, name)
    return X, slabs.batch_queries(name, X["W"], X["H"], X["gseed"], X["specs"], X["pair"], div)


@pytest.mark.parametrize("name,div", [("XGEO_A", slabs.DIV_PIPE), ("XGEO_B", slabs.DIV_PIPE), ("XGEO_C", slabs.DIV_TEAM)])
def test_cross_geometry_cases_differ_and_reach_a_later_slab(name, div):
    """Every RRT* query of a cross-geometry batch has different cells under the two divisors, and every one whose box can
    exceed a slab on the cells it runs on meets the floor."""
    X, (og8, qs) = _xgeo(name, div)
    checked = 0
    for k, d in enumerate(qs):
        if d["alg"] == 0:
            continue
        assert d["shifts"][0] != d["shifts"][1], (k, d["shifts"])
        if d["cov"] is not None:
            print(f"{name} query {k}: r={d['rr']} shifts={d['shifts']} j={d['ro'].j} {d['cov']}")
            assert slabs.meets_floor(d["cov"]), (k, d["cov"])
            checked += 1
    assert checked >= 2


# ------------------------------------------------------------------------------------------------------------ GPU
_GROUP1 = {"onebody": {"onebody": True}, "onebody8": {"team": 8, "onebody": True}}


def _kernel_args(kernel):
    return _GROUP1.get(kernel) or KERNEL_ARGS[kernel]


def _group1_kernels():
    return KERNELS_NOFAULT + list(_GROUP1)


def _run_slab_case(ctx, c, kernel):
    """One query on a batch of its own (the kernel's name is the batch's to tell); an Informed one through the unit-ball hand-over."""
    d = slabs.slab_case(c)
    ctx.set_grid(d["og8"])
    b = _ffi.Batch(ctx, 1, c["n"], logs=True, **_kernel_args(kernel))
    qu, keep = query_of(c["alg"], c["n"], d["xs"], d["xg"], d["samples"], d["r2"], c["rg"])
    b.set_query(0, qu)
    b.launch()
    b.sync()
    name = b.kernel_name()
    hand_over_unitballs(b, [d], (c["id"], kernel))
    same_as_oracle(b.get_result(0), d["st"], d["ro"], (c["id"], kernel))
    info = b.team_info()
    b.close()
    return name, info


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", _group1_kernels())
@pytest.mark.parametrize("c", slabs.SLAB_CASES, ids=_id)
def test_slab_radii_on_every_kernel(gpu_ctx, c, kernel):
    name, info = _run_slab_case(gpu_ctx, c, kernel)
    inf = "true" if c["alg"] == 2 else "false"
    if kernel == "team":  # one query without a cap: committer and workers as two kernels in two shifts (an Informed one keeps the one-body kernel)
        assert name == (TWO_SHIFTS if c["alg"] != 2 else "rrt_expand_block_kernel<64, 1, true, true>"), name
        assert info["created"] == info["last"] == (128 if c["alg"] != 2 else 64), info
    elif kernel == "team64":  # the cap of 64: the same pair in one shift
        assert name == (ONE_SHIFT if c["alg"] != 2 else "rrt_expand_block_kernel<64, 1, true, true>"), name
        assert info["created"] == 64 and info["last"] == 64, info
    elif kernel == "onebody":
        assert name == f"rrt_expand_block_kernel<64, 1, true, {inf}>", name
    elif kernel == "onebody8":
        assert name == f"rrt_expand_block_kernel<8, 8, true, {inf}>", name
    elif kernel == "team2":  # the wide team of two (32 samples per member); not built for Informed queries
        assert name == ("rrt_expand_block_kernel<2, 32, true, false>" if c["alg"] != 2 else "rrt_expand_block_kernel<2, 16, true, true>"), name
    elif kernel == "block":
        assert name == ("rrt_pipe_kernel" if c["alg"] != 2 else "rrt_expand_block_kernel<1, 16, false, true>"), name
    elif kernel == "block16":
        assert name == f"rrt_expand_block_kernel<1, 16, false, {inf}>", name
    if kernel != "serial":
        assert info["timeouts"] == 0, info


@pytest.mark.gpu
def test_slab_radius_on_a_team_that_loses_a_member(gpu_ctx):
    """r_rewire = 120 on a team of 8 whose member 1 leaves at once: the batch goes on with one CU per query from the block
    boundary where the hand-off timed out."""
    c = slabs.SLAB_CASES[1]
    name, info = _run_slab_case(gpu_ctx, c, "teamfault")
    assert info["timeouts"] >= 1, info


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("c", slabs.DUBINS_SLAB_CASES, ids=_id)
def test_dubins_near_sets_past_64_cells(gpu_ctx, c, serial):
    d = slabs.dubins_slab_case(c)
    gpu_ctx.set_grid(d["og8"])
    res, ro = device_vs_oracle_dubins(gpu_ctx, d["og8"], 1, c["n"], d["xs"], d["xg"], d["samples"], d["heads"], c["rr"], c["rho"], serial=serial)
    check_dubins_tree(d["og8"], res, c["rho"], 64, d["xs"])
    if not serial:
        independent_collision_witness(d["og8"], res, d["samples"], d["heads"], c["rho"], 64)
    a = oracle.dubins_audit(d["og8"], c["n"], 1, d["samples"], d["heads"], res.pts, res.head, res.vcost, res.parent, res.j, r2_rewire=d["r2"],
                            rho=c["rho"], nh=64)
    assert a["n_accepted"] == res.j - 1
    assert_audit_clean(a, 1)


# ---- cross-geometry launches -----------------------------------------------------------------------------------------
def _resume_informed(b, og8, qs):
    """The Informed queries of a launched batch: hand each its unit-ball stream, launch again, compare with the oracle's run
    on the same stream (as test_pipelined_informed_batch_has_no_timeouts does).  Returns how many were resumed."""
    waiting = {}
    for q, d in enumerate(qs):
        if d["alg"] != 2:
            continue
        r = b.get_result(q, arrays=False)
        if r.c.status == _ffi.RRT_NEED_UNITBALL:
            rng = np.random.default_rng()
            rng.bit_generator.state = d["rng"].bit_generator.state  # the generator right after the free draws
            waiting[q] = (hostprep.draw_unitball(rng, d["n"] - r.c.i_switch), r.c.i_switch)
            b.set_unitball(q, *waiting[q])
    if waiting:
        b.launch()
        b.sync()
    for q, d in enumerate(qs):
        if d["alg"] != 2:
            continue
        kw = dict(unitball=waiting[q][0], ub_offset=waiting[q][1]) if q in waiting else {}
        Cm = hostprep.rotation_to_world_frame(np.asarray(d["xs"], dtype=np.int64), np.asarray(d["xg"], dtype=np.int64))
        st, ro = oracle.plan(og8, d["n"], 2, d["xs"], d["xg"], d["samples"], r2_rewire=d["r2"], r_goal=d["rg"], Cmat=Cm, **kw)
        same_as_oracle(b.get_result(q), st, ro, f"Informed query {q}")
    return len(waiting)


@pytest.mark.gpu
def test_block_kernel_on_the_pipelines_cells(gpu_ctx):
    """One CU per query and an Informed query among them: every query runs rrt_expand_block_kernel<1, 16, false, true>, the RRT*
    ones on the divisor 4 cells they were set with (boxes of 81, 196 and 289 cells: up to five slabs)."""
    X, (og8, qs) = _xgeo("XGEO_A", slabs.DIV_PIPE)
    gpu_ctx.set_grid(og8)
    b = _ffi.Batch(gpu_ctx, len(qs), X["n"], logs=True, team=1)
    keep = fill_batch(b, qs)
    b.launch()
    b.sync()
    assert b.kernel_name() == "rrt_expand_block_kernel<1, 16, false, true>" and b.team_info()["last"] == 1
    for q, d in enumerate(qs):
        if d["alg"] != 2:
            same_as_oracle(b.get_result(q), d["st"], d["ro"], f"query {q}")
    assert _resume_informed(b, og8, qs) >= 1
    assert b.kernel_name() == "rrt_expand_block_kernel<1, 16, false, true>"
    for q, d in enumerate(qs):  # the finished queries are untouched by the second launch
        if d["alg"] != 2:
            same_as_oracle(b.get_result(q), d["st"], d["ro"], f"query {q} after the resume")
    b.close()
    del keep


@pytest.mark.gpu
def test_team_of_two_on_the_pipelines_cells(gpu_ctx):
    """100 queries, one of them Informed: two CUs per query without a committer, the RRT* queries on divisor 4 cells
    (r_rewire = 70 and 100: boxes of 100 and 196 cells)."""
    X, (og8, qs) = _xgeo("XGEO_B", slabs.DIV_PIPE)
    gpu_ctx.set_grid(og8)
    b = _ffi.Batch(gpu_ctx, len(qs), X["n"], logs=True)
    keep = fill_batch(b, qs)
    b.launch()
    b.sync()
    assert b.kernel_name() == "rrt_expand_block_kernel<2, 16, false, true>", b.kernel_name()
    info = b.team_info()
    assert info["last"] == 2 and info["timeouts"] == 0, info
    for q, d in enumerate(qs):
        if d["alg"] != 2:
            same_as_oracle(b.get_result(q), d["st"], d["ro"], f"query {q}")
    _resume_informed(b, og8, qs)
    assert b.team_info()["timeouts"] == 0
    b.close()
    del keep


@pytest.mark.gpu
def test_pipeline_on_the_teams_cells(gpu_ctx):
    """A default-team batch launched while a batch of 512 one-CU queries holds every compute unit of the registry (its claim
    lasts until it is synchronised): the registry shrinks the teams to one CU per query and the launch runs rrt_pipe_kernel on
    the divisor 2 cells the queries were set with.  Nothing depends on timing, only on the order of launch and sync.  Alone
    again, the batch gets its team back, and the trees are the same."""
    X, (og8, qs) = _xgeo("XGEO_C", slabs.DIV_TEAM)
    gpu_ctx.set_grid(og8)
    free = np.argwhere(og8 == 0)
    Qh, nh = 512, 64  # (min(Q, CUs) are claimed: every CU of a device of up to 512)
    hold = _ffi.Batch(gpu_ctx, Qh, nh, team=1)
    hs = hostprep.draw_free_samples(np.random.default_rng(900), free, nh)
    hq, hkeep = _ffi.make_query(0, nh, qs[0]["xs"], qs[0]["xg"], hs)
    for q in range(Qh):
        hold.set_query(q, hq)
    b = _ffi.Batch(gpu_ctx, len(qs), X["n"], logs=True)
    keep = fill_batch(b, qs)
    created = b.team_info()["created"]
    assert created > 1 and b.team_info()["shrunk"] == 0
    hold.launch()
    b.launch()
    hold.sync()
    b.sync()
    info = b.team_info()
    assert b.kernel_name() == "rrt_pipe_kernel" and info["last"] == 1 and info["shrunk"] == 1 and info["timeouts"] == 0, (b.kernel_name(), info)
    for q, d in enumerate(qs):
        same_as_oracle(b.get_result(q), d["st"], d["ro"], f"query {q} on the pipeline")
    st, ro = oracle.plan(og8, nh, 0, qs[0]["xs"], qs[0]["xg"], hs)
    for q in (0, Qh - 1):
        r = hold.get_result(q)
        assert r.status == st and r.j == ro.j and np.array_equal(r.parent[:ro.j], ro.parent[:ro.j])
    hold.close()
    b.rearm()
    b.launch()
    b.sync()
    info = b.team_info()
    assert info == dict(created=created, last=created, timeouts=0, shrunk=1) and b.kernel_name() != "rrt_pipe_kernel", (b.kernel_name(), info)
    for q, d in enumerate(qs):
        same_as_oracle(b.get_result(q), d["st"], d["ro"], f"query {q} on the team")
    b.close()
    del keep, hkeep


# ---- more than one query on the one-CU kernels -----------------------------------------------------------------------------
_MULTI_N = [3000, 1, 1001, 2500, 3000]  # the capacity twice, 1, and one that is no multiple of 64
_MULTI_R = [40, 64, 24, 100, 30]


def _multi_straight(og, og8, rewire, informed_at):
    free = np.argwhere(og8 == 0)
    sg = np.random.default_rng(17)
    qs = []
    for q, n in enumerate(_MULTI_N):
        xs, xg = random_connected_pair(og, sg)
        rng = np.random.default_rng(400 + q)
        samples = hostprep.draw_free_samples(rng, free, n)
        alg = 2 if q == informed_at else 1
        rg = 10 if alg == 2 else None
        r2 = hostprep.radius_threshold(_MULTI_R[q])
        Cm = hostprep.rotation_to_world_frame(np.asarray(xs, dtype=np.int64), np.asarray(xg, dtype=np.int64)) if alg == 2 else None
        kw = dict(r2_rewire=r2, r_goal=rg or 0.0, Cmat=Cm, rewire=rewire)
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, **kw)
        ub = None
        if st == oracle.ORC_NEED_UNITBALL:
            ub = hostprep.draw_unitball(rng, n - ro.i_switch)
            st, ro = oracle.plan(og8, n, alg, xs, xg, samples, unitball=ub, ub_offset=ro.i_switch, **kw)
        qs.append(dict(alg=alg, n=n, xs=xs, xg=xg, samples=samples, r2=r2, rg=rg, st=st, ro=ro, ub=ub))
    return qs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["rewire", "serial"])
def test_five_queries_on_the_one_sample_kernels(gpu_ctx, mode):
    """rrt_expand_kernel<true, false> (the opt-in rewire) and <false, false> (RRT_FLAG_SERIAL) with query offsets above 0: five
    queries of different n, start, goal and radius (the rewire batch with an Informed one, resumed), logs on, launched twice
    with a rearm between (which must reset the rewire's child lists and frontier)."""
    og, og8 = slabs.grid_of(512, 512, 2)
    gpu_ctx.set_grid(og8)
    rewire = mode == "rewire"
    qs = _multi_straight(og, og8, rewire, informed_at=3 if rewire else -1)
    if rewire:
        assert qs[3]["ub"] is not None and sum(d["ro"].n_rewired > 0 for d in qs) >= 3
    b = _ffi.Batch(gpu_ctx, len(qs), max(_MULTI_N), logs=True, rewire=rewire, serial=not rewire)
    keep = fill_batch(b, qs)
    for rep in range(2):
        b.launch()
        b.sync()
        assert b.kernel_name() == f"rrt_expand_kernel<{'true' if rewire else 'false'}, false>"
        for q, d in enumerate(qs):
            if d["ub"] is not None:
                r = b.get_result(q, arrays=False)
                assert r.c.status == _ffi.RRT_NEED_UNITBALL and r.c.i_switch == d["ro"].i_switch, (rep, q)
                b.set_unitball(q, d["ub"], r.c.i_switch)
                b.launch()
                b.sync()
        for q, d in enumerate(qs):
            res = b.get_result(q)
            same_as_oracle(res, d["st"], d["ro"], (mode, rep, q), rewire=rewire)
            assert (res.n_rewired, res.n_propagated) == (d["ro"].n_rewired, d["ro"].n_propagated), (mode, rep, q)
        b.rearm()
    b.close()
    del keep


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [True, False])
def test_five_dubins_queries_with_logs(gpu_ctx, serial):
    """The Dubins kernels (one sample per iteration, and the default 16 per round) with query offsets above 0: different n, pose,
    radius, rho and number of headings per query, logs on, two launches with a rearm between."""
    og, og8 = slabs.grid_of(512, 512, 2)
    gpu_ctx.set_grid(og8)
    free = np.argwhere(og8 == 0)
    sg = np.random.default_rng(19)
    rhos, nhs = [5.0, 3.0, 8.0, 6.5, 4.0], [64, 8, 32, 256, 64]
    b = _ffi.Batch(gpu_ctx, 5, max(_MULTI_N), logs=True, dubins=True, serial=serial)
    keep, refs = [], []
    for q, n in enumerate(_MULTI_N):
        a, c = random_connected_pair(og, sg)
        nh = nhs[q]
        xs, xg = (int(a[0]), int(a[1]), q % nh), (int(c[0]), int(c[1]), (3 * q + 1) % nh)
        rng = np.random.default_rng(600 + q)
        s = hostprep.draw_free_samples(rng, free, n)
        hd = rng.integers(0, nh, size=n)
        star = q % 2 == 0
        r2 = hostprep.radius_threshold(_MULTI_R[q]) if star else 0
        qu, k = _ffi.make_query(_ffi.ALG_DUBINS_STAR if star else _ffi.ALG_DUBINS, n, xs, xg, s, r2_rewire=r2, headings=hd, rho=rhos[q], nh=nh)
        keep.append(k)
        b.set_query(q, qu)
        refs.append(oracle.dubins_plan(og8, n, star, xs, xg, s, hd, r2_rewire=r2, rho=rhos[q], nh=nh))
    for rep in range(2):
        b.launch()
        b.sync()
        assert b.kernel_name() == ("rrt_expand_kernel<false, true>" if serial else "rrt_dubins_block_kernel")
        for q, (st, ro) in enumerate(refs):
            res = b.get_result(q)
            live = ro.j + (1 if ro.found else 0)
            tag = (serial, rep, q)
            assert res.status == st and (res.j, res.found, res.vgoal) == (ro.j, ro.found, ro.vgoal), tag
            assert np.array_equal(res.nearest_log, ro.nearest_log) and np.array_equal(res.accept_log, ro.accept_log), tag
            assert np.array_equal(res.pts[:live], ro.pts[:live]) and np.array_equal(res.head[:live], ro.head[:live]), tag
            assert np.array_equal(res.parent[:live], ro.parent[:live]) and np.array_equal(res.vcost[:live], ro.vcost[:live]), tag
            assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near, tag
        b.rearm()
    b.close()
    del keep


@pytest.mark.gpu
def test_rewire_batch_of_more_queries_than_compute_units(gpu_ctx):
    """300 rewire queries of n = 300: more workgroups than the device has CUs, every per-query stride of the child lists and the
    frontier in use."""
    og, og8 = slabs.grid_of(300, 260, 5)
    gpu_ctx.set_grid(og8)
    free = np.argwhere(og8 == 0)
    sg = np.random.default_rng(23)
    Q, n = 300, 300
    b = _ffi.Batch(gpu_ctx, Q, n, logs=True, rewire=True)
    keep, refs = [], []
    for q in range(Q):
        xs, xg = random_connected_pair(og, sg)
        samples = hostprep.draw_free_samples(np.random.default_rng(3000 + q), free, n)
        r2 = hostprep.radius_threshold(30 if q % 3 else 70)
        qu, k = _ffi.make_query(1, n, xs, xg, samples, r2_rewire=r2)
        keep.append(k)
        b.set_query(q, qu)
        refs.append((xs,) + oracle.plan(og8, n, 1, xs, xg, samples, r2_rewire=r2, rewire=True))
    assert sum(ro.n_rewired > 0 for _, _, ro in refs) > Q // 2
    b.launch()
    b.sync()
    assert b.kernel_name() == "rrt_expand_kernel<true, false>"
    for q, (xs, st, ro) in enumerate(refs):
        res = b.get_result(q)
        same_as_oracle(res, st, ro, f"query {q}", rewire=True)
        if q in (0, 1, 150, 299):
            check_rewired_tree(og8, res, xs)
    b.close()
    del keep
