"""Every team kernel of rrt_block_variants.def against the oracle.

tests/variants.py reads the table from the file that defines it and says, row by row, which `Batch` reaches the row.
CPU: every row has such a recipe and a name, the table and the Makefile name the same units, and every (team, pipelined,
Informed, wide, as two kernels) that `plan_launch` can form is a row (a missing one is RRT_E_UNSUPPORTED "no team kernel
for ..." at launch time, possibly only when another launch holds compute units).  GPU: one test per row; the row's kernel
must be the one that ran, and every array and per-iteration log must equal the oracle's, twice (rearm between).

Workloads (inputs of tests/test_gpu_parity.py, so nothing new on the oracle's side):
  A  1024^2 perlin(seed=1), pair default_rng(7), samples seed 0, n = 40 000, r_rewire 64, RRTStandard and RRT*: the node scan
     crosses from LDS chunks into HBM chunks (test_device_vs_oracle_beyond_lds_capacity)
  B  the same grid and pair, n = 25 000, r_rewire 64, r_goal 12, Informed: the ellipse moves after the switch, a pipelined
     team voids and restarts blocks (test_device_vs_oracle_informed_1024_n25000)
  C  64^2 perlin(seed=1), pair default_rng(1), samples seed 1, n = 3000, r_rewire 9, RRT*: r2 = 81 is below a cell (the
     brute-force near scan; what selects the team of two with 16 samples per member), most samples interact inside a block
  E  256^2 perlin(seed=4), pair default_rng(1), samples seed 3, n = 5000, r_rewire 10^6, RRT*: the near set is the whole tree
     and overflows the LDS lists (test_device_vs_oracle_near_set_spills)
A row without Informed queries runs A (each algorithm), C and E, one query per batch, as far as its recipe's radius rule admits
the batch; an Informed row runs {B, A as RRT* cut to n = 25 000} and {B, A as RRTStandard cut alike}: two queries still get
64 + 1 compute units each on 256.  Every oracle run is made once per process (`_query`)."""
import itertools

import numpy as np
import pytest

import slabs
import variants
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import random_connected_pair

WORKLOADS = {
    "A": dict(grid=1024, gseed=1, pair=7, seed=0, n=40000, rr=64, rg=None),
    "B": dict(grid=1024, gseed=1, pair=7, seed=0, n=25000, rr=64, rg=12),
    "C": dict(grid=64, gseed=1, pair=1, seed=1, n=3000, rr=9, rg=None),
    "E": dict(grid=256, gseed=4, pair=1, seed=3, n=5000, rr=1e6, rg=None),
}
# batches as lists of (workload, alg, n); alg 0 = RRTStandard, 1 = RRT*, 2 = Informed RRT*
PLAIN_BATCHES = [[("A", 0, 40000)], [("A", 1, 40000)], [("C", 1, 3000)], [("E", 1, 5000)]]
INFORMED_BATCHES = [[("B", 2, 25000), ("A", 1, 25000)], [("B", 2, 25000), ("A", 0, 25000)]]
A_MIN_J = 36000  # the full-length runs of A must grow a tree of more than this (far more than fits the LDS node cache)

_drawn, _queries = {}, {}


def _workload(tag):
    """(og8, xs, xg, samples, generator right behind the draws) of a workload"""
    if tag not in _drawn:
        w = WORKLOADS[tag]
        og, og8 = slabs.grid_of(w["grid"], w["grid"], w["gseed"])
        xs, xg = random_connected_pair(og, np.random.default_rng(w["pair"]))
        rng = np.random.default_rng(w["seed"])
        samples = hostprep.draw_free_samples(rng, np.argwhere(og8 == 0), w["n"])
        _drawn[tag] = (og8, xs, xg, samples, rng)
    return _drawn[tag]


def _query(spec):
    """One query and the oracle's run of it (an Informed one through the unit-ball hand-over), once per process: the dict that
    slabs.fill_batch and slabs.hand_over_unitballs take"""
    if spec not in _queries:
        tag, alg, n = spec
        w = WORKLOADS[tag]
        og8, xs, xg, samples, rng = _workload(tag)
        assert n <= w["n"] and (alg == 2) == (w["rg"] is not None), spec
        if alg == 2:
            assert n == w["n"], spec  # (the unit-ball stream continues the generator behind exactly n draws)
            r = np.random.default_rng()
            r.bit_generator.state = rng.bit_generator.state
            rng = r
        st, ro, r2, ub = slabs.run_query(og8, alg, n, xs, xg, samples[:n], rng, w["rr"] if alg else None, w["rg"])
        _queries[spec] = dict(tag=tag, alg=alg, n=n, xs=xs, xg=xg, samples=samples[:n], r2=r2, rg=w["rg"], st=st, ro=ro, ub=ub, og8=og8)
    return _queries[spec]


def _narrow(batch):
    """plan_launch: `if (d.alg != RRT_ALG_STANDARD && d.r2_rewire < 257u) narrow = true;` over the queries of the launch"""
    return any(alg != 0 and hostprep.radius_threshold(WORKLOADS[tag]["rr"]) < variants.NARROW_R2 for tag, alg, n in batch)


def batches_of(rec):
    """the batches a recipe admits: Informed or not, and launches whose radii bring them to the recipe's row"""
    pool = INFORMED_BATCHES if rec.informed else PLAIN_BATCHES
    return [b for b in pool if rec.radius is None or (rec.radius == "narrow") == _narrow(b)]


def _ellipse_moves(ro):
    """distinct best costs from the switch on (cbest_log: NaN where no iteration ran)"""
    cb = np.asarray(ro.cbest_log)[ro.i_switch:]
    return int(np.unique(cb[~np.isnan(cb)]).size) - 1


def _check_workload(d):
    """what a workload must do for the matrix to mean something, on the oracle's run"""
    ro = d["ro"]
    if d["tag"] == "A" and d["n"] == WORKLOADS["A"]["n"]:
        assert d["st"] == 0 and ro.found and ro.j > A_MIN_J, (d["tag"], d["alg"], ro.j)
    if d["tag"] == "B":
        assert d["ub"] is not None and ro.i_switch < d["n"] and _ellipse_moves(ro) >= 1, (ro.i_switch, _ellipse_moves(ro))


# ------------------------------------------------------------------------------------------------------------ CPU
ROWS = variants.rows()


def test_the_table_as_parsed():
    us = variants.units()
    print(f"{len(us)} units, {len(ROWS)} rows")
    assert len(set(ROWS)) == len(ROWS)
    for listed in ("K(32, 2, true, true)", "K(32, 2, false, true)", "K(16, 4, false, true)", "K(8, 8, false, false)", "K(8, 8, false, true)",
                   "K(2, 32, true, false)", "S(64, 1, false)"):
        kind, a = listed[0], [s.strip() for s in listed[2:-1].split(",")]
        flags = [s == "true" for s in a[2:]]
        assert variants.Row(kind, int(a[0]), int(a[1]), True if kind == "S" else flags[0], flags[-1]) in ROWS, listed


def test_every_row_has_a_recipe_a_name_and_a_batch():
    recipes, names = {}, {}
    for row in ROWS:
        rec = variants.recipe(row)  # LookupError: a row nobody knows how to launch
        key = (tuple(sorted(rec.batch.items())), rec.informed, rec.radius)
        assert key not in recipes, f"{row} and {recipes[key]} are launched the same way: one of them never runs"
        recipes[key] = row
        name = variants.kernel_name(row)
        assert name not in names and len(name) < 128, name  # (rrt_batch_kernel_name's callers pass 128 bytes)
        names[name] = row
        assert len(batches_of(rec)) >= 1, row
        _ffi.kernel_flags(logs=True, **rec.batch)  # the keyword arguments are ones a Batch takes


_TEXT = """// a comment that names K(9, 9, true, true) and U(99)
#define RRT_UNIT_10(K, S) K(64, 1, true, false)  // and S(1, 1, true) here
#define RRT_UNIT_12(K, S) K(4, 16, false, false) K(2, 32, true, false)
#define RRT_UNIT_22(K, S) S(64, 1, false)
#define RRT_BLOCK_UNITS(U) U(10) U(22) U(12)
"""


def test_parser_and_recipes_refuse_what_they_do_not_know():
    R = variants.Row
    assert variants.units(_TEXT) == [10, 22, 12]
    assert variants.rows(_TEXT) == [R("K", 64, 1, True, False), R("S", 64, 1, True, False), R("K", 4, 16, False, False), R("K", 2, 32, True, False)]
    extra = _TEXT.replace("K(4, 16, false, false)", "K(4, 16, false, false) K(3, 16, false, false)")
    assert variants.rows(extra)[3] == R("K", 3, 16, False, False)
    with pytest.raises(LookupError):
        [variants.recipe(r) for r in variants.rows(extra)]
    # wide rows other than the pipelined team of two, committer + worker pairs that split_team never forms, teams pick_team never forms
    for row in (R("K", 2, 32, True, True), R("K", 4, 32, True, False), R("K", 2, 32, False, False), R("S", 4, 16, True, False),
                R("S", 8, 8, True, True), R("S", 2, 32, True, False), R("K", 1, 16, True, False), R("K", 5, 8, True, False), R("K", 128, 1, False, False)):
        with pytest.raises(LookupError):
            variants.recipe(row)
    for bad in (_TEXT.replace(" U(12)", ""), _TEXT.replace("U(12)", "U(12) U(13)"), _TEXT.replace("U(12)", "U(12) U(10)"),
                _TEXT.replace("S(64, 1, false)", "S(64, 1, true, false)"), _TEXT.replace("K(64, 1, true, false)", "K(64, 1, 1, false)"),
                _TEXT.replace("S(64, 1, false)", "S(64, 1, false) T(1)"), _TEXT.replace("RRT_BLOCK_UNITS", "RRT_UNITS")):
        assert bad != _TEXT
        with pytest.raises(ValueError):
            variants.rows(bad)


def test_units_of_the_table_and_of_the_makefile():
    """A new unit is named in RRT_BLOCK_UNITS and in the Makefile's TUS (units 1 to 4 are the other kernels)."""
    us, tus = variants.units(), variants.makefile_units()
    assert len(set(tus)) == len(tus)
    assert set(us) <= set(tus), sorted(set(us) - set(tus))
    assert {k for k in tus if k >= 10} <= set(us), sorted({k for k in tus if k >= 10} - set(us))
    assert all(k >= 10 for k in us)


def _planned(team, pipelined, inf, narrow, onebody):
    """(team, pipe, inf, wide, split) as plan_launch in rrt_engine.hip forms it, restated from these of its lines:
        p.pipe = ts.team > 1 && ts.pipe;
        p.wide = p.pipe && !inf && p.team == 2 && !narrow;
        p.split = split_team(p.team, p.pipe, inf, p.wide, b->flags);
            split_team: return pipe && !inf && !wide && team >= 8 && !(flags & RRT_FLAG_ONEBODY);
        p.row = find_variant(p.team, p.pipe, inf, p.wide, p.split);"""
    pipe = team > 1 and pipelined
    wide = pipe and not inf and team == 2 and not narrow
    split = pipe and not inf and not wide and team >= 8 and not onebody
    return team, pipe, inf, wide, split


def _find_variant(table, team, pipe, inf, wide, split):
    """find_variant: `r.G == team && r.pipe == pipe && r.inf == inf && (r.BSM > 16) == wide && (r.commit != nullptr) == split`,
    the first such row"""
    for r in table:
        if r.G == team and r.pipe == pipe and r.inf == inf and (r.BSM > 16) == wide and (r.kind == "S") == split:
            return r
    return None


def _launch_shapes():
    """every team size pick_team can return (and one CU per query, where RRT_FLAG_NOPIPE1, an Informed query or the
    continuation of a launch that timed out runs the block kernel), with every value of what else plan_launch looks at"""
    for pipelined, teams in ((False, variants.TEAMS_UNPIPELINED), (True, variants.TEAMS_PIPELINED + (1,))):
        for team, inf, narrow, onebody in itertools.product(teams, (False, True), (False, True), (False, True)):
            yield team, pipelined, inf, narrow, onebody


def test_every_launch_plan_ends_on_a_row_of_the_table():
    reached = set()
    for shape in _launch_shapes():
        want = _planned(*shape)
        row = _find_variant(ROWS, *want)
        assert row is not None, f"no team kernel for (team, pipelined, Informed, wide, as two kernels) = {want}"
        reached.add(row)
    assert reached == set(ROWS), sorted(set(ROWS) - reached)  # and no row that no launch plan reaches
    # what the closure test is for: without this row a shrunk Informed launch would fail with RRT_E_UNSUPPORTED
    fewer = [r for r in ROWS if r != variants.Row("K", 8, 8, False, True)]
    assert len(fewer) == len(ROWS) - 1
    assert any(_find_variant(fewer, *_planned(*s)) is None for s in _launch_shapes())


def test_every_recipe_plans_its_own_row():
    """The recipe's keyword arguments, put through the restated launch plan, select the row they were made for."""
    for row in ROWS:
        rec = variants.recipe(row)
        for batch in batches_of(rec):
            inf = any(alg == 2 for _, alg, _ in batch)
            kw = rec.batch
            if kw["team"] == 1:
                assert kw.get("pipe1") is False or inf, row  # (or rrt_pipe_kernel runs)
            got = _find_variant(ROWS, *_planned(kw["team"], kw["pipe"], inf, _narrow(batch), kw.get("onebody", False)))
            assert got == row, (row, batch, got)


def test_workloads_do_what_the_matrix_needs():
    """The oracle's runs: A grows a tree past the LDS node cache and finds the goal, B reaches its ellipse phase and the
    ellipse moves there, C is the only narrow workload."""
    for spec in sorted({s for b in PLAIN_BATCHES + INFORMED_BATCHES for s in b}):
        d = _query(spec)
        print(spec, "status", d["st"], "j", d["ro"].j, "found", d["ro"].found, "i_switch", d["ro"].i_switch,
              "ellipse moves", _ellipse_moves(d["ro"]) if spec[1] == 2 else "-")
        _check_workload(d)
    assert [_narrow(b) for b in PLAIN_BATCHES] == [False, False, True, False] and not any(_narrow(b) for b in INFORMED_BATCHES)
    assert sum(1 for b in PLAIN_BATCHES + INFORMED_BATCHES for s in b if s[0] == "A" and s[2] == WORKLOADS["A"]["n"]) == 2


# ------------------------------------------------------------------------------------------------------------ GPU
def _check_launch(b, row, tag):
    """the launch ran this row's kernel (or the test says nothing about it) on a whole team, and no hand-off timed out"""
    assert b.kernel_name() == variants.kernel_name(row), (tag, b.kernel_name())
    info = b.team_info()
    assert b.team() == (row.G, 0) and info == dict(created=row.G, last=row.G, timeouts=0, shrunk=0), (tag, b.team(), info)
    assert b.pipelined() == row.pipe, tag


def _compare_plain(b, qs, tag):
    for q, d in enumerate(qs):
        if d["alg"] != 2:
            slabs.same_as_oracle(b.get_result(q), d["st"], d["ro"], tag + (q,))


def _run_batch(ctx, row, rec, batch):
    qs = [_query(spec) for spec in batch]
    for d in qs:
        _check_workload(d)
    ctx.set_grid(qs[0]["og8"])
    b = _ffi.Batch(ctx, len(qs), max(d["n"] for d in qs), logs=True, **rec.batch)
    keep = slabs.fill_batch(b, qs)
    for rep in range(2):  # the second time on the same buffers, after a rearm
        tag = (variants.kernel_name(row), tuple(batch), rep)
        b.launch()
        b.sync()
        _check_launch(b, row, tag)
        _compare_plain(b, qs, tag)
        if rec.informed:
            assert slabs.hand_over_unitballs(b, qs, tag) == 1, tag
            _check_launch(b, row, tag + ("resumed",))
            for q, d in enumerate(qs):
                if d["alg"] == 2:
                    slabs.same_as_oracle(b.get_result(q), d["st"], d["ro"], tag + (q,))
            _compare_plain(b, qs, tag + ("untouched by the second launch",))
        b.rearm()
    ms = b.elapsed_ms()
    b.close()
    del keep
    return ms


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=variants.kernel_name)
def test_every_row_against_the_oracle(gpu_ctx, row):
    rec = variants.recipe(row)
    ran = 0
    for batch in batches_of(rec):
        ms = _run_batch(gpu_ctx, row, rec, batch)
        print(f"{variants.kernel_name(row)}: {batch} Batch({rec.batch}) last launch {ms:.2f} ms")
        ran += 1
    assert ran >= 1, row
