"""The nearest-vertex search of the cell-record kernels past its last box, on pocket maps.

rrt_pipe_kernel and the Dubins block kernel find the nearest vertex in the cells of a box around the sample and leave out the
cells farther than the box radius.  A tree confined to a pocket in the far corner of a map, and samples drawn over the whole
map, put the nearest vertex in cells that even the last, map-wide box leaves out (tests/farnn.py says when).  The device must
still return the oracle's `near()[0]`: the nearest vertex, the lowest index among equals.

CPU: the oracle's trees of every case reach that pass (the cases test what they claim to).  GPU: the kernels against the
oracle, every array and per-iteration log bit for bit."""
import numpy as np
import pytest

import farnn
import oracle
from devcheck import KERNELS_NOFAULT, oracle_vs_device
from posecalls import assert_audit_clean, device_vs_oracle_dubins
from rrtplanner_amd import _ffi, hostprep


# ------------------------------------------------------------------------------------------------------------ CPU
def test_terminal_pass_geometry():
    """The restated geometry at the points the cases rely on, and at the bench's grids (1024^2, 2048^2: the last box of
    both searches keeps every cell within the diagonal, so nothing there can reach a culled terminal pass)."""
    assert farnn.cell_shift(63, 63, 0, farnn.DIV_PIPE) == 4 and farnn.first_radius(False, 0, 4) == (31, 1023)
    assert farnn.terminal_pass("pipe", 63, 63, False, 0) == (4, 63, 63 * 63)
    assert farnn.terminal_pass("pipe", 63, 63, True, 4096) == (4, 63, 4095)      # r_rewire = 64: no doubling
    assert farnn.terminal_pass("pipe", 64, 64, False, 0) is None                 # 63 < 64: a miss scans every vertex
    assert farnn.terminal_pass("dubins", 127, 127, False, 0) == (4, 127, 127 * 127)
    assert farnn.terminal_pass("dubins", 127, 127, True, 576) == (4, 127, 127 * 127)
    assert farnn.terminal_pass("pipe", 1024, 1024, True, 4096) is None
    for grid, r2 in ((1024, 0), (1024, 4096), (2048, 0), (2048, 4096)):
        _, _, keep = farnn.terminal_pass("dubins", grid, grid, r2 > 0, r2)
        assert keep >= 2 * (grid - 1) ** 2


@pytest.mark.parametrize("c", farnn.PIPE_CASES, ids=lambda c: c["id"])
def test_pipe_cases_reach_the_terminal_pass(c):
    og8, samples, r2, st, ro, cov = farnn.run_pipe_oracle(c)
    print(f"{c['id']}: j={ro.j} reach={cov['reach']} no-vertex={cov['novertex']} ties={cov['ties']} first={cov['first']}")
    assert st == 0 and ro.j > farnn.TINY
    assert np.all(og8[ro.pts[:ro.j, 0], ro.pts[:ro.j, 1]] == 0)
    assert np.array_equal(ro.jlog, farnn.dubins_jlog(ro))  # the tree-size rule the Dubins check uses
    assert cov["reach"] >= 1
    assert (cov["novertex"] == cov["start_culled"] == 0) if c["parent_safe"] else (cov["novertex"] >= 1)


@pytest.mark.parametrize("c", farnn.DUBINS_CASES, ids=lambda c: c["id"])
def test_dubins_cases_reach_the_terminal_pass(c):
    og8, samples, heads, r2, st, ro, cov = farnn.run_dubins_oracle(c)
    print(f"{c['id']}: status={st} j={ro.j} reach={cov['reach']} no-vertex={cov['novertex']} ties={cov['ties']} first={cov['first']}")
    assert ro.j > farnn.TINY
    assert cov["reach"] >= 1
    assert (cov["novertex"] == cov["start_culled"] == 0) if c["parent_safe"] else (cov["novertex"] >= 1)
    if c.get("ties"):
        assert cov["ties"] >= 1


def test_pipe_pocket_fuzz_reaches_the_terminal_pass():
    """At least half of the pocket fuzz's cases reach the terminal pass; every case has a tree beyond the tiny path."""
    cases = farnn.pipe_fuzz_cases()
    assert len(cases) >= 24
    reached = 0
    for c in cases:
        og8, samples, r2, st, ro, cov = farnn.run_pipe_oracle(c)
        print(f"{c['id']}: {c['W']}x{c['H']} alg={c['alg']} pieces={len(c['rects'])} j={ro.j} reach={cov['reach']} "
              f"no-vertex={cov['novertex']} ties={cov['ties']}")
        assert ro.j > farnn.TINY
        reached += cov["reach"] > 0
    print(f"pipe pocket fuzz: {reached} of {len(cases)} cases reach the terminal pass")
    assert 2 * reached >= len(cases)


def test_dubins_pocket_fuzz_reaches_the_terminal_pass():
    cases = farnn.dubins_fuzz_cases()
    reached = 0
    for c in cases:
        og8, samples, heads, r2, st, ro, cov = farnn.run_dubins_oracle(c)
        print(f"{c['id']}: {c['W']}x{c['H']} star={c['star']} rho={c['rho']} j={ro.j} reach={cov['reach']} no-vertex={cov['novertex']}")
        assert ro.j > farnn.TINY
        reached += cov["reach"] > 0
    print(f"Dubins pocket fuzz: {reached} of {len(cases)} cases reach the terminal pass")
    assert 2 * reached >= len(cases)


# ------------------------------------------------------------------------------------------------------------ GPU
def _pipe_device_vs_oracle(ctx, c, kernel):
    og8 = farnn.pocket_grid(c["W"], c["H"], c["rects"], c.get("field"))
    ctx.set_grid(og8)
    try:
        # (the same draws as farnn.pipe_case: default_rng(seed), hostprep.draw_free_samples over the free cells)
        return oracle_vs_device(ctx, og8, c["alg"], c["n"], c["seed"], c["xs"], c["xg"], c["rr"], None, kernel=kernel)
    except AssertionError as e:
        raise AssertionError(f"pocket case {c['id']} ({c['W']}x{c['H']} alg {c['alg']} r {c['rr']}) on {kernel}") from e


def _batch_vs_oracle(res, st, ro, tag):
    live = ro.j + (1 if ro.found else 0)
    assert res.status == st and res.j == ro.j and res.found == ro.found and res.vgoal == ro.vgoal, tag
    assert np.array_equal(res.nearest_log, ro.nearest_log), tag
    assert np.array_equal(res.accept_log, ro.accept_log), tag
    assert np.array_equal(res.pts[:live], ro.pts[:live]), tag
    assert np.array_equal(res.parent[:live], ro.parent[:live]), tag
    assert np.array_equal(res.vcost[:live], ro.vcost[:live]), tag
    assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near, tag


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", KERNELS_NOFAULT)
@pytest.mark.parametrize("c", farnn.PIPE_CASES, ids=lambda c: c["id"])
def test_pipe_pocket_cases_vs_oracle(gpu_ctx, c, kernel):
    """`block` runs rrt_pipe_kernel (checked through a batch of one); the other kernels scan every vertex and are controls."""
    _pipe_device_vs_oracle(gpu_ctx, c, kernel)
    if kernel == "block":
        og8, samples, r2 = farnn.pipe_case(c)
        b = _ffi.Batch(gpu_ctx, 1, c["n"], logs=True, team=1)
        qu, keep = _ffi.make_query(c["alg"], c["n"], c["xs"], c["xg"], samples, r2_rewire=r2)
        b.set_query(0, qu)
        b.launch()
        b.sync()
        assert b.kernel_name() == "rrt_pipe_kernel"
        st, ro = oracle.plan(og8, c["n"], c["alg"], c["xs"], c["xg"], samples, r2_rewire=r2)
        _batch_vs_oracle(b.get_result(0), st, ro, c["id"])
        b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["block", "serial"])
def test_pipe_pocket_fuzz_vs_oracle(gpu_ctx, kernel):
    """The 24 cases of farnn.pipe_fuzz_cases (RRTStandard and RRT* with r_rewire = 64), none skipped."""
    for c in farnn.pipe_fuzz_cases():
        _pipe_device_vs_oracle(gpu_ctx, c, kernel)


@pytest.mark.gpu
def test_pipe_pocket_batch_one_cu_per_query(gpu_ctx):
    """Ten pocket queries at once in one batch on rrt_pipe_kernel, one CU each: fuzz maps share one grid only when equal, so
    every query runs on the 63 x 63 L-shaped map with its own start, seed and planner; each one against the oracle."""
    c0 = farnn.PIPE_CASES[0]
    og8 = farnn.pocket_grid(c0["W"], c0["H"], c0["rects"])
    gpu_ctx.set_grid(og8)
    free = np.argwhere(og8 == 0)
    Q, n = 10, 4000
    rng = np.random.default_rng(31)
    b = _ffi.Batch(gpu_ctx, Q, n, logs=True, team=1)
    keep, refs, reached = [], [], 0
    for q in range(Q):
        alg = q % 2
        xs = (int(rng.integers(48, 63)), int(rng.integers(48, 63)))
        xg = (int(rng.integers(48, 63)), int(rng.integers(48, 63)))
        samples = hostprep.draw_free_samples(np.random.default_rng(500 + q), free, n)
        r2 = hostprep.radius_threshold(64) if alg else 0
        qu, k = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2)
        keep.append(k)
        b.set_query(q, qu)
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2)
        refs.append((st, ro))
        reached += farnn.coverage("pipe", 63, 63, alg >= 1, r2, samples, ro.pts, ro.nearest_log, ro.jlog)["reach"] > 0
    assert reached >= Q // 2
    b.launch()
    b.sync()
    assert b.kernel_name() == "rrt_pipe_kernel"
    for q in range(Q):
        _batch_vs_oracle(b.get_result(q), *refs[q], f"query {q}")
    b.close()


def _dubins_device_vs_oracle(ctx, c, serial, audit=True):
    og8, samples, heads, r2 = farnn.dubins_case(c)
    ctx.set_grid(og8)
    try:
        res, ro = device_vs_oracle_dubins(ctx, og8, c["star"], c["n"], c["xs"], c["xg"], samples, heads, c["rr"], c["rho"],
                                          serial=serial)
    except AssertionError as e:
        raise AssertionError(f"Dubins pocket case {c['id']} ({c['W']}x{c['H']} star {c['star']}) serial={serial}") from e
    if not audit:
        return
    a = oracle.dubins_audit(og8, c["n"], c["star"], samples, heads, res.pts, res.head, res.vcost, res.parent, res.j, r2_rewire=r2,
                            rho=c["rho"], nh=64)
    assert a["n_accepted"] == res.j - 1
    assert_audit_clean(a, c["star"])


@pytest.mark.gpu
@pytest.mark.parametrize("serial", [False, True])
@pytest.mark.parametrize("c", farnn.DUBINS_CASES, ids=lambda c: c["id"])
def test_dubins_pocket_cases_vs_oracle(gpu_ctx, c, serial):
    _dubins_device_vs_oracle(gpu_ctx, c, serial)


@pytest.mark.gpu
def test_dubins_pocket_fuzz_vs_oracle(gpu_ctx):
    """farnn.dubins_fuzz_cases: grids with 63 < max(W, H) <= 127, the default kernel and the serial one on every case, bit for
    bit against the oracle like test_device_dubins_fuzz_small.  (No libm audit here: with rho 1 and 2 on integer poses, a
    sample can lie on a quarter circle from its nearest vertex, a word whose straight part is exactly 0; the shared header's
    arithmetic finds it, dubins_ref.c's p^2 rounds below zero and it takes a word one full turn longer.)"""
    for c in farnn.dubins_fuzz_cases():
        for serial in (False, True):
            _dubins_device_vs_oracle(gpu_ctx, c, serial, audit=False)
