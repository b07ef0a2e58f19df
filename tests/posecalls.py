"""Dubins tree calls on the GPU, the helpers more than one test module uses: a poseref workload planned on a batch of its own (told
apart by what they return), one grow_poses against posegrowref's restatement, a refusal held to its golden text, and the driver of
the Dubins kernels against the oracle with its independent checks.  The workloads are poseref.py's and posegrowref.py's; same_result
and the refusals by code and word are treecalls.py's.  Asserts here are not rewritten by pytest: orchelp.differ says where."""
import math

import numpy as np
import pytest

import oracle
import poseref
from orchelp import differ
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd import dubins as dub
from treecalls import same_result

GROW_KERNELS = {"block": (False, "rrt_dubins_block_kernel"), "serial": (True, "rrt_expand_kernel<false, true>")}


# ------------------------------------------------------------------------------------------------ a workload on a batch of its own
def planned_batch(ctx, w, serial=False):
    """workload w on a batch of its own, launched and synchronised, its tree the oracle's: the batch"""
    ctx.set_grid(w.og8)
    b = _ffi.Batch(ctx, 1, w.n, dubins=True, serial=serial)
    q, keep = poseref.device_query(w)
    b.set_query(0, q)
    b.launch()
    b.sync()
    res = b.get_result(0)
    assert res.status == w.status and res.j == w.j
    assert np.array_equal(res.parent[:w.j], w.ro.parent[:w.j]), differ(res.parent[:w.j], w.ro.parent[:w.j])
    assert np.array_equal(res.head[:w.j], w.ro.head[:w.j]), differ(res.head[:w.j], w.ro.head[:w.j])
    assert np.array_equal(res.vcost[:w.j], w.ro.vcost[:w.j]), differ(res.vcost[:w.j], w.ro.vcost[:w.j])
    return b


def planned_batch_and_result(ctx, w):
    """the same, and the query's result: (batch, result)"""
    b = planned_batch(ctx, w)
    return b, b.get_result(0)


def planned_logged_batch(ctx, w, kernel, Q=1, stream=None):
    """workload w in every query of a batch of its own, launched and synchronised, its trees the oracle's; stream: (samples, headings,
    n) in place of the workload's"""
    ctx.set_grid(w.og8)
    samples, heads, n = stream if stream is not None else (w.samples, w.heads, w.n)
    b = _ffi.Batch(ctx, Q, n, logs=True, dubins=True, serial=GROW_KERNELS[kernel][0])
    keep = []
    for q in range(Q):
        qu, k = _ffi.make_query(_ffi.ALG_DUBINS_STAR if w.star else _ffi.ALG_DUBINS, n, w.xs, w.xg, samples, r2_rewire=w.r2, headings=heads, rho=w.rho,
                                nh=w.nh)
        keep.append(k)
        b.set_query(q, qu)
    b.launch()
    b.sync()
    for q in range(Q):
        res = b.get_result(q)
        j = w.j
        assert res.j == j and np.array_equal(res.parent[:j], w.ro.parent[:j]), (q, res.j, j, differ(res.parent[:j], w.ro.parent[:j]))
        assert np.array_equal(res.head[:j], w.ro.head[:j]), (q, differ(res.head[:j], w.ro.head[:j]))
        assert np.array_equal(res.vcost[:j].view(np.int64), w.ro.vcost[:j].view(np.int64)), (q, differ(res.vcost[:j], w.ro.vcost[:j]))
    b.own_n = n
    return b


def grow_poses_checked(b, q, w, g, ids, samples, kernel):
    """one grow_poses of query q, launched, against the restatement g whose seed has the original numbers ids"""
    j0, old_id, log0 = b.grow_poses(q, samples)
    assert j0 == len(ids) == log0 == g.j0 and old_id.dtype == np.int32 and np.array_equal(old_id, ids), (j0, len(ids), log0, g.j0, differ(old_id, ids))
    b.launch()
    b.sync()
    res = b.get_result(q)
    same_result(res, g, log0)
    assert b.team()[1] == 0 and b.kernel_name() == GROW_KERNELS[kernel][1], b.kernel_name()  # team_fallbacks == 0: this kernel ran it all
    ms = b.grow_ms()
    assert len(ms) == 3 and all(t >= 0.0 for t in ms)
    return res


def refused_with_golden_text(golden, key, fn, *args, **fmt):
    """fn(*args) raises what golden[key] = (code, text) says, with exactly that text"""
    code, text = golden[key]
    with pytest.raises(ValueError if code == "ValueError" else _ffi.RRTError) as e:
        fn(*args)
    if code == "ValueError":
        assert str(e.value) == text, str(e.value)
    else:
        assert e.value.code == code and str(e.value) == f"librrt_hip error {code}: {text.format(**fmt)}", str(e.value)


# ------------------------------------------------------------------------------------------------ the Dubins kernels against the oracle
def _independent_sweep(og8, a, b, rho, nh):
    """The collision sweep of the edge a -> b WITHOUT include/rrt_dubins.h: the polyline of rrtplanner_amd/dubins.py (numpy /
    libm, its own word construction) sampled every DUB_DS = 0.5 cells of arc length, a sample occupying the cell round-half-up
    of its coordinates.  Returns (blocked, ambiguous) per sample: blocked = outside the grid or on an obstacle; ambiguous = a
    coordinate within 1e-7 of a cell boundary (libm and the fixed-order arithmetic may then name neighbouring cells)."""
    f = dub.dubins_polyline(a, b, rho, nh, ds=0.5) + 0.5
    cells = np.floor(f).astype(np.int64)
    amb = np.abs(f - np.round(f)).min(axis=1) < 1e-7
    inside = (cells[:, 0] >= 0) & (cells[:, 0] < og8.shape[0]) & (cells[:, 1] >= 0) & (cells[:, 1] < og8.shape[1])
    blocked = ~inside
    blocked[inside] = og8[cells[inside, 0], cells[inside, 1]] != 0
    return blocked, amb


def independent_collision_witness(og8, res, samples, heads, rho, nh, count=300):
    """The device's collision DECISIONS against the independent sweep above (the oracle shares the kernel's geometry header, so
    HIP == oracle says nothing about a wrong formula in it): every edge of the device's tree is free, and every iteration the
    device rejected although its cell was new has a blocked (or boundary-ambiguous) sample on the word nearest -> sample."""
    live = res.j + (1 if res.found else 0)
    par, pts, hd = res.parent[:live].astype(np.int64), res.pts[:live].astype(np.int64), res.head[:live].astype(np.int64)
    for c in range(1, live, max(1, live // count)):
        p = par[c]
        blocked, amb = _independent_sweep(og8, (pts[p, 0], pts[p, 1], hd[p]), (pts[c, 0], pts[c, 1], hd[c]), rho, nh)
        assert not np.any(blocked & ~amb), f"edge {p} -> {c} of the device's tree crosses an obstacle"
    first_index = {}
    for k in range(res.j - 1, 0, -1):
        first_index[(int(pts[k, 0]), int(pts[k, 1]))] = k
    rej = np.flatnonzero(res.accept_log == 0)
    seen = 0
    for i in rej[:: max(1, rej.size // count)]:
        x, y, h, jtop = int(samples[i, 0]), int(samples[i, 1]), int(heads[i]), int(res.j_log[i])
        if first_index.get((x, y), jtop) < jtop or jtop >= res.n:
            continue  # rejected as a duplicate of an earlier vertex (rrt.py:425) or because the tree is full
        v = int(res.nearest_log[i])
        blocked, amb = _independent_sweep(og8, (pts[v, 0], pts[v, 1], hd[v]), (x, y, h), rho, nh)
        assert np.any(blocked | amb), f"iteration {i}: rejected, but the word from vertex {v} to the sample is free"
        seen += 1
    return seen


def check_dubins_tree(og8, r, rho, nh, xs):
    live = r.j + (1 if r.found else 0)
    par, pts, hd = r.parent[:live].astype(np.int64), r.pts[:live].astype(np.int64), r.head[:live].astype(np.int64)
    assert par[0] == -1 and np.all(par[1:] >= 0) and np.all(par[1:] < np.arange(1, live)) and (pts[0, 0], pts[0, 1], hd[0]) == tuple(xs)
    assert np.all(og8[pts[:, 0], pts[:, 1]] == 0) and np.all((0 <= hd) & (hd < nh))
    assert len({(a, b) for a, b in pts[:r.j].tolist()}) >= r.j - 1  # one node per cell (xstart may repeat once, rrt.py:425)
    L = dub.dubins_shortest(pts[par[1:], 0], pts[par[1:], 1], 2 * math.pi * hd[par[1:]] / nh, pts[1:, 0], pts[1:, 1], 2 * math.pi * hd[1:] / nh, rho)[3]
    assert np.allclose(r.vcost[1:live], r.vcost[par[1:]] + L, rtol=0, atol=1e-8)
    for c in range(1, live, max(1, live // 300)):  # every edge's sweep is free
        p = par[c]
        cells = oracle.dub_sweep_cells(pts[p, 0], pts[p, 1], 2 * math.pi * hd[p] / nh, pts[c, 0], pts[c, 1], 2 * math.pi * hd[c] / nh, rho)
        assert np.all((cells >= 0) & (cells < og8.shape[0])) and np.all(og8[cells[:, 0], cells[:, 1]] == 0)


def assert_audit_clean(a, star):
    """What oracle/dubins_ref.c's second opinion must say about a tree (its head comment): every accept / reject and every
    chosen parent either equal to its own, or within the stated tolerance / ambiguity -- never plainly different."""
    assert a["nearest_mismatch"] == 0 and a["accept_mismatch"] == 0, a
    assert a["parent_wrong"] == 0 and a["parent_blocked"] == 0 and a["cost_mismatch"] == 0, a
    assert a["max_cost_err"] < 1e-8, a
    assert a["parent_is_argmin"] + a["parent_within_tol"] == a["n_accepted"], a
    # the tolerance classes are the exception, not the rule
    assert a["parent_within_tol"] <= max(3, a["n_accepted"] // 1000) and a["accept_ambiguous"] + a["parent_blocked_ambiguous"] <= max(3, a["n_accepted"] // 1000), a


def device_vs_oracle_dubins(ctx, og8, star, n, xs, xg, samples, heads, rr, rho, nh=64, serial=False, counters=False):
    """serial = False: the 16-samples-per-round kernel (rrt_dubins_block.h, the default); True: the one-sample-per-iteration
    kernel (RRT_FLAG_SERIAL), kept as a second implementation of the same semantics."""
    r2 = hostprep.radius_threshold(rr) if star else 0
    q, keep = _ffi.make_query(_ffi.ALG_DUBINS_STAR if star else _ffi.ALG_DUBINS, n, xs, xg, samples, r2_rewire=r2, headings=heads, rho=rho, nh=nh)
    rc, res = ctx.plan(q, n, logs=True, serial=serial)
    st, ro = oracle.dubins_plan(og8, n, star, xs, xg, samples, heads, r2_rewire=r2, rho=rho, nh=nh, counters=counters)
    assert rc == st
    live = ro.j + (1 if ro.found else 0)
    assert (res.j, res.found, res.vgoal) == (ro.j, ro.found, ro.vgoal)
    assert np.array_equal(res.nearest_log, ro.nearest_log) and np.array_equal(res.accept_log, ro.accept_log), (differ(res.nearest_log, ro.nearest_log), differ(res.accept_log, ro.accept_log))
    assert np.array_equal(res.pts[:live], ro.pts[:live]) and np.array_equal(res.head[:live], ro.head[:live]), (differ(res.pts[:live], ro.pts[:live]), differ(res.head[:live], ro.head[:live]))
    assert np.array_equal(res.parent[:live], ro.parent[:live]), differ(res.parent[:live], ro.parent[:live])
    assert np.array_equal(res.vcost[:live], ro.vcost[:live]), differ(res.vcost[:live], ro.vcost[:live])  # bit-exact: one arithmetic on both sides
    assert res.sum_j == ro.sum_j and res.sum_cells_nn == ro.sum_cells_nn and res.sum_near == ro.sum_near
    return res, ro
