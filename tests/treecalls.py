"""Straight-line tree calls on the GPU (grow, keep_tree, reroot, connect_goals, routes), the helpers more than one test module uses:
the launch shapes a non-Informed query can take, cases planned by the oracle and cached once per process, maps and sample streams,
a query planned on a batch of its own, one grow against growref's restatement, the comparisons of results and routes, and the
refusals.  tree_of, same_result and snapshot take the headings along where a result has them, so the Dubins tests use them too.
The cache is keyed by a case's own parameters.  Asserts here are not rewritten by pytest: orchelp.differ says where arrays differ."""
import numpy as np
import pytest

import goalref
import growref
import keepref
import oracle
import routeref
from orchelp import differ
from rrtplanner_amd import _ffi, hostprep
from rrtplanner_amd.oggen import perlin_occupancygrid, random_connected_pair

N, RR = 2000, 24
R2 = hostprep.radius_threshold(RR)
# the committer + worker pair of 64: what a batch of one or two RRTStandard / RRT* queries runs when it is capped at 64 (one query) or
# cannot have 129 compute units per query (two), and the same pair on 2 x 64 workers, the default of a single query without a cap
ONE_SHIFT = "rrt_expand_block_kernel<64, 1, true, false> as rrt_block_commit_kernel + rrt_block_work_kernel<64, 1, false>"
TWO_SHIFTS = ONE_SHIFT + " in 2 shifts"


MI355X_CUS = 256  # the compute units of the device the GPU tests run on: the fixed names below hold for it, as TWO_SHIFTS needs 129 of them


def planned_name(Q, want=64, cus=MI355X_CUS, narrow=False):
    """The name of the kernel a batch of Q RRTStandard / RRT* queries with a team cap of `want` runs on an otherwise idle device of
    `cus` compute units, one shift: pick_team of rrt_engine.hip restated, then the row of rrt_block_variants.def that plan_launch
    takes (tests/variants.py, test_variant_matrix.py).  narrow: the RRT* queries have r2_rewire < variants.NARROW_R2 (only a
    pipelined team of two asks)."""
    import variants

    def stride_of(g):
        step = 8 if g <= 16 else (4 if g == 32 else 2)
        stride = (Q + step - 1) // step * step
        if g == 32 and stride % 8 == 0:
            stride += 4
        if g == 64 and stride % 4 == 0:
            stride += 2
        return stride
    team, pipe, pipe_g = 1, False, 0
    for g in (2, 4, 8, 16, 32, 64):
        if g <= want and stride_of(g) * g <= cus:
            team = g
    for g in (2, 3, 4, 8, 16, 32, 64):
        if g <= want and stride_of(g) * (g + 1) <= cus:
            pipe_g = g
    if pipe_g != 0 and team <= 2 * pipe_g:
        team, pipe = pipe_g, True
    if team == 1:
        return "rrt_pipe_kernel"
    wide = pipe and team == variants.WIDE_TEAM and not narrow
    split = pipe and not wide and team >= variants.SPLIT_FROM
    for r in variants.rows():
        if r.G == team and r.pipe == pipe and not r.inf and (r.BSM > 16) == wide and (r.kind == "S") == split:
            return variants.kernel_name(r)
    raise LookupError(f"no team kernel for Q={Q}, want={want}, cus={cus}")


def team_name_ok(name, Q):
    """the "team" shape (no cap) held to its name: one query runs two shifts, two run the pair of 64 in one shift, and a larger
    batch what the launch plan gives it (three queries on 256 compute units: the pair of 32, because the stride of a team of 64 is
    6 slots for them)"""
    return name == (TWO_SHIFTS if Q == 1 else ONE_SHIFT if Q == 2 else planned_name(Q))


def team64_name_ok(name, Q):
    """the cap of 64: as team_name_ok, but a single query keeps one shift"""
    return name == (ONE_SHIFT if Q <= 2 else planned_name(Q, 64))


SHAPES = {  # launch shape -> (Batch keywords, what the kernel's name has to say: check(name, Q) with Q the queries of the batch)
    "team": (dict(), team_name_ok),
    "team8": (dict(team=8), lambda s, Q=1: s.startswith("rrt_expand_block_kernel<8,")),
    "team2": (dict(team=2), lambda s, Q=1: s.startswith("rrt_expand_block_kernel<2,")),
    "pipe1": (dict(team=1), lambda s, Q=1: s == "rrt_pipe_kernel"),
    "block1": (dict(team=1, pipe1=False), lambda s, Q=1: s == "rrt_expand_block_kernel<1, 16, false, false>"),
    "serial": (dict(serial=True), lambda s, Q=1: s == "rrt_expand_kernel<false, false>"),
    "team64": (dict(team=64), team64_name_ok),  # (last: test_tree_sequences_gpu.py pairs shapes with seeds by position)
}
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------------------------------------ cases the oracle planned
def base(W=200, gseed=3, pair=5, n=N, seed=21, alg=1, r2=R2):
    """a noise map, a connected start / goal pair, n samples and the oracle's plan of them"""
    key = ("base", W, gseed, pair, n, seed, alg, r2)

    def make():
        og = perlin_occupancygrid(W, W, seed=gseed)
        og8 = oracle.og_u8(og)
        xs, xg = random_connected_pair(og, np.random.default_rng(pair))
        samples = hostprep.draw_free_samples(np.random.default_rng(seed), np.argwhere(og8 == 0), n)
        st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2)
        return dict(og8=og8, xs=xs, xg=xg, samples=samples, st=st, ro=ro, n=n, alg=alg, r2=r2, key=key)
    return _once(key, make)


def mixed_goals(og8, seed=9, m=64):
    free = np.argwhere(og8 == 0)
    g = free[np.random.default_rng(seed).integers(0, len(free), size=m - 4)]
    return np.concatenate([g, np.argwhere(og8 != 0)[::max(1, int((og8 != 0).sum()) // 4)][:4]])[:m]


def wall(c):
    """the base map with a wall stamped in, the restatement's seed on it and the samples of the grow"""
    def make():
        og2 = c["og8"].copy()
        W = og2.shape[0]
        og2[W // 2:W // 2 + 3, :] = 1  # a wall across the map ...
        og2[W // 2:W // 2 + 3, (c["xs"][1] + W // 2) % W:(c["xs"][1] + W // 2) % W + 12] = 0  # ... with one gap
        og2[c["xs"][0], c["xs"][1]] = 0
        ro = c["ro"]
        alive, ids, sp, sc, spar = keepref.view(og2, ro.pts, ro.parent, ro.vcost, ro.j)
        cut = np.flatnonzero(~alive)
        cut_free = [k for k in cut.tolist() if og2[ro.pts[k][0], ro.pts[k][1]] == 0]
        m = c["n"] - len(ids)
        rng = np.random.default_rng(77)
        fill = hostprep.draw_free_samples(rng, np.argwhere(og2 == 0), m)
        special = np.concatenate([ro.pts[cut_free[:40]], [c["xs"]], np.argwhere(og2 != 0)[:1]]).astype(fill.dtype)
        where = rng.choice(m, size=len(special), replace=False)
        fill[where] = special
        return dict(og2=og2, alive=alive, ids=ids, seed=(sp, sc, spar), cut_free=cut_free, samples=fill, special=special, where=where)
    return _once(("wall",) + c["key"][1:], make)  # (c is a case of base(): the key is its parameters)


def oracle_case(og8, alg, n, xs, xg, samples, r2):
    st, ro = oracle.plan(og8, n, alg, xs, xg, samples, r2_rewire=r2)
    return dict(og8=og8, xs=np.asarray(xs), xg=np.asarray(xg), samples=samples, st=st, ro=ro, n=n, alg=alg, r2=r2)


SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025]


def sized(k, seed):
    """an empty 64 x 64 map and samples that leave a tree of exactly k vertices: k - 1 distinct cells, then repeats"""
    og8 = np.zeros((64, 64), dtype=np.uint8)
    rng = np.random.default_rng(seed)
    cells = rng.permutation(64 * 64)
    xs = np.array(divmod(int(cells[0]), 64))
    distinct = np.array([divmod(int(v), 64) for v in cells[1:k]], dtype=np.int64).reshape(-1, 2)
    n = 1040
    fill = np.tile(distinct[:1] if k > 1 else xs[None, :], (n - (k - 1), 1))
    if k == 1:
        og8 = og8.copy()
        og8[max(xs[0] - 1, 0):xs[0] + 2, max(xs[1] - 1, 0):xs[1] + 2] = 1
        og8[xs[0], xs[1]] = 0  # the start boxed in: no sample is ever accepted
        fill = np.tile(np.array([[(xs[0] + 5) % 64, (xs[1] + 5) % 64]]), (n, 1))
    return og8, xs, np.concatenate([distinct, fill])[:n], n


# ------------------------------------------------------------------------------------------------ maps and sample streams
def wall_map(W=200, H=160):
    """two walls across the map, each with a gap at one end, and a closed box"""
    og = np.zeros((W, H), dtype=np.int64)
    og[W // 3:W // 3 + 4, :H * 3 // 4] = 1
    og[2 * W // 3:2 * W // 3 + 3, H // 4:] = 1
    og[20:41, 120:141] = 1
    og[22:39, 122:139] = 0  # the inside of the box is free and closed
    return og


def free_samples(og, n, seed):
    return hostprep.draw_free_samples(np.random.default_rng(seed), np.argwhere(og == 0), n)


def free_goals(og, m, seed):
    free = np.argwhere(og == 0)
    return free[np.random.default_rng(seed).integers(0, len(free), size=m)]


def corridor_map(W=200, H=160):
    """three corridors along x, joined at alternating ends, each a slalom round pillars that stand alternately on its lower and its
    upper wall; and the way through them"""
    og = np.zeros((W, H), dtype=np.int64)
    og[0:185, 38:42] = 1   # between corridors 1 and 2, open at the right end
    og[15:200, 78:82] = 1  # between corridors 2 and 3, open at the left end
    way = [(5, 20)]
    for c, (y0, xs) in enumerate([(0, range(20, 180, 20)), (42, range(180, 20, -20)), (82, range(20, 180, 20))]):
        for i, x in enumerate(xs):
            if i % 2 == 0:
                og[x, y0:y0 + 24] = 1
                way.append((x, y0 + 30))
            else:
                og[x, y0 + 14:y0 + 38] = 1
                way.append((x, y0 + 8))
        way.append((192, y0 + 20) if c % 2 == 0 else (8, y0 + 20))
        if c < 2:
            way.append((192, y0 + 60) if c % 2 == 0 else (8, y0 + 60))
    return og, way


def march(way, step=3):
    """samples along the polyline `way` in steps of at most `step` cells a coordinate: each one's nearest vertex is (almost always) the
    one before it, which chains the tree"""
    out, p = [], np.array(way[0])
    for w in way[1:]:
        while np.any(p != np.array(w)):
            p = p + np.clip(np.array(w) - p, -step, step)
            out.append(p.tolist())
    return np.array(out)


# ------------------------------------------------------------------------------------------------ batches and queries
def shaped_batch(ctx, c, shape, Q=1, n_cap=None, og8=None):
    kw, _ = SHAPES[shape]
    ctx.set_grid(c["og8"] if og8 is None else og8)
    return _ffi.Batch(ctx, Q, n_cap or c["n"], logs=True, **kw)


def set_case_query(b, q, c):
    qu, keep = _ffi.make_query(c["alg"], c["n"], c["xs"], c["xg"], c["samples"], r2_rewire=c["r2"])
    b.set_query(q, qu)
    return keep


def plan_on_own_batch(ctx, alg, n, xs, xg, samples, r2=0, goal_d2=0, Cmat=None, **bkw):
    """one query on a batch of its own, launched and synchronised: (batch, result)"""
    b = _ffi.Batch(ctx, 1, n, **bkw)
    q, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=r2, goal_d2=goal_d2, Cmat=Cmat)
    b.set_query(0, q)
    b.launch()
    b.sync()
    return b, b.get_result(0)


# ------------------------------------------------------------------------------------------------ results, exactly
def tree_of(r):
    """(pts, parent, vcost, j) of a result or a restatement, copied; (pts, head, parent, vcost, j) where it has headings"""
    head = (np.array(r.head, dtype=np.int64),) if hasattr(r, "head") else ()
    return (np.array(r.pts, dtype=np.int64),) + head + (np.array(r.parent, dtype=np.int64), np.array(r.vcost), r.j)


def same_result(res, g, log0=None):
    """the device's result against a grown restatement g (growref's, or posegrowref's where the result has headings); log0: the rows
    of the logs that the grown iterations wrote, which are compared with the statistics when it is given"""
    posed = hasattr(res, "head")
    live = g.j + g.found
    assert (res.status, res.j, res.found, res.vgoal, res.rows) == (g.status, g.j, g.found, g.vgoal, g.rows)
    assert np.array_equal(res.pts[:live], g.pts[:live]) and np.array_equal(res.parent[:live], g.parent[:live]), (differ(res.pts[:live], g.pts[:live]), differ(res.parent[:live], g.parent[:live]))
    if posed:
        assert np.array_equal(res.head[:live], g.head[:live]), differ(res.head[:live], g.head[:live])
    assert np.array_equal(res.vcost[:live].view(np.int64), g.vcost[:live].view(np.int64)), differ(res.vcost[:live], g.vcost[:live])
    if log0 is not None:
        m = len(g.accept_log)
        assert np.array_equal(res.nearest_log[log0:log0 + m], g.nearest_log), differ(res.nearest_log[log0:log0 + m], g.nearest_log)
        assert np.array_equal(res.accept_log[log0:log0 + m], g.accept_log), differ(res.accept_log[log0:log0 + m], g.accept_log)
        assert np.array_equal(res.j_log[log0:log0 + m], g.jlog), differ(res.j_log[log0:log0 + m], g.jlog)
        assert res.sum_j == g.sum_j and res.sum_near == g.sum_near  # the statistics count the grown iterations alone
        if posed:  # ... and the cells of the nearest-vertex search, which test_dubins.py compares between device and oracle
            assert res.sum_cells_nn == g.sum_cells_nn, (res.sum_cells_nn, g.sum_cells_nn)


def snapshot(res):
    live = res.j + (1 if res.found else 0)
    head = (res.head[:live].copy(),) if hasattr(res, "head") else ()
    return (res.status, res.j, res.vgoal, res.found, res.sum_j, res.sum_near, res.pts[:live].copy()) + head + (res.parent[:live].copy(), res.vcost[:live].copy())


def same_snapshot(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


ROUTE_ARRAYS = ("vertex", "cost", "length", "offsets", "xy", "ids")


def same_routes(got, want):
    for name, g, w in zip(ROUTE_ARRAYS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(g, w), (name, np.flatnonzero(np.asarray(g != w).reshape(len(g), -1).any(axis=1))[:8])


# ------------------------------------------------------------------------------------------------ the tree calls against the host checks
def goals_and_routes(b, q, og8, res, seed=9, connected=8):
    """connect_goals and routes (shortcut) of query q for 64 goals against goalref / routeref on the arrays of `res`; at least
    `connected` of the goals have to see a vertex"""
    goals = mixed_goals(og8, seed)
    pts, parent, vcost, j = tree_of(res)
    v, cost = b.connect_goals(q, goals)
    rv, rc, _ = goalref.connect(og8, pts, vcost, j, goals)
    assert np.array_equal(v, rv) and np.array_equal(cost, rc) and (rv >= 0).sum() >= connected, (differ(v, rv), differ(cost, rc), (rv >= 0).sum())
    got = b.routes(q, goals, shortcut=True)
    want = routeref.routes(og8, pts, vcost, parent, j, goals, cut=True)
    for x, y in zip(got, want):
        assert np.array_equal(x, y), differ(x, y)


def class_goals_and_routes(p, og8, g, goals):
    """RRT.connect_goals and RRT.routes_to (shortcut) against goalref / routeref on the restatement's grown arrays"""
    v, cost = p.connect_goals(goals)
    rv, rc, _ = goalref.connect(og8, g.pts, g.vcost, g.j, goals)
    assert np.array_equal(v, rv) and np.array_equal(cost, rc) and (rv >= 0).sum() >= 8, (differ(v, rv), differ(cost, rc), (rv >= 0).sum())
    want = routeref.routes(og8, g.pts, g.vcost, g.parent, g.j, goals, cut=True)
    routes, length = p.routes_to(goals, shortcut=True)
    assert np.array_equal(length, want[2]) and len(routes) == len(goals), (differ(length, want[2]), len(routes), len(goals))
    for k, r in enumerate(routes):
        lo, hi = want[3][k], want[3][k + 1]
        assert (r is None and lo == hi) or np.array_equal(r, want[4][lo:hi]), k


def shape_ran(b, shape, Q=1):
    """the last launch of batch b (Q queries, none Informed) ran the kernel of this launch shape, by its exact name where the shape
    is "team" or "team64"; a single query on 128 workers (two shifts) or 64, and no launch fell back to one CU per query"""
    name = b.kernel_name()
    assert SHAPES[shape][1](name, Q), (shape, Q, name)
    if Q == 1 and shape in ("team", "team64"):
        assert b.team() == ((128, 0) if shape == "team" else (64, 0)), (shape, b.team())


def grow_checked(b, q, og8, prev, view, samples, c, shape, Q=1):
    """one grow of query q of a batch of Q on map og8 from the tree `prev` = (pts, parent, vcost, j); view: the tree was kept on og8.
    Checked against growref.  Returns (restatement, result)."""
    ids, sp, sc, spar = growref.seed(*prev, og8_view=og8 if view else None)
    g = growref.grow(og8, c["alg"], c["n"], c["xg"], c["r2"], sp, sc, spar, samples)
    j0, old_id, log0 = b.grow(q, samples)
    assert j0 == len(ids) == log0 and np.array_equal(old_id, ids), (j0, len(ids), log0, differ(old_id, ids))
    b.launch()
    b.sync()
    res = b.get_result(q)
    same_result(res, g, log0)
    info = b.team_info()
    assert info["timeouts"] == 0 and b.team()[1] == 0, info
    shape_ran(b, shape, Q)
    ms = b.grow_ms()
    assert len(ms) == 3 and all(t >= 0.0 for t in ms)
    return g, res


# ------------------------------------------------------------------------------------------------ refusals
def refused_with_code(code, call):
    """call() is refused with this code; the text of the refusal"""
    with pytest.raises(_ffi.RRTError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def refused_with_word(code, word, fn, *args):
    with pytest.raises(_ffi.RRTError) as e:
        fn(*args)
    assert e.value.code == code and word in str(e.value), str(e.value)
