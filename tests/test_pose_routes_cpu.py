"""CPU: the host restatement of rrt_batch_pose_routes (poseroutesref.py) pinned to things it does not share with the kernel, and the
conditions that make a GPU comparison against it worth something.

poseroutesref takes its rows from a Python parent walk, its lengths from the oracle's words and its points from
tests/dubpoints, which includes include/rrt_dubins_points.h -- the header the kernel includes.  Two checks here share nothing with
that header: floor(P + 0.5) of every point against oracle.dub_sweep_cells (the oracle's own sweep, which calls dub_sweep_cell),
exactly; and every point against numpy's dubins_polyline (libm, independent formulas) within 1e-8, the tolerance tests/test_dubins.py
uses between the two arithmetics.  length == cost is an equality of bits, not a tolerance."""
import numpy as np
import pytest

import oracle
import poseref
import posekeepref
import poseroutesref as prr
from orchelp import bits
from rrtplanner_amd.dubins import WORDS, dubins_polyline, dubins_shortest

WORKLOADS = ["A", "B", "D", "E", "G1", "G256"]
TOL = 1e-8


def _own_walk(parent, v):
    out = [v]
    while out[-1] != 0:
        out.append(int(parent[out[-1]]))
    return out[::-1]


TIES = []  # legs on which libm and the fixed-order arithmetic chose different words of one length


def _libm_line(a, b, rho, nh):
    """numpy's polyline of the leg a -> b: dubins_polyline, which takes ITS shortest word.  Two words can have one length (equal
    headings across a chord: RLR and LRL are mirror images), and then the last bit decides which one either arithmetic takes; the
    polylines are then mirror images, not the same curve.  Such a leg -- libm's word is another than the oracle's, and the two
    lengths agree within 1e-9 -- is integrated here with numpy's sine and cosine along the ORACLE's word (its t, p, q), point by
    point as dubins_polyline does it.  Every other leg goes through dubins_polyline as it is."""
    a, b = tuple(int(x) for x in a), tuple(int(x) for x in b)
    th0, th1 = poseref.theta(a[2], nh), poseref.theta(b[2], nh)
    t, p, q, length, word = oracle.dub_shortest(float(a[0]), float(a[1]), th0, float(b[0]), float(b[1]), th1, rho)
    lt, lp, lq, llen, lword = (float(v) for v in dubins_shortest(a[0], a[1], th0, b[0], b[1], th1, rho))
    if int(lword) == word:
        return dubins_polyline(a, b, rho, nh, 0.5)
    assert abs(llen - length) < 1e-9, (a, b, WORDS[int(lword)], WORDS[word], llen, length)
    TIES.append((a, b))
    s = np.append(np.arange(0.0, length, 0.5), length) / rho
    out = np.empty((s.size, 2))
    x, y, th, start = 0.0, 0.0, th0, 0.0
    for kind, tau_len in zip([{"L": 1, "S": 0, "R": -1}[ch] for ch in WORDS[word]], (t, p, q)):
        m = (s >= start) & (s <= start + tau_len + 1e-12)
        tau = s[m] - start
        if kind == 0:
            out[m, 0], out[m, 1] = x + np.cos(th) * tau, y + np.sin(th) * tau
            x, y = x + np.cos(th) * tau_len, y + np.sin(th) * tau_len
        else:
            out[m, 0] = x + kind * (np.sin(th + kind * tau) - np.sin(th))
            out[m, 1] = y - kind * (np.cos(th + kind * tau) - np.cos(th))
            x, y = x + kind * (np.sin(th + kind * tau_len) - np.sin(th)), y - kind * (np.cos(th + kind * tau_len) - np.cos(th))
            th = th + kind * tau_len
        start += tau_len
    return np.array(a[:2], dtype=np.float64) + out * rho


def _check_case(c, libm=True):
    """rows, lengths, cells and (libm) numpy points of every route of case c, on the map c.og8"""
    w, r = c.w, c.routes
    ro, og8 = w.ro, c.og8
    W, H = og8.shape
    m = len(c.goals)
    assert r.offsets[0] == 0 and r.point_offsets[0] == 0 and r.offsets[m] == len(r.rows) == len(r.ids) and r.point_offsets[m] == len(r.points)
    on = r.vertex >= 0
    assert np.array_equal(bits(r.length[on]), bits(r.cost[on])), "length != cost"
    assert np.all(np.isinf(r.length[~on])) and np.all(np.diff(r.offsets)[~on] == 0) and np.all(np.diff(r.point_offsets)[~on] == 0)
    for g in range(m):
        if not on[g]:
            continue
        route, ids = r.route(g), r.ids[r.offsets[g]:r.offsets[g + 1]]
        vs = _own_walk(ro.parent, int(r.vertex[g]))  # what paths_to_poses does: route2gv, then the poses, then the goal pose
        assert ids.tolist() == vs + [-1]
        assert np.array_equal(route[:-1], np.column_stack([ro.pts[vs], ro.head[vs]])) and np.array_equal(route[-1], c.goals[g])
        if c.alive is not None:
            assert c.alive[vs].all()
        path = r.path(g)
        assert np.array_equal(path[-1], c.goals[g][:2].astype(np.float64))
        at = 0
        for a, b in zip(route[:-1], route[1:]):
            th0, th1 = poseref.theta(a[2], w.nh), poseref.theta(b[2], w.nh)
            length = oracle.dub_shortest(float(a[0]), float(a[1]), th0, float(b[0]), float(b[1]), th1, w.rho)[3]
            n = int(np.floor(length / 0.5)) + 1
            p = path[at:at + n]
            at += n
            assert np.array_equal(p[0], a[:2].astype(np.float64))  # sample 0 is the start pose exactly
            cells = oracle.dub_sweep_cells(int(a[0]), int(a[1]), th0, int(b[0]), int(b[1]), th1, w.rho, cap=n + 16)
            mine = np.floor(p + 0.5).astype(np.int32)
            # (the oracle's sweep lists its samples and may list the end cell behind them: the samples are what is compared)
            assert len(cells) >= n and np.array_equal(mine, cells[:n]), (g, a, b)
            assert np.all((mine[:, 0] >= 0) & (mine[:, 0] < W) & (mine[:, 1] >= 0) & (mine[:, 1] < H)) and not np.any(og8[mine[:, 0], mine[:, 1]])
            assert og8[b[0], b[1]] == 0
            if libm and length > 0.0:
                line = _libm_line(a, b, w.rho, w.nh)
                assert 0 <= len(line) - n <= 1, (len(line), n, length)
                assert np.max(np.abs(line[:n] - p)) < TOL, (g, a, b, np.max(np.abs(line[:n] - p)))
        assert at == len(path) - 1


@pytest.mark.parametrize("name", WORKLOADS)
def test_workload_rows_lengths_cells_and_libm_points(name):
    before = len(TIES)
    c = prr.case(name)
    _check_case(c)
    assert 8 * (len(TIES) - before) <= len(c.routes.rows), TIES[before:]  # ties between words are the exception (one heading: G1)


@pytest.mark.parametrize("name", WORKLOADS)
def test_conditions_that_make_the_comparison_worth_running(name):
    c = prr.case(name)
    poseref.check_conditions(c.w)
    r = c.routes
    on = int((r.vertex >= 0).sum())
    assert 2 * on >= len(c.goals)
    assert len(r.rows) > 3 * on, (len(r.rows), on)  # the mean route has more than 3 rows
    assert max(n for _, n in r.leg_spans) > 64  # a leg longer than a wavefront
    starts = np.array([a for a, _ in r.leg_spans])
    assert max(int(((starts >= b) & (starts < b + 64)).sum()) for b in range(0, len(r.points), 64)) >= 3  # a wavefront of points on 3 legs


def test_nothing_connects_on_workload_f():
    c = prr.case("F")
    poseref.check_conditions(c.w)
    r = c.routes
    assert np.all(r.vertex == -1) and np.all(r.offsets == 0) and np.all(r.point_offsets == 0) and len(r.rows) == 0 and len(r.points) == 0


def test_a_chain_of_half_cell_legs_repeats_every_end_pose():
    c = prr.half_cell_chain()
    _check_case(c)
    r = c.routes
    assert r.vertex[0] >= 5 and r.vertex[2] == -1
    route, path = r.route(0), r.path(0)
    tree_legs = len(route) - 2
    for k in range(tree_legs):  # a straight word of length exactly 4.0: 9 samples, the last of them the end pose
        p = path[9 * k:9 * k + 9]
        assert np.array_equal(p[:, 0], route[k][0] + 0.5 * np.arange(9)) and np.all(p[:, 1] == prr.CHAIN_Y)
        assert np.array_equal(p[8], route[k + 1][:2].astype(np.float64)) and np.array_equal(path[9 * k + 9], p[8])  # ... twice


def test_a_goal_pose_that_is_a_vertex_pose():
    for name in ("G1", "G256"):
        c = prr.case(name)
        w, r = c.w, c.routes
        v = w.j // 2
        assert tuple(c.goals[0]) == (w.ro.pts[v, 0], w.ro.pts[v, 1], w.ro.head[v]) and r.vertex[0] >= 0
    for j in (63, 64, 65):  # the root's own pose as a goal: vertex 0, cost 0.0, a leg of no length and one point, then the goal cell
        c = prr.made_case(poseref.stride_tree(j, 1))
        r = c.routes
        g = poseref.I_VERTEX
        assert r.vertex[g] == 0 and r.length[g] == 0.0 and r.ids[r.offsets[g]:r.offsets[g + 1]].tolist() == [0, -1]
        assert np.array_equal(r.path(g), np.array([[30.0, 48.0], [30.0, 48.0]]))


@pytest.mark.parametrize("j", [1, 2, 63, 64, 65])
def test_trees_of_exactly_j_vertices(j):
    for star in (0, 1):
        w = poseref.stride_tree(j, star)
        poseref.check_stride_tree(w, j)
        c = prr.made_case(w)
        _check_case(c)
        assert (c.routes.vertex >= 0).sum() >= 2


def test_the_chain_of_1100_vertices_is_one_route_of_1101_rows():
    c = prr.long_chain()
    r = c.routes
    assert c.w.j == 1100 and r.vertex.tolist() == [1099, 1099, -1] and np.diff(r.offsets).tolist() == [1101, 1101, 0]
    assert r.ids[:1101].tolist() == list(range(1100)) + [-1]
    _check_case(c, libm=False)  # (straight unit legs but the last two: the libm comparison is the other tests')
    assert np.array_equal(bits(r.length[:2]), bits(r.cost[:2]))


@pytest.mark.parametrize("name", ["A", "E", "G256"])
def test_after_a_keep_on_a_changed_map(name):
    c = prr.kept_case(name)
    k = posekeepref.changed(name)
    assert 0 < k.alive.sum() < c.w.j and np.array_equal(c.vertex[:len(k.vertex)], k.vertex) and np.array_equal(bits(c.cost[:len(k.cost)]), bits(k.cost))
    assert (c.vertex >= 0).sum() >= 8
    _check_case(c)  # alive vertices only, every cell free on the NEW map, length == cost
