"""No GPU: what the host restatement of the pose shortcuts (poseshortref.py) must satisfy whatever the kernel does, and what makes the
workloads of test_pose_shortcuts_gpu.py worth running.

The properties are checked against the oracle's own sweep cells (oracle.dub_sweep_cells), evaluated here and not through
poseref.sweep_free, which the restatement uses.  The conditions were measured before they were written down: routes shortened
A 13 of 26, B 9 of 27, C 14 of 19, D 7 of 29, E 13 of 32, kept A 14 of 24, kept C 14 of 19, kept E 19 of 28; anchors that take a tested
candidate after a farther one was blocked, at least 8 (D); anchors that find every candidate blocked, at least 17 (kept E); the rings
80, 45, 11, 1 and 202, 153, 103, 55, 7, 1 blocked candidates in front of the kept rows of their longest route."""
import math

import numpy as np
import pytest

import oracle
import poseref
import poseroutesref as prr
import poseshortref as psr

CASES = {
    **{name: (lambda name=name: prr.case(name)) for name in "ABCDE"},
    **{"kept " + name: (lambda name=name: prr.kept_case(name)) for name in "ACE"},
    "ring small": lambda: psr.ring("small"),
    "ring large": lambda: psr.ring("large"),
    "half-cell chain": prr.half_cell_chain,
}
PERLIN = [name for name in CASES if len(name) == 1 or name.startswith("kept")]


def _free_by_cells(og8, a, b, rho, nh):
    """the sweep of the shortest word a -> b by the oracle's cells: every cell inside the grid and free, then b's cell"""
    args = (float(a[0]), float(a[1]), poseref.theta(a[2], nh), float(b[0]), float(b[1]), poseref.theta(b[2], nh), float(rho))
    length = oracle.dub_shortest(*args)[3]
    if not math.isfinite(length):
        return False
    cells = oracle.dub_sweep_cells(a[0], a[1], poseref.theta(a[2], nh), b[0], b[1], poseref.theta(b[2], nh), rho, cap=int(length / 0.5) + 16)
    assert len(cells) == int(length / 0.5) + 1
    W, H = og8.shape
    for x, y in cells.tolist():
        if not (0 <= x < W and 0 <= y < H) or og8[x, y] != 0:
            return False
    return og8[b[0], b[1]] == 0


@pytest.mark.parametrize("name", list(CASES))
def test_the_restatement_is_the_greedy_pass(name):
    c = CASES[name]()
    w, raw, r = c.w, c.routes, psr.of_case(c)
    assert r.raw is raw and np.array_equal(r.vertex, raw.vertex) and np.array_equal(r.cost.view(np.int64), raw.cost.view(np.int64))
    for g in range(len(c.goals)):
        if raw.vertex[g] < 0:
            assert r.offsets[g + 1] == r.offsets[g] and r.point_offsets[g + 1] == r.point_offsets[g] and r.length[g] == np.inf
            continue
        poses = [tuple(int(x) for x in p) for p in raw.route(g)]
        ids = raw.ids[raw.offsets[g]:raw.offsets[g + 1]]
        kept = r.kept_rows[g]
        k = len(poses)
        # a subsequence of the raw rows with their ids, the first and the goal row among them
        assert kept[0] == 0 and kept[-1] == k - 1 and all(x < y for x, y in zip(kept[:-1], kept[1:]))
        assert np.array_equal(r.route(g), np.array([poses[i] for i in kept])) and np.array_equal(r.ids[r.offsets[g]:r.offsets[g + 1]], ids[kept])
        assert r.ids[r.offsets[g + 1] - 1] == -1
        for a, b in zip(kept[:-1], kept[1:]):
            assert _free_by_cells(c.og8, poses[a], poses[b], w.rho, w.nh), (name, g, a, b)  # the untested successor, too
            for far in range(b + 1, k):
                assert not _free_by_cells(c.og8, poses[a], poses[far], w.rho, w.nh), (name, g, a, b, far)
        # the margin covers the rounding of up to 251 f64 additions on either side and nothing else
        assert r.length[g] <= raw.length[g] * (1 + 1e-9), (name, g, r.length[g], raw.length[g])
        # the path: per kept leg its samples, then the goal cell; every point rounds to a free cell of the active map
        p = r.path(g)
        cells = np.floor(p + 0.5).astype(np.int64)
        assert np.all(c.og8[cells[:, 0], cells[:, 1]] == 0) and tuple(p[-1]) == (float(poses[-1][0]), float(poses[-1][1]))
        assert len(p) == sum(n for _, n in r.legs_of(g)) + 1


@pytest.mark.parametrize("name", ["A", "kept E", "half-cell chain"])
def test_without_shortcuts_it_is_the_raw_restatement(name):
    c = CASES[name]()
    w = c.w
    got = psr.routes(w.ro.pts, w.ro.head, w.ro.parent, w.j, c.goals, c.vertex, c.cost, w.rho, w.nh, c.og8, shortcut=False)
    for field in ("vertex", "cost", "length", "offsets", "rows", "ids", "point_offsets", "points"):
        x, y = getattr(got, field), getattr(c.routes, field)
        assert x.dtype == y.dtype and np.array_equal(x.view(np.int64) if x.dtype == np.float64 else x, y.view(np.int64) if y.dtype == np.float64 else y), field
    again = psr.routes(w.ro.pts, w.ro.head, w.ro.parent, w.j, c.goals, c.vertex, c.cost, w.rho, w.nh, c.og8)
    prr.same((again.vertex, again.cost, again.length, again.offsets, again.rows, again.ids, again.point_offsets, again.points), psr.of_case(c))


# ---- what keeps a comparison on the GPU from being empty
@pytest.mark.parametrize("name", PERLIN)
def test_the_workloads_shorten_routes_and_meet_blocked_candidates(name):
    connected, shortened, past, none, _ = psr.counts(psr.of_case(CASES[name]()))
    assert 5 * shortened >= connected > 0, (name, shortened, connected)
    assert past >= 5, (name, past)    # a tested winner behind a blocked farther candidate: the sweep loop goes on past a failure
    assert none >= 10, (name, none)   # every candidate blocked: the untested successor is taken


def test_the_rings_reach_the_second_third_and_fourth_batch_of_candidates():
    for name, vertices, need, longest in (("small", 150, 65, 116), ("large", 300, 129, 251)):
        c = psr.ring(name)
        w = c.w
        assert w.j == w.n == vertices and np.all(w.ro.parent[1:w.j] == np.arange(w.j - 1))  # one chain
        assert w.vertex[4] == -1 and (w.vertex[:4] >= 0).all()  # the centre cell lies on the disc
        r = psr.of_case(c)
        assert int(np.diff(c.routes.offsets).max()) == longest
        connected, shortened, past, none, most = psr.counts(r)
        assert shortened == connected == 4 and most >= need, (name, most)
        # a winner in the middle of a batch of 64, and one in its first lane (no candidate blocked before it) is not all there is
        mids = [blocked % 64 for anchors in r.anchors for a, b, blocked, cands in anchors if b > a + 1]
        assert any(0 < x < 63 for x in mids), mids
    blocked = [x[2] for x in psr.of_case(psr.ring("large")).anchors[0]]
    assert max(blocked) >= 3 * 64 and sorted(x // 64 for x in blocked if x >= 64) == [1, 2, 3], blocked  # batches two, three and four


def test_the_half_cell_chain_has_a_shortcut_leg_with_a_duplicate_point():
    c = prr.half_cell_chain()
    r = psr.of_case(c)
    w = c.w
    connected, shortened, _, _, _ = psr.counts(r)
    assert connected == shortened == 2
    exact = 0
    for g in range(2):
        rows = r.route(g)
        legs = r.legs_of(g)
        for (a, b), (at, n) in zip(zip(rows[:-1], rows[1:]), legs):
            length = prr.leg(tuple(a), tuple(b), w.rho, w.nh)[0]
            if length > 4.0 and length == math.floor(length / 0.5) * 0.5:  # longer than a tree leg: a shortcut
                exact += 1
                assert n == int(length / 0.5) + 1
                assert np.array_equal(r.points[at + n - 1], r.points[at + n])  # its last sample IS the next leg's first point
    assert exact >= 1


# ---- the interface, as far as it shows without a device
def test_the_symbols_and_the_keyword_are_there():
    import inspect
    import json
    import os

    from rrtplanner_amd import RRTStar, _ffi
    from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins

    for name in ("rrt_batch_pose_shortcuts", "rrt_batch_pose_shortcuts_ms", "rrt_plan_pose_shortcuts", "rrt_plan_pose_shortcuts_ms"):
        assert name in _ffi.SYMBOLS, name
    for fn in (_ffi.Batch.pose_routes, _ffi.Context.pose_routes, RRTDubins.routes_to_poses, RRTStarDubins.routes_to_poses, RRTStar.routes_to_poses):
        assert inspect.signature(fn).parameters["shortcut"].default is False, fn
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_shortcuts_refusals.json")) as f:
        golden = json.load(f)
    w = poseref.workload("E")
    with pytest.raises(ValueError) as e:  # the straight-line planners take the keyword and refuse with the text they had
        RRTStar(w.og, 50, 10, pbar=False).routes_to_poses(w.goals, shortcut=True)
    assert str(e.value) == golden["straight_line_planner"][1]
