"""CPU: the host restatement of the routes calls (routeref.py) on hand-written polylines and grids, and what RRT.routes_to decides
without the device.  The device side is tests/test_routes_gpu.py."""
import numpy as np
import pytest

import oracle
import orchelp
import routeref
from rrtplanner_amd import rrt as amd
from rrtplanner_amd.dubins import RRTDubins, RRTStarDubins


def _two_walls():
    """the map of the non-contiguous case: from s = (5, 50) the points A and C are visible, B and g are not; only C sees g"""
    og = np.zeros((200, 160), dtype=np.uint8)
    og[25:27, 0:41] = 1
    og[0:101, 60:62] = 1
    return og


S, A, B, C, G = (5, 50), (40, 50), (40, 20), (110, 30), (110, 80)


def test_the_visible_rows_need_not_be_contiguous():
    og8 = _two_walls()
    free = lambda p, q: oracle.collisionfree(og8, p, q)[0]  # noqa: E731
    assert [free(S, x) for x in (A, B, C, G)] == [True, False, True, False]
    assert [free(x, G) for x in (S, A, B, C)] == [False, False, False, True]
    rows = np.array([S, A, B, C, G])
    keep, tested = routeref.shortcut(og8, rows)
    assert keep == [0, 3, 4] and tested == 3  # (from s: B, C, g; from C the goal is the next row, untested)
    r, i, ln = routeref.polyline(og8, rows, [0, 1, 2, 3, -1], True)
    assert r.tolist() == [list(S), list(C), list(G)] and i.tolist() == [0, 3, -1]
    assert ln == float(np.sqrt(np.float64(105 * 105 + 20 * 20)) + np.sqrt(np.float64(50 * 50)))
    r, i, ln = routeref.polyline(og8, rows, [0, 1, 2, 3, -1], False)
    assert r.tolist() == rows.tolist() and i.tolist() == [0, 1, 2, 3, -1]
    assert ln == float(((np.float64(35.0) + np.float64(30.0)) + np.sqrt(np.float64(70 * 70 + 10 * 10))) + np.float64(50.0))


def test_a_polyline_blocked_everywhere_comes_back_unchanged():
    """a slalom round pillars: every row sees only its neighbours"""
    og8 = np.zeros((60, 30), dtype=np.uint8)
    rows = []
    for k in range(6):
        x = 5 + 10 * k  # a row below a pillar from the top, then one above a pillar from the bottom
        og8[x, (10 if k % 2 == 0 else 0):(30 if k % 2 == 0 else 20)] = 1
        rows.append((x, 5 if k % 2 == 0 else 25))
    rows = np.array(rows)
    for a in range(len(rows)):
        for b in range(a + 1, len(rows)):
            assert oracle.collisionfree(og8, rows[a], rows[b])[0] == (b == a + 1), (a, b)
    keep, tested = routeref.shortcut(og8, rows)
    assert keep == list(range(6)) and tested == 4 + 3 + 2 + 1
    r, i, ln = routeref.polyline(og8, rows, list(range(5)) + [-1], True)
    assert r.tolist() == rows.tolist() and ln == routeref.length(rows)


def test_an_open_polyline_becomes_one_leg():
    og8 = np.zeros((60, 30), dtype=np.uint8)
    rows = np.array([(1, 1), (10, 20), (20, 3), (30, 25), (50, 10)])
    assert routeref.shortcut(og8, rows) == ([0, 4], 3)
    assert routeref.polyline(og8, rows, [0, 4, 2, 9, -1], True)[1].tolist() == [0, -1]


def test_the_untested_neighbour_is_taken_even_if_its_line_is_blocked():
    """b == a + 1 is a tree edge or the goal edge: no line is walked for it, whatever the grid says"""
    og8 = np.zeros((20, 20), dtype=np.uint8)
    og8[5, :] = 1
    rows = np.array([(1, 1), (10, 1), (10, 10)])
    assert not oracle.collisionfree(og8, rows[0], rows[1])[0] and not oracle.collisionfree(og8, rows[0], rows[2])[0]
    assert routeref.shortcut(og8, rows) == ([0, 1, 2], 1)


def test_one_and_two_rows():
    og8 = np.zeros((20, 20), dtype=np.uint8)
    # k = 2: the goal hangs off the root; nothing to test
    assert routeref.shortcut(og8, np.array([(1, 1), (4, 5)])) == ([0, 1], 0)
    r, i, ln = routeref.polyline(og8, [(1, 1), (4, 5)], [0, -1], True)
    assert r.tolist() == [[1, 1], [4, 5]] and i.tolist() == [0, -1] and ln == 5.0
    # k = 1 cannot come out of a tree (a route has the root and the goal), but the pass takes it: the row, no leg
    assert routeref.shortcut(og8, np.array([(1, 1)])) == ([0], 0)
    assert routeref.polyline(og8, [(1, 1)], [0], True)[2] == 0.0
    # the goal ON the start: two rows with the same point, length 0
    pts, parent, vcost = np.array([(3, 3), (9, 9)]), np.array([-1, 0]), np.array([0.0, np.sqrt(72.0)])
    v, c, ln, off, xy, ids = routeref.routes(og8, pts, vcost, parent, 2, [(3, 3)], cut=True)
    assert (v.tolist(), c.tolist(), ln.tolist(), off.tolist()) == ([0], [0.0], [0.0], [0, 2])
    assert xy.tolist() == [[3, 3], [3, 3]] and ids.tolist() == [0, -1]


def test_routes_over_a_small_tree():
    og8 = _two_walls()
    pts = np.array([S, A, B, C, (0, 0)])
    parent = np.array([-1, 0, 1, 2, 7])
    vcost = np.array([0.0, 35.0, 65.0, 65.0 + np.sqrt(np.float64(5000)), 0.0])
    goals = [G, (25, 10), A, (199, 159)]  # behind both walls; on a wall; a vertex itself; the far corner
    for cut in (False, True):
        v, c, ln, off, xy, ids = routeref.routes(og8, pts, vcost, parent, 4, goals, cut=cut)
        assert v.tolist() == [3, -1, 0, 3] and c[1] == np.inf and ln[1] == np.inf
        assert v.dtype == np.int32 and off.dtype == np.int64 and xy.dtype == np.int32 and ids.dtype == np.int32
        assert off.tolist() == ([0, 3, 3, 5, 8] if cut else [0, 5, 5, 7, 12])
        assert xy[off[2]:off[3]].tolist() == [list(S), list(A)] and ids[off[2]:off[3]].tolist() == [0, -1] and ln[2] == 35.0
        if cut:
            assert xy[:3].tolist() == [list(S), list(C), list(G)] and ids[:3].tolist() == [0, 3, -1]
            assert np.all(ln[[0, 3]] < c[[0, 3]])
        else:
            assert ids[:5].tolist() == [0, 1, 2, 3, -1] and ln[0] == c[0]
    with pytest.raises(AssertionError, match="vertex 0"):
        routeref.raw_route(pts, np.array([-1, 2, 1, 2, 0]), 3, G)  # a cycle 1 <-> 2


def test_routes_to_needs_a_tree_on_the_device():
    og = np.zeros((64, 48), dtype=np.int64)
    p = amd.RRTStar(og, 300, 12, pbar=False)
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.routes_to([(5, 5)])
    p = orchelp.use_oracle(amd.RRTStar(og, 300, 12, pbar=False, seed=0))
    p.plan(np.array((3, 3)), np.array((55, 40)))
    with pytest.raises(ValueError, match="outside"):
        p.routes_to([(64, 0)], shortcut=True)
    p.set_n(300)
    with pytest.raises(RuntimeError, match="plan\\(\\) first"):
        p.routes_to([(5, 5)], shortcut=True)
    p = amd.RRTStar(og, 50, 12, costfn=lambda vc, pts, v, x: vc[v] + 1.0, pbar=False)
    p._tree_resident = "host"
    with pytest.raises(ValueError, match="host route"):
        p.routes_to([(5, 5)])
    for cls in (RRTDubins, RRTStarDubins):
        d = cls(og, 100, 3.0, pbar=False) if cls is RRTDubins else cls(og, 100, 20, 3.0, pbar=False)
        with pytest.raises(ValueError, match="Dubins"):
            d.routes_to([(5, 5)], shortcut=True)
