"""GPU: every refusal of the calls that work on a finished tree (connect_goals, connect_poses, routes, keep_tree, grow, their
rrt_plan_* forms and their small companions), code and full message, pinned against tests/golden/tree_call_refusals.json.

The module walks a fixed list of states of a batch and of the context's rrt_plan batch; in each state it makes a fixed list of calls,
each with a good argument, with each bad one, and with every pair of a bad q and a bad payload, and records the code and the message
of the refusal, or "ok".  A call that is wrong in two ways has to be refused for the same reason as when the golden file was
written.  Every call here succeeds or is refused on the host.

The golden file is written by this module itself:  python tests/test_tree_call_refusals_gpu.py --record"""
import ctypes as C
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # (--record runs without conftest.py)
    sys.path.insert(0, ROOT)

from rrtplanner_amd import _ffi, hostprep  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "tree_call_refusals.json")
N, Q, NH = 300, 1, 16
BIG = (1 << 20) + 1
XS, XG = (5, 5), (40, 40)
STATES = ("no_query", "set_not_launched", "finished", "rearmed", "grid_replaced", "grid_other_shape", "kept", "kept_root_blocked",
          "informed_waits", "dubins", "rewire", "large_grid", "no_plan")
FLAGS = {"dubins": dict(dubins=True), "rewire": dict(rewire=True), "large_grid": dict(large_grid=True)}


def _maps():
    og = np.zeros((64, 64), dtype=np.uint8)
    og[30:33, :] = 1  # a wall with one gap: some samples are refused, so the tree leaves room to grow
    og[30:33, 40:50] = 0
    og[10:20, 10:14] = 1
    og2 = og.copy()  # the map a tree is kept on: another wall cuts part of it
    og2[45:48, 0:40] = 1
    og3 = og2.copy()  # ... and with the root blocked
    og3[XS[0], XS[1]] = 1
    return og, og2, og3, np.zeros((48, 48), dtype=np.uint8)


OG, OG_KEPT, OG_ROOT, OG_OTHER = _maps()
SAMPLES = hostprep.draw_free_samples(np.random.default_rng(18), np.argwhere(OG == 0), N)
HEADINGS = np.random.default_rng(19).integers(0, NH, size=N)

GOOD = np.array([(5, 5), (40, 40), (20, 20), (60, 60), (50, 10), (31, 5)], dtype=np.int32)
OUTSIDE = GOOD.copy()
OUTSIDE[2] = (64, 5)
GOOD_H = np.array([0, 3, 5, 15, 8, 1], dtype=np.int32)
_bufs = {}


def _buffers():
    """arguments and outputs of the calls, allocated once.  The outputs have room for BIG goals: a call that should have been refused
    and was not writes inside them."""
    if not _bufs:
        big = np.zeros((BIG, 3), dtype=np.int32)
        poses = lambda xy, h: np.ascontiguousarray(np.concatenate([xy, h[:, None]], axis=1), dtype=np.int32)  # noqa: E731
        bad_h = GOOD_H.copy()
        bad_h[1] = NH
        _bufs.update(
            goals=dict(good=GOOD, too_many=big[:, :2].copy(), outside=OUTSIDE, null=None),
            poses=dict(good=poses(GOOD, GOOD_H), too_many=big, outside=poses(OUTSIDE, GOOD_H), bad_heading=poses(GOOD, bad_h),
                       heading_then_outside=poses(np.concatenate([GOOD[:3], [(5, -1)], GOOD[4:]]), bad_h), null=None),
            vertex=np.zeros(BIG, dtype=np.int32), cost=np.zeros(BIG), length=np.zeros(BIG), offsets=np.zeros(BIG + 1, dtype=np.int64),
            xy=np.zeros((4096, 2), dtype=np.int32), ids=np.zeros(4096, dtype=np.int32), alive=np.zeros(N + 1, dtype=np.uint8),
            old_id=np.zeros(N + 1, dtype=np.int32), big=big)
    return _bufs


def _query(state):
    if state == "dubins":
        return _ffi.make_query(_ffi.ALG_DUBINS_STAR, N, XS + (0,), XG + (3,), SAMPLES, r2_rewire=400, headings=HEADINGS, rho=3.0, nh=NH)
    if state == "informed_waits":
        return _ffi.make_query(_ffi.ALG_INFORMED, N, XS, XG, SAMPLES, r2_rewire=400, goal_d2=900,
                               Cmat=hostprep.rotation_to_world_frame(np.array(XS), np.array(XG)))
    return _ffi.make_query(_ffi.ALG_STAR, N, XS, XG, SAMPLES, r2_rewire=400)


def _build(state):
    """a fresh context (the messages carry its grid generation) with a batch in `state`, and the same state behind rrt_plan where
    rrt_plan can reach it.  .j: the vertices a grow would start from, None without a finished tree."""
    ctx = _ffi.Context(0)
    ctx.set_grid(OG)
    s = SimpleNamespace(ctx=ctx, b=None, j=None)
    if state == "no_plan":
        return s
    kw = FLAGS.get(state, {})
    s.b = b = _ffi.Batch(ctx, Q, N, **kw)
    if state == "no_query":
        return s
    qu, keep = _query(state)
    b.set_query(0, qu)
    if state == "set_not_launched":
        return s
    b.launch()
    b.sync()
    res = b.get_result(0, arrays=False)
    if state == "rearmed":
        b.rearm()
        return s
    rc, _ = ctx.plan(qu, N, **{k: v for k, v in kw.items() if k != "dubins"})
    if state == "informed_waits":
        assert res.status == _ffi.RRT_NEED_UNITBALL and rc == _ffi.RRT_NEED_UNITBALL
        return s
    assert res.status == _ffi.RRT_OK and rc == _ffi.RRT_OK and 10 < res.j < N - 10, (res.status, rc, res.j)
    s.j = res.j
    if state == "grid_replaced":
        ctx.set_grid(OG)
    elif state == "grid_other_shape":
        ctx.set_grid(OG_OTHER)
    elif state in ("kept", "kept_root_blocked"):
        ctx.set_grid(OG_KEPT if state == "kept" else OG_ROOT)
        s.j = int(b.keep_tree(0).sum())
        assert int(ctx.keep_tree().sum()) == s.j and (0 < s.j < res.j if state == "kept" else s.j == 0)
    return s


def _ptr(a):
    return None if a is None else a.ctypes.data


def _len(a):
    return len(GOOD) if a is None else len(a)


def _calls(s):
    """the fixed list: (key, changes the state if accepted, thunk -> return code).  Batch calls first, then the rrt_plan_* forms."""
    L, B = _ffi.lib(), _buffers()
    h, bh = s.ctx.handle, (s.b._h if s.b is not None else None)
    vertex, cost, length, offsets = (_ptr(B[k]) for k in ("vertex", "cost", "length", "offsets"))
    n_alive, j0, log0, tree_j = C.c_int32(-1), C.c_int32(-1), C.c_int32(-1), C.c_int32(-1)
    ms, counts = (C.c_float * 3)(), (C.c_int64 * 2)()
    res = _ffi.ResultArrays(N)
    room = N + 1 if s.j is None else N - s.j + 1
    grown = dict(good=np.ascontiguousarray(SAMPLES[:5], dtype=np.int32), outside=OUTSIDE, beyond_room=B["big"][:room, :2].copy(),
                 too_many=B["goals"]["too_many"], null=None)
    qs = (("q0", 0), ("q-1", -1), ("qQ", Q))
    out = []

    def rows(extra=0):  # the rows the last accepted routes call left (0 after a refused one), or one more
        r = int(B["offsets"][len(GOOD)]) if s.rows_known else 0
        assert 0 <= r < 4096
        return _ptr(B["xy"]), _ptr(B["ids"]), r + extra

    if bh is not None:
        for qn, q in qs:
            for pn, g in B["goals"].items():
                out.append((f"rrt_batch_connect_goals/{qn}/{pn}", False,
                            lambda q=q, g=g: L.rrt_batch_connect_goals(bh, q, _ptr(g), _len(g), vertex, cost)))
        for qn, q in qs:
            for pn, g in B["poses"].items():
                out.append((f"rrt_batch_connect_poses/{qn}/{pn}", False,
                            lambda q=q, g=g: L.rrt_batch_connect_poses(bh, q, _ptr(g), _len(g), vertex, cost)))
        out.append(("rrt_batch_connect_poses_counts", False, lambda: L.rrt_batch_connect_poses_counts(bh, C.byref(counts))))
        out.append(("rrt_batch_routes_rows/before", False, lambda: L.rrt_batch_routes_rows(bh, _ptr(B["xy"]), _ptr(B["ids"]), 0)))
        for qn, q in qs:
            for pn, g in B["goals"].items():
                for fn_, flags in (("", 0), ("/shortcut", 1), ("/bad_flags", 2)):
                    if fn_ and pn not in ("good", "outside"):
                        continue
                    key = f"rrt_batch_routes/{qn}/{pn}{fn_}"

                    def routes(q=q, g=g, flags=flags, key=key):
                        rc = L.rrt_batch_routes(bh, q, _ptr(g), _len(g), flags, vertex, cost, length, offsets)
                        s.rows_known = rc == 0
                        return rc
                    out.append((key, False, routes))
                    if pn == "good" and qn == "q0":
                        out.append((f"{key}/rows", False, lambda: L.rrt_batch_routes_rows(bh, *rows())))
                        out.append((f"{key}/rows+1", False, lambda: L.rrt_batch_routes_rows(bh, *rows(1))))
        out.append(("rrt_batch_routes_rows/after", False, lambda: L.rrt_batch_routes_rows(bh, _ptr(B["xy"]), _ptr(B["ids"]), 0)))
        for qn, q in qs:
            out.append((f"rrt_batch_keep_tree/{qn}", q == 0, lambda q=q: L.rrt_batch_keep_tree(bh, q, C.byref(n_alive), _ptr(B["alive"]))))
        out.append(("rrt_batch_keep_tree/q-1/null", False, lambda: L.rrt_batch_keep_tree(bh, -1, None, _ptr(B["alive"]))))
        out.append(("rrt_batch_keep_tree_ms", False, lambda: L.rrt_batch_keep_tree_ms(bh, C.byref(ms))))
        for qn, q in qs:
            for pn, g in grown.items():
                out.append((f"rrt_batch_grow/{qn}/{pn}", q == 0 and pn == "good", lambda q=q, g=g: L.rrt_batch_grow(
                    bh, q, _ptr(g), _len(g), C.byref(j0), _ptr(B["old_id"]), C.byref(log0))))
        out.append(("rrt_batch_grow_ms", False, lambda: L.rrt_batch_grow_ms(bh, C.byref(ms), 3)))
        out.append(("rrt_batch_grow_ms/count4", False, lambda: L.rrt_batch_grow_ms(bh, C.byref(ms), 4)))
    for pn, g in B["goals"].items():
        out.append((f"rrt_plan_connect_goals/{pn}", False, lambda g=g: L.rrt_plan_connect_goals(h, _ptr(g), _len(g), vertex, cost)))
    for pn, g in B["poses"].items():
        out.append((f"rrt_plan_connect_poses/{pn}", False, lambda g=g: L.rrt_plan_connect_poses(h, _ptr(g), _len(g), vertex, cost)))
    out.append(("rrt_plan_routes_rows/before", False, lambda: L.rrt_plan_routes_rows(h, _ptr(B["xy"]), _ptr(B["ids"]), 0)))
    for pn, g in B["goals"].items():
        for fn_, flags in (("", 0), ("/bad_flags", 2)):
            def plan_routes(g=g, flags=flags):
                rc = L.rrt_plan_routes(h, _ptr(g), _len(g), flags, vertex, cost, length, offsets)
                s.rows_known = rc == 0
                return rc
            out.append((f"rrt_plan_routes/{pn}{fn_}", False, plan_routes))
            if pn == "good" and not fn_:
                out.append(("rrt_plan_routes/good/rows", False, lambda: L.rrt_plan_routes_rows(h, *rows())))
                out.append(("rrt_plan_routes/good/rows+1", False, lambda: L.rrt_plan_routes_rows(h, *rows(1))))
    out.append(("rrt_plan_routes_rows/after", False, lambda: L.rrt_plan_routes_rows(h, _ptr(B["xy"]), _ptr(B["ids"]), 0)))
    out.append(("rrt_plan_tree_size", False, lambda: L.rrt_plan_tree_size(h, C.byref(tree_j))))
    out.append(("rrt_plan_keep_tree", True, lambda: L.rrt_plan_keep_tree(h, C.byref(n_alive), _ptr(B["alive"]))))
    out.append(("rrt_plan_keep_tree/null", False, lambda: L.rrt_plan_keep_tree(h, None, _ptr(B["alive"]))))
    out.append(("rrt_plan_keep_tree_ms", False, lambda: L.rrt_plan_keep_tree_ms(h, C.byref(ms))))
    for pn, g in grown.items():
        out.append((f"rrt_plan_grow/{pn}", pn == "good",
                    lambda g=g: L.rrt_plan_grow(h, _ptr(g), _len(g), C.byref(j0), _ptr(B["old_id"]), C.byref(res.c))))
    out.append(("rrt_plan_grow_ms", False, lambda: L.rrt_plan_grow_ms(h, C.byref(ms), 3)))
    return out


def _outcome(s, rc):
    if rc in (_ffi.RRT_OK, _ffi.RRT_E_GOAL_UNREACHABLE):  # (the latter: rrt_plan_grow ran and its goal stayed out of reach)
        return "ok" if rc == _ffi.RRT_OK else f"ok:{rc}"
    return [rc, _ffi.lib().rrt_last_error_string(s.ctx.handle).decode()]


def _walk(state):
    """{key: outcome} of one state.  First every call that leaves the state as it is, accepted or not; then the first good
    connect_goals again, which has to give the arrays it gave before all the refusals; then the calls that change the state when they
    are accepted, each on a state built anew, followed by the timing call that goes with it."""
    B = _buffers()
    got = {}
    s = _build(state)
    s.rows_known = False
    calls = _calls(s)
    first = None
    for key, changes, call in calls:
        if changes:
            continue
        got[key] = _outcome(s, call())
        if first is None and key == "rrt_batch_connect_goals/q0/good" and got[key] == "ok":
            first = (B["vertex"][:len(GOOD)].copy(), B["cost"][:len(GOOD)].copy())
    if first is not None:
        key, _, call = calls[0]
        assert key == "rrt_batch_connect_goals/q0/good" and _outcome(s, call()) == "ok"
        assert np.array_equal(first[0], B["vertex"][:len(GOOD)]) and np.array_equal(first[1].view(np.int64), B["cost"][:len(GOOD)].view(np.int64))
    follow = {"rrt_batch_keep_tree/q0": "rrt_batch_keep_tree_ms", "rrt_plan_keep_tree": "rrt_plan_keep_tree_ms",
              "rrt_batch_grow/q0/good": "rrt_batch_grow_ms", "rrt_plan_grow/good": "rrt_plan_grow_ms"}
    for key in [k for k, changes, _ in calls if changes]:
        by_key = {k: c for k, _, c in calls}
        got[key] = _outcome(s, by_key[key]())
        got[f"{key}/then/{follow[key]}"] = _outcome(s, by_key[follow[key]]())
        if isinstance(got[key], list):  # refused: the state is what it was
            continue
        s.ctx.close()
        s = _build(state)
        s.rows_known = False
        calls = _calls(s)
    s.ctx.close()  # (the batch with it)
    return got


def _walk_all():
    return {state: _walk(state) for state in STATES}


def test_every_refusal_is_the_recorded_one():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = json.loads(json.dumps(_walk_all()))
    assert list(got) == list(want)
    for state in STATES:
        assert list(got[state]) == list(want[state]), state
        differ = {k: (got[state][k], want[state][k]) for k in got[state] if got[state][k] != want[state][k]}
        assert not differ, (state, dict(list(differ.items())[:5]))
    refused = sum(1 for st in want.values() for v in st.values() if isinstance(v, list))
    accepted = sum(1 for st in want.values() for v in st.values() if not isinstance(v, list))
    assert refused > 1000 and accepted > 50, (refused, accepted)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_tree_call_refusals_gpu.py --record")
    rec = _walk_all()
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"{GOLDEN}: {sum(len(v) for v in rec.values())} calls in {len(rec)} states, library {_ffi.LIB_PATH}")
