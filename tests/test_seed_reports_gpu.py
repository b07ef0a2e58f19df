"""GPU: which report call answers after which seed call, and what every report call says when it refuses, pinned against
tests/golden/seed_reports.json.

A seed call replaces a query's tree and re-arms it: grow, reroot, relax on a straight-line batch, grow_poses, relax_poses, reroot_poses
on a Dubins batch.  The report calls (the _ms and _stats forms) answer for the last successful one only.  The module walks

  pairs    every ordered pair (first, second) of the three seed calls of a family, the query relaunched and synchronised in between, and
           after either call every report of the family: with its full count, and each _ms with count 0 and with one stage too many;
  refused  a second call that is refused (q out of range, root = j, a root that is not alive in a kept view): every report answers as
           it did after the first call;
  fresh    every report form of all nine families on a batch no tree call has touched, with a NULL out and a NULL handle too, and the
           rrt_plan_ forms on a context without a plan;
  once     keep_tree, cost_field, pose_routes and pose_shortcuts (with and without points) after one success: how many stages are read
           and how many trailing ones are exactly 0.0,

each through the rrt_batch_ forms on a batch and through the rrt_plan_ forms on a context's plan.  An entry is [return code, message]
of a refusal (and the context's own message behind it where that is another one: a NULL handle has no context to record it on), or of
a success how many values were written; of the stage times only whether each is > 0 or == 0.  No call here fails past its refusals:
the failures behind them are device-side ones, which are not provoked.

The shapes are the smallest that still have a tree to work on: a 32 x 32 grid with one short wall, n = 64, one query, RRT* and
Dubins-RRT* (rho 1.5, 8 headings) with r_rewire 6 on one CU, two samples per seed call.  The module takes about a second.

The golden file is written by this module itself:  python tests/test_seed_reports_gpu.py --record"""
import ctypes as C
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # (--record runs without conftest.py)
    sys.path.insert(0, ROOT)

from rrtplanner_amd import _ffi, field, hostprep, moving  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "seed_reports.json")
N, NH, RHO, M = 64, 8, 1.5, 2
R2 = hostprep.radius_threshold(6)
XS, XG, HS, HG = (4, 4), (27, 27), 0, 2
FORMS = ("rrt_batch_", "rrt_plan_")


def _maps():
    og = np.zeros((32, 32), dtype=np.uint8)
    og[14:16, 4:22] = 1  # one short wall: some samples are refused, so the tree leaves room to grow
    og2 = og.copy()  # the map a tree is kept on: another wall cuts part of it
    og2[22:24, 8:32] = 1
    return og, og2


OG, OG_CUT = _maps()
SAMPLES = hostprep.draw_free_samples(np.random.default_rng(0), np.argwhere(OG == 0), N)
HEADINGS = np.random.default_rng(100).integers(0, NH, size=N)
MORE = np.ascontiguousarray(hostprep.draw_free_samples(np.random.default_rng(5), np.argwhere((OG | OG_CUT) == 0), 4 * M), dtype=np.int32)
MORE_H = np.ascontiguousarray(np.concatenate([MORE, np.random.default_rng(6).integers(0, NH, size=(4 * M, 1))], axis=1), dtype=np.int32)
GOAL_POSES = np.array([XG + (HG,), (10, 10, 1), (20, 6, 5)], dtype=np.int32)

# the _ms forms: (stages of a full read, takes a count); the _stats forms write four counters
MS = {"keep_tree_ms": (3, False), "grow_ms": (3, True), "reroot_ms": (8, True), "relax_ms": (9, True), "relax_poses_ms": (9, True),
      "reroot_poses_ms": (10, True), "pose_routes_ms": (4, False), "pose_shortcuts_ms": (5, False), "cost_field_ms": (4, False)}
STATS = ("relax_stats", "relax_poses_stats", "reroot_poses_stats", "cost_field_stats")
SEEDS = {"line": ("grow", "reroot", "relax"), "poses": ("grow_poses", "relax_poses", "reroot_poses")}
REROOT = {"line": "reroot", "poses": "reroot_poses"}
REPORTS = {"line": ("grow_ms", "reroot_ms", "relax_ms", "relax_stats"),
           "poses": ("grow_ms", "relax_poses_ms", "relax_poses_stats", "reroot_poses_ms", "reroot_poses_stats")}
OWN = {"grow": {"grow_ms"}, "reroot": {"reroot_ms"}, "relax": {"relax_ms", "relax_stats"}, "grow_poses": {"grow_ms"},
       "relax_poses": {"relax_poses_ms", "relax_poses_stats"}, "reroot_poses": {"reroot_poses_ms", "reroot_poses_stats"}}
UNWRITTEN_MS, UNWRITTEN_STAT = -1.0, -7


def _lib():
    moving._lib()  # (the prototypes of the reroot_poses and cost_field symbols are declared by their modules)
    return field._lib()


def _refusal(s, rc):
    L = _lib()
    said, on_ctx = L.rrt_last_error_string(None).decode(), L.rrt_last_error_string(s.ctx.handle).decode()
    return [rc, said] if said == on_ctx else [rc, said, on_ctx]


def _read(s, name, count=None, out=True, handle=True, trailing=False):
    """one report call: its refusal, or how many values it wrote -- the buffer has room for more than any count asked for here -- and of
    stage times which are > 0 (+) and which == 0 (0), or with `trailing` only how many at the end are exactly 0.0"""
    fn = getattr(_lib(), s.form + name)
    if name in MS:
        stages, counted = MS[name]
        buf = (C.c_float * 16)(*([UNWRITTEN_MS] * 16))
        args = (stages if count is None else count,) if counted else ()
    else:
        buf, args = (C.c_int64 * 16)(*([UNWRITTEN_STAT] * 16)), ()
    rc = fn(s.h if handle else None, C.cast(buf, fn.argtypes[1]) if out else None, *args)
    if rc != _ffi.RRT_OK:
        return _refusal(s, rc)
    vals = list(buf)
    read = sum(1 for v in vals if v != (UNWRITTEN_MS if name in MS else UNWRITTEN_STAT))
    assert all(v == (UNWRITTEN_MS if name in MS else UNWRITTEN_STAT) for v in vals[read:]), (name, vals)
    if name not in MS:
        return {"read": read}
    assert all(v >= 0.0 for v in vals[:read]), (name, vals)
    signs = "".join("+" if v > 0.0 else "0" for v in vals[:read])
    return {"read": read, "trailing_zeros": len(signs) - len(signs.rstrip("0"))} if trailing else {"read": read, "signs": signs}


def _reports(s, names, probes=False, trailing=False):
    """every report of `names`: with its full count, each counted _ms with count 0 and with one stage too many; probes: with a NULL out
    and with a NULL handle too"""
    got = {}
    for name in names:
        got[name] = _read(s, name, trailing=trailing)
        if name in MS and MS[name][1]:
            got[name + "/count0"] = _read(s, name, 0)
            got[name + "/count+1"] = _read(s, name, MS[name][0] + 1)
        if probes:
            got[name + "/null_out"] = _read(s, name, out=False)
            got[name + "/null_handle"] = _read(s, name, handle=False)
    return got


def _build(family, form, planned=True):
    """a fresh context with the query of `family` planned on a batch of one query (rrt_batch_) or by rrt_plan (rrt_plan_)"""
    ctx = _ffi.Context(0)
    ctx.set_grid(OG)
    poses = family == "poses"
    if poses:
        query = _ffi.make_query(_ffi.ALG_DUBINS_STAR, N, XS + (HS,), XG + (HG,), SAMPLES, r2_rewire=R2, headings=HEADINGS, rho=RHO, nh=NH)
    else:
        query = _ffi.make_query(_ffi.ALG_STAR, N, XS, XG, SAMPLES, r2_rewire=R2)
    s = SimpleNamespace(ctx=ctx, family=family, form=form, b=None, h=ctx.handle, calls=0, res=_ffi.ResultArrays(N, headings=poses), query=query)
    if form == "rrt_batch_":
        # (no REWIRE, no LARGE_GRID: grow is allowed; one CU per query: a team's buffers take longer to allocate than a walk takes)
        s.b = _ffi.Batch(ctx, 1, N, team=1, dubins=poses)
        s.h = s.b._h
        if planned:
            s.b.set_query(0, query[0])
            _relaunch(s)
    elif planned:
        s.res = ctx.plan(query[0], N, team=1)[1]
    return s


def _relaunch(s):
    if s.b is not None:  # (an rrt_plan_ seed call launches and waits itself)
        s.b.launch()
        s.b.sync()


def _tree_size(s):
    if s.b is not None:
        return s.b.get_result(0, arrays=False).j
    j = C.c_int32(-1)
    assert _lib().rrt_plan_tree_size(s.h, C.byref(j)) == _ffi.RRT_OK
    return j.value


def _seed(s, name, q=0, root=1):
    """one seed call with the next two samples: its refusal, or its return code and j0"""
    L = _lib()
    at = M * (s.calls % 4)
    s.calls += 1
    rows = np.ascontiguousarray((MORE_H if s.family == "poses" else MORE)[at:at + M])
    lead = {"grow": (), "grow_poses": (), "reroot": (root,), "relax": (R2,), "relax_poses": (R2,), "reroot_poses": (root, R2)}[name]
    j0, log0, old_id = C.c_int32(-1), C.c_int32(-1), np.full(N + 1, -1, dtype=np.int32)
    if s.b is not None:
        rc = getattr(L, "rrt_batch_" + name)(s.h, q, *lead, rows.ctypes.data, M, C.byref(j0), old_id.ctypes.data, C.byref(log0))
    else:
        rc = getattr(L, "rrt_plan_" + name)(s.h, *lead, rows.ctypes.data, M, C.byref(j0), old_id.ctypes.data, C.byref(s.res.c))
    if rc not in (_ffi.RRT_OK, _ffi.RRT_E_GOAL_UNREACHABLE):  # (the latter: an rrt_plan_ call ran and its goal stayed out of reach)
        return _refusal(s, rc)
    return {"ok": rc, "j0": j0.value}


def _keep(s):
    if s.family == "poses":
        return s.b.keep_pose_tree(0) if s.b is not None else s.ctx.keep_pose_tree()
    return s.b.keep_tree(0) if s.b is not None else s.ctx.keep_tree()


def _walk_pair(family, form, first, second):
    s = _build(family, form)
    names = REPORTS[family]
    got = {"first": _seed(s, first)}
    got["after_first"] = _reports(s, names)
    if isinstance(got["first"], dict):
        _relaunch(s)
        got["second"] = _seed(s, second)
        got["after_second"] = _reports(s, names)
    s.ctx.close()
    return got


def _walk_refused(family, form, first):
    s = _build(family, form)
    names = REPORTS[family]
    got = {"first": _seed(s, first)}
    got["after_first"] = _reports(s, names)
    if isinstance(got["first"], dict):
        _relaunch(s)
        if s.b is not None:  # (an rrt_plan_ call has no q)
            for second in SEEDS[family]:
                got[f"{second}/qQ"] = _seed(s, second, q=1)
                got[f"{second}/qQ/reports"] = _reports(s, names)
        got["root=j"] = _seed(s, REROOT[family], root=_tree_size(s))
        got["root=j/reports"] = _reports(s, names)
        s.ctx.set_grid(OG_CUT)
        alive = _keep(s)
        dead = int(np.flatnonzero(~alive)[0]) if not alive.all() else -1
        got["kept"] = {"alive": int(alive.sum()), "of": len(alive), "dead": dead}
        got["root_dead"] = _seed(s, REROOT[family], root=dead)
        got["root_dead/reports"] = _reports(s, names)
    s.ctx.close()
    return got


def _walk_fresh(family, form, planned):
    s = _build(family, form, planned)
    got = _reports(s, list(MS) + list(STATS), probes=True)
    s.ctx.close()
    return got


def _walk_once(family, form):
    s = _build(family, form)
    got = {}
    if family == "line":
        got["keep_tree/alive"] = int(_keep(s).sum())
        got["keep_tree"] = _reports(s, ["keep_tree_ms"], trailing=True)
        window = (0, 0) + OG.shape
        vertex, _ = field.batch_cost_field(s.b, 0, window) if s.b is not None else field.context_cost_field(s.ctx, window)
        got["cost_field/connected"] = int((vertex >= 0).sum())
        got["cost_field"] = _reports(s, ["cost_field_ms", "cost_field_stats"], trailing=True)
    else:
        for shortcut in (False, True):
            for points in (False, True):
                out = s.b.pose_routes(0, GOAL_POSES, points, shortcut) if s.b is not None else s.ctx.pose_routes(GOAL_POSES, points, shortcut)
                key = ("pose_shortcuts" if shortcut else "pose_routes") + ("/points" if points else "")
                got[key + "/rows"] = int(out[3][-1])
                got[key] = _reports(s, ["pose_routes_ms", "pose_shortcuts_ms"], trailing=True)
    s.ctx.close()
    return got


def _cases():
    cases = {}
    for family in SEEDS:
        for form in FORMS:
            for first in SEEDS[family]:
                for second in SEEDS[family]:
                    cases[f"pairs/{family}/{form}/{first}/{second}"] = lambda a=(family, form, first, second): _walk_pair(*a)
                cases[f"refused/{family}/{form}/{first}"] = lambda a=(family, form, first): _walk_refused(*a)
            cases[f"fresh/{family}/{form}"] = lambda a=(family, form, True): _walk_fresh(*a)
            cases[f"once/{family}/{form}"] = lambda a=(family, form): _walk_once(*a)
    cases["fresh/line/rrt_plan_/no_plan"] = lambda: _walk_fresh("line", "rrt_plan_", False)
    return cases


CASES = _cases()
_want = {}


def _golden():
    if not _want:
        with open(GOLDEN) as f:
            _want.update(json.load(f))
    return _want


def _answers(entry):
    return isinstance(entry, dict)


def _holds(key, got):
    """what has to hold whatever the golden file says: [] or what does not"""
    wrong = []
    group, family = key.split("/")[:2]
    if group == "pairs":
        first, second = key.split("/")[3:]
        if not (_answers(got["first"]) and _answers(got.get("second"))):
            return [f"{key}: a seed call of the pair was refused"]
        for call, after in ((first, "after_first"), (second, "after_second")):
            for name in REPORTS[family]:  # exactly the reports of the last call answer
                if _answers(got[after][name]) != (name in OWN[call]):
                    wrong.append(f"{key}: {name} after {call}: {got[after][name]}")
                if name in OWN[call] and name in MS and (got[after][name]["read"] != MS[name][0] or "0" in got[after][name]["signs"]):
                    wrong.append(f"{key}: {name} after {call}: {got[after][name]}")
    if group == "refused":
        if not _answers(got["first"]) or "root_dead" not in got:
            return [f"{key}: the first call was refused"]
        for k, v in got.items():
            if k.endswith("/reports") and v != got["after_first"]:
                wrong.append(f"{key}: {k} differ from those after the first call")
            if k in ("root=j", "root_dead") or k.endswith("/qQ"):
                if _answers(v):
                    wrong.append(f"{key}: {k} was accepted")
        if "is not alive in the kept view" not in str(got["root_dead"]):
            wrong.append(f"{key}: root_dead: {got['kept']} {got['root_dead']}")
    if group == "fresh":
        wrong += [f"{key}: {k} answers" for k, v in got.items() if _answers(v)]
    if group == "once":
        wrong += [f"{key}: {k} has no answer" for k, v in got.items() if isinstance(v, dict) and not any(_answers(e) for e in v.values())]
    return wrong


@pytest.mark.parametrize("key", list(CASES))
def test_reports_are_the_recorded_ones(key):
    want = _golden()
    assert list(want) == list(CASES)
    got = json.loads(json.dumps(CASES[key]()))
    assert _holds(key, got) == []
    assert list(got) == list(want[key]), key
    differ = {k: (got[k], want[key][k]) for k in got if got[k] != want[key][k]}
    assert not differ, (key, dict(list(differ.items())[:3]))


def test_the_golden_file_has_refusals_and_answers_of_every_group():
    want = _golden()
    flat = [e for key, got in want.items() for v in got.values() for e in (v.values() if isinstance(v, dict) and "read" not in v and "ok" not in v else [v])]
    refused = sum(1 for e in flat if isinstance(e, list))
    answered = sum(1 for e in flat if isinstance(e, dict) and "read" in e)
    assert refused > 1000 and answered > 150, (refused, answered)
    for key, got in want.items():
        assert _holds(key, got) == [], key


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_seed_reports_gpu.py --record")
    rec, wrong, t0 = {}, [], time.perf_counter()
    for key, walk in CASES.items():
        t = time.perf_counter()
        rec[key] = json.loads(json.dumps(walk()))
        wrong += _holds(key, rec[key])
        print(f"{time.perf_counter() - t:6.3f} s  {key}")
    with open(GOLDEN, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=False)
        f.write("\n")
    print(f"{GOLDEN}: {len(rec)} cases in {time.perf_counter() - t0:.1f} s, library {_ffi.LIB_PATH}")
    if wrong:
        sys.exit("\n".join(["recorded, but:"] + wrong))
