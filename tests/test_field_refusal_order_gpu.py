"""GPU: which refusal of rrt_batch_cost_field and rrt_batch_pose_field wins when a call is wrong in two ways, pinned against
tests/golden/field_refusal_order.json.

test_cost_field_gpu.py and test_pose_field_gpu.py hold every refusal sentence of the two calls, one wrong argument at a time.  This
module holds their order: each case is a call that two neighbouring refusals of the order would refuse, and the golden file has the
code and the full text of the one that does.  The order of both calls is

  the batch's kind  >  q out of range  >  an unfinished query  >  the grid replaced  >  the window's size  >  the window inside the grid
  >  a NULL output  >  (pose_field) the heading

and the rrt_plan_ forms refuse a NULL context and a context without a plan in front of all of it.  After the last case one valid call
on each batch answers what it answered before the first: a refusal changes nothing.

Three refusals stand in that order and are not here, because nothing outside the library can provoke them without corrupting a
descriptor or planning a tree of more than 2^18 poses: `query %d reports rho=%g, nh=%d` (pose_field, in front of the heading),
`query %d reports %d vertices, capacity %d` and POSE_FIELD_MAX_J's `query %d has %d vertices, at most %d` (behind everything).

The straight-line side is treecalls.wall_map() with 300 samples, the pose side posefieldcases.workload("E") with its 8 x 8 window.
Every context is a fresh one: the message of a replaced grid carries the context's grid generations.

The golden file is written by this module itself:  python tests/test_field_refusal_order_gpu.py --record"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # (--record runs without conftest.py)
    sys.path.insert(0, ROOT)

import oracle  # noqa: E402
import posefieldcases as pfc  # noqa: E402
import posefieldref  # noqa: E402
import poseref  # noqa: E402
import treecalls as tc  # noqa: E402
from posecalls import refused_with_golden_text  # noqa: E402
from rrtplanner_amd import _ffi, field, posefield  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "field_refusal_order.json")
N = 300


def _same(got, want):
    """the arrays of two answers, equal entry for entry; costs as raw bits"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.int64) if g.dtype == np.float64 else g, w.view(np.int64) if w.dtype == np.float64 else w)


def _side(refused, name, og8, window, straight, query, take, lib, extra=()):
    """The cases of one call.  refused(key, fn): fn() has to be refused; straight: the call is the straight-line one; query(): a query
    for a batch of the call's kind; take(handle, q or None, window, *heading): the module's call on a Batch or a Context; lib: the
    library with the call's prototypes; extra: (key, window, heading, NULL output or None) for the cases of a call with a heading."""
    W, H = og8.shape
    outside = (W - 3, 0, 4, 4)
    cells = window[2] * window[3]
    outs = [np.zeros(cells, dtype=t) for t in ((np.int32, np.float64) if straight else (np.int32, np.float64, np.int32))]
    ptrs = [a.ctypes.data for a in outs]
    heading = () if straight else (-1,)

    def raw(ctx, b, win, head, null):
        p = list(ptrs)
        if null is not None:
            p[null] = None
        _ffi._check(ctx.handle, getattr(lib, f"rrt_batch_{name}")(b._h, 0, *win, *head, *p))

    ctx = _ffi.Context(0)
    ctx.set_grid(og8)
    refused(f"{name}/plan/null_context+zero_window", lambda: _ffi._check(None, getattr(lib, f"rrt_plan_{name}")(None, 0, 0, 0, 0, *heading, *ptrs)))
    refused(f"{name}/plan/no_plan+zero_window", lambda: take(ctx, None, (0, 0, 0, 0)))
    other = _ffi.Batch(ctx, 1, N, dubins=straight)
    refused(f"{name}/kind+q", lambda: take(other, 5, window))
    other.close()
    b = _ffi.Batch(ctx, 2, N, dubins=not straight)
    refused(f"{name}/q+window_size", lambda: take(b, 2, (0, 0, 0, 5)))
    q, keep = query()
    b.set_query(0, q)
    refused(f"{name}/unfinished+window_outside", lambda: take(b, 0, outside))
    b.launch()
    b.sync()
    first = take(b, 0, window)
    refused(f"{name}/window_size+window_outside", lambda: take(b, 0, (-1, 0, 0, 5)))
    refused(f"{name}/window_outside+null", lambda: raw(ctx, b, outside, heading, 0))
    for key, win, head, null in extra:
        refused(f"{name}/{key}", lambda: raw(ctx, b, win, (head,), null))
    # the grid replaced: on a context and a batch of its own, so that the batch above keeps its tree
    ctx2 = _ffi.Context(0)
    ctx2.set_grid(og8)
    b2 = _ffi.Batch(ctx2, 1, N, dubins=not straight)
    b2.set_query(0, q)
    b2.launch()
    b2.sync()
    second = take(b2, 0, window)
    ctx2.set_grid(og8)
    refused(f"{name}/grid_replaced+zero_window", lambda: take(b2, 0, (0, 0, 0, 0)))
    ctx2.set_grid(np.zeros((W + 1, H), dtype=np.uint8))
    refused(f"{name}/grid_shape+zero_window", lambda: take(b2, 0, (0, 0, 0, 0)))
    ctx2.close()
    _same(second, first)
    _same(take(b, 0, window), first)
    ctx.close()
    return first


def _walk(refused):
    """every case of both calls in a fixed order; returns the two valid answers"""
    og = tc.wall_map()
    og8 = oracle.og_u8(og)
    samples = tc.free_samples(og, N, 17)
    line = _side(refused, "cost_field", og8, (0, 0, 8, 8), True, lambda: _ffi.make_query(1, N, (5, 5), (190, 150), samples, r2_rewire=900),
                 lambda handle, q, win: field.context_cost_field(handle, win) if q is None else field.batch_cost_field(handle, q, win), field._lib())
    w, window, f = pfc.workload("E")
    assert w.n == N and window[2:] == (8, 8)
    W, H = w.og8.shape
    poses = _side(refused, "pose_field", w.og8, window, False, lambda: poseref.device_query(w),
                  lambda handle, q, win: posefield.context_pose_field(handle, win) if q is None else posefield.batch_pose_field(handle, q, win),
                  posefield._lib(), extra=(("null+heading", window, w.nh, 2), ("window_outside+heading", (W - 3, 0, 4, 4), -2, None)))
    posefieldref.same(poses, posefieldref.answer(f, -1))
    return line, poses


def test_the_refusal_that_wins_is_the_recorded_one():
    with open(GOLDEN) as fh:
        golden = json.load(fh)
    seen = []

    def refused(key, fn):
        seen.append(key)
        refused_with_golden_text(golden, key, fn)

    _walk(refused)
    assert seen == list(golden) and len(seen) == 20


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_field_refusal_order_gpu.py --record")
    rec = {}

    def record(key, fn):
        try:
            fn()
        except _ffi.RRTError as e:
            prefix = f"librrt_hip error {e.code}: "
            assert str(e).startswith(prefix) and key not in rec
            rec[key] = [e.code, str(e)[len(prefix):]]
        else:
            sys.exit(f"{key}: not refused")

    _walk(record)
    with open(GOLDEN, "w") as fh:
        json.dump(rec, fh, indent=0, sort_keys=False)
        fh.write("\n")
    print(f"{GOLDEN}: {len(rec)} cases, library {_ffi.LIB_PATH}")
