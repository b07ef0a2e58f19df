"""The cost-to-come field: every cell of the map connected to the finished tree (include/rrt_hip_field.h, rrt_field.h).

connect_goals answers for the goals the caller lists.  cost_field answers for the whole grid, or a window of it: per cell the cost from
the start and the tree vertex to enter the tree at -- what connect_goals gives for that one cell, entry for entry and bit for bit.  With
the tree planned from the goal it is a feedback policy for a robot that may be anywhere; it is also the table to pick from when the
goal is "any cell of this region".  The vertices are bucketed once per call and a cell looks only at the buckets that can still beat what
it has found, so a field costs a small fraction of the same cells sent through connect_goals.

The module binds its six symbols itself, on the handle _ffi.lib() returns, through the binder moving.py and posefield.py use too
(_ffi._side_binding): the signature table of _ffi and the methods of Context, Batch and the planner classes are a recorded surface.

  cost_field(planner, window=None)               the field of the tree of planner's last plan(); window (x0, y0, w, h), None: the grid
  batch_cost_field(batch, q, window)             rrt_batch_cost_field
  context_cost_field(ctx, window)                rrt_plan_cost_field
  cost_field_ms(handle), cost_field_stats(handle)  the stage times and the counters of the last call on a Batch or a Context"""
import ctypes as C

import numpy as np

from . import _ffi

FIELD_STATS = ("cells", "buckets", "priced", "los")

_vp, _i32, _i64, _P = C.c_void_p, C.c_int32, C.c_int64, C.POINTER
_PROTOTYPES = {
    "rrt_batch_cost_field": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp],
    "rrt_plan_cost_field": [_vp, _i32, _i32, _i32, _i32, _vp, _vp],
    "rrt_batch_cost_field_ms": [_vp, _P(C.c_float * 4)],
    "rrt_plan_cost_field_ms": [_vp, _P(C.c_float * 4)],
    "rrt_batch_cost_field_stats": [_vp, _P(_i64 * 4)],
    "rrt_plan_cost_field_stats": [_vp, _P(_i64 * 4)],
}
_lib, _tree_of = _ffi._side_binding(_PROTOTYPES)


def _window(window):
    """(x0, y0, w, h) as four ints"""
    try:
        x0, y0, w, h = (int(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"window must be (x0, y0, w, h), got {window!r}") from None
    return x0, y0, w, h


def _planner_window(who, planner, window):
    """the window of a planner-level field call, `who`, as four ints: None is the whole grid, anything else has to lie inside it"""
    W, H = np.asarray(planner.og).shape
    x0, y0, w, h = (0, 0, W, H) if window is None else _window(window)
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError(f"{who}: the window ({x0}, {y0}) + {w} x {h} does not lie inside the {W}x{H} occupancy grid")
    return x0, y0, w, h


def _answers(window, kinds):
    """(window as four ints, one (w, h) array per (dtype, fill) of kinds); the arrays are sized by the window asked for, which the
    library checks against its grid before it writes any"""
    x0, y0, w, h = _window(window)
    return (x0, y0, w, h), [np.full((max(w, 0), max(h, 0)), fill, dtype=dtype) for dtype, fill in kinds]


def _field(tree, window):
    """the call on a _Tree: (vertex int32 (w, h), cost float64 (w, h))"""
    win, (vertex, cost) = _answers(window, ((np.int32, -1), (np.float64, np.inf)))
    tree.call("cost_field", *win, vertex.ctypes.data, cost.ctypes.data)
    return vertex, cost


def batch_cost_field(batch, q, window):
    """rrt_batch_cost_field: for every cell of window = (x0, y0, w, h) of the context's current grid, what batch.connect_goals(q, [cell])
    answers.  Returns (vertex int32 (w, h), cost float64 (w, h)), cell (x, y) at [x - x0, y - y0]: the vertex of the finished tree of
    query q to enter it at -- after keep_tree an alive one, in the numbers of the tree as get_result gave it -- and the cost from the
    start through it; (-1, inf) for an obstacle cell and for a free cell that no vertex sees."""
    return _field(_tree_of(batch, q), window)


def context_cost_field(ctx, window):
    """rrt_plan_cost_field: batch_cost_field on the tree of this context's last plan() / plan_resume()"""
    return _field(_tree_of(ctx), window)


def cost_field_ms(handle):
    """time in ms of the stages of the last cost_field on a Batch or a Context: (buckets, decide, remap, read-back)"""
    return _tree_of(handle).stage_ms("cost_field", 4)


def cost_field_stats(handle):
    """of the last cost_field: dict(cells, buckets, priced, los) -- free cells decided, buckets visited, vertices priced, lines of
    sight walked"""
    return _tree_of(handle).relax_stats("cost_field", FIELD_STATS)


def cost_field(planner, window=None):
    """The cost-to-come field of the tree of planner's last plan(): (vertex int32 (w, h), cost float64 (w, h)) over window =
    (x0, y0, w, h), by default the whole grid.  Entry [x - x0, y - y0] is what planner.connect_goals([(x, y)]) returns for that cell:
    the tree vertex, in the numbers of the T plan() returned, whose line to the cell is free and whose vcost plus the length of that
    line is smallest (the lower number among equals), and that cost; (-1, inf) for an obstacle cell and for a free cell that no vertex
    sees.  After keep_tree the field is taken on the new map over the alive vertices; after grow, reroot and relax over the new tree.

    ValueError for a Dubins planner (its goal is a pose, and there is no field of poses) and for a window that is not four integers
    or does not lie inside the grid; otherwise the errors of connect_goals."""
    if hasattr(planner, "n_headings"):
        raise ValueError("cost_field: a Dubins planner's goal is a pose and its edge a Dubins word; there is no field of poses, and the "
                         "field kernel prices straight lines to cells (RRTStandard, RRTStar, RRTStarInformed only)")
    window = _planner_window("cost_field", planner, window)
    planner._keep_guard("cost_field")
    return context_cost_field(planner._device(), window)
