"""The pose cost field: every cell of the map connected to the finished tree of a Dubins planner (include/rrt_hip_pose_field.h,
rrt_pose_field.h).

connect_poses answers for the goal poses the caller lists.  pose_field answers for the whole grid, or a window of it: per cell the
cost from the start, the tree vertex to leave the tree at and the heading to arrive with -- what connect_poses gives for a pose on that
one cell, entry for entry and bit for bit.  The arrival heading is one the caller fixes, or the best of all n_headings (the
planner's connect_poses with heading -1): the table to pick from when the goal is "any cell of this region, at any heading", and
the vehicle's navigation function over a window.  The vertices are bucketed once per call and one bound serves every heading of a
cell; in a window of 8192 cells and more a cell also starts from its neighbour's winner.  Measured (README, profiles/pose_field_wall.json),
the field wins at any heading where the cells are reached cheaply, by one to three orders of magnitude over the same cells sent
through connect_poses; for a fixed heading on windows with unreached or deeply hidden cells connect_poses remains the faster call,
by up to 4.5 times: there the work is sweeps that no bound removes, and the field gives a cell one wavefront.

The module binds its six symbols itself, on the handle _ffi.lib() returns, through the binder field.py and moving.py use too
(_ffi._side_binding): the signature table of _ffi and the methods of Context, Batch and the planner classes are a recorded surface.

  pose_field(planner, window=None, heading=None)   the field of the tree of planner's last plan(); window (x0, y0, w, h), None: the grid;
                                                   heading None: any arrival heading
  batch_pose_field(batch, q, window, heading=-1)   rrt_batch_pose_field
  context_pose_field(ctx, window, heading=-1)      rrt_plan_pose_field
  pose_field_ms(handle), pose_field_stats(handle)  the stage times and the counters of the last call on a Batch or a Context"""
import ctypes as C

import numpy as np

from . import _ffi
from .field import _answers, _planner_window

POSE_FIELD_STATS = ("cells", "buckets", "words", "sweeps")

_vp, _i32, _i64, _P = C.c_void_p, C.c_int32, C.c_int64, C.POINTER
_PROTOTYPES = {
    "rrt_batch_pose_field": [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "rrt_plan_pose_field": [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp],
    "rrt_batch_pose_field_ms": [_vp, _P(C.c_float * 4)],
    "rrt_plan_pose_field_ms": [_vp, _P(C.c_float * 4)],
    "rrt_batch_pose_field_stats": [_vp, _P(_i64 * 4)],
    "rrt_plan_pose_field_stats": [_vp, _P(_i64 * 4)],
}
_lib, _tree_of = _ffi._side_binding(_PROTOTYPES)


def _field(tree, window, heading):
    """the call on a _Tree: (vertex int32 (w, h), cost float64 (w, h), heading int32 (w, h))"""
    win, out = _answers(window, ((np.int32, -1), (np.float64, np.inf), (np.int32, -1)))
    tree.call("pose_field", *win, int(heading), *(a.ctypes.data for a in out))
    return tuple(out)


def batch_pose_field(batch, q, window, heading=-1):
    """rrt_batch_pose_field: for every cell (x, y) of window = (x0, y0, w, h) of the context's current grid, what
    batch.connect_poses(q, [(x, y, heading)]) answers; with heading -1 the (cost, heading)-smallest of the answers for all the query's
    headings.  Returns (vertex int32 (w, h), cost float64 (w, h), heading int32 (w, h)), cell (x, y) at [x - x0, y - y0]: the vertex of
    the finished Dubins tree of query q to leave it at -- after keep_pose_tree an alive one, in the numbers of the tree as get_result
    gave it --, the cost from the start through it, and the arrival heading of that answer; (-1, inf, -1) for an obstacle cell and for
    a free cell that nothing reaches (connect_poses has no heading to give back; the field writes -1 also where one heading was
    asked for)."""
    return _field(_tree_of(batch, q), window, heading)


def context_pose_field(ctx, window, heading=-1):
    """rrt_plan_pose_field: batch_pose_field on the tree of this context's last plan()"""
    return _field(_tree_of(ctx), window, heading)


def pose_field_ms(handle):
    """time in ms of the stages of the last pose_field on a Batch or a Context: (buckets, decide, remap, read-back)"""
    return _tree_of(handle).stage_ms("pose_field", 4)


def pose_field_stats(handle):
    """of the last pose_field: dict(cells, buckets, words, sweeps) -- free cells decided, buckets visited, Dubins words evaluated,
    sweeps run"""
    return _tree_of(handle).relax_stats("pose_field", POSE_FIELD_STATS)


def pose_field(planner, window=None, heading=None):
    """The pose cost field of the tree of a Dubins planner's last plan(): (vertex int32 (w, h), cost float64 (w, h), heading int32
    (w, h)) over window = (x0, y0, w, h), by default the whole grid.  With heading = H entry [x - x0, y - y0] is what
    planner.connect_poses([(x, y, H)]) returns for that cell; with heading None (or -1), any arrival heading, what
    planner.connect_poses([(x, y, -1)]) returns: over all pairs of a heading and a tree vertex whose Dubins word to the cell sweeps
    free, the smallest (cost, heading, vertex).  The vertex is in the numbers of the T plan() returned.  (-1, inf, -1) for an obstacle
    cell and for a free cell that nothing reaches -- where connect_poses echoes a fixed heading for an unconnected pose, the field
    writes -1.  After keep_pose_tree the field is taken on the new map over the alive vertices; after grow_poses, relax_poses and
    reroot_poses over the new tree.

    ValueError for a straight-line planner (field.cost_field is its field), for a window that is not four integers or does not lie
    inside the grid, and for a heading outside [0, n_headings); otherwise the errors of connect_poses."""
    if not hasattr(planner, "n_headings"):
        raise ValueError("pose_field: a straight-line planner's goal is a cell and its edge a line; its field is field.cost_field "
                         "(RRTDubins, RRTStarDubins only)")
    window = _planner_window("pose_field", planner, window)
    nh = int(planner.n_headings)
    try:
        hd = -1 if heading is None else int(heading)
        ok = hd == heading or heading is None
    except (TypeError, ValueError):
        ok = False
    if not ok or hd < -1 or hd >= nh:
        raise ValueError(f"pose_field: heading must be an integer in [0, {nh}), or None (-1) for any heading, got {heading!r}")
    planner._keep_guard("pose_field")
    return context_pose_field(planner._device(), window, hd)
