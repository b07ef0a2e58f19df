"""The moving start of a Dubins vehicle: re-root the finished Dubins tree at one of its poses (include/rrt_hip_moving.h,
rrt_pose_reroot.h) instead of planning again from the pose the vehicle has reached.

RRT.reroot reverses parent pointers and refuses a Dubins planner, because a Dubins word is not reversible.  reroot_poses builds the
shortest-path tree from the new root's pose over the directed graph of the tree's own poses, as relax_poses builds it from vertex 0:
what hangs below the new root keeps its old edges, everything else is re-attached by words between poses swept on the current map,
what cannot be reached is cut, and m new pose samples grow it back.

The module binds its six symbols itself, on the handle _ffi.lib() returns, through the binder field.py and posefield.py use too
(_ffi._side_binding): the signature table of _ffi and the methods of Context, Batch and the planner classes are a recorded surface.

  reroot_poses(planner, vertex, r=None, m=0)             the call of RRTDubins / RRTStarDubins
  batch_reroot_poses(batch, q, root, r2, samples=())     rrt_batch_reroot_poses
  context_reroot_poses(ctx, root, r2, samples, n)        rrt_plan_reroot_poses
  reroot_poses_ms(handle), reroot_poses_stats(handle)    the stage times and the counters of the last call on a Batch or a Context"""
import ctypes as C

from . import _ffi, hostprep

POSE_REROOT_STATS = ("rounds", "reached", "sweeps", "words")

_vp, _i32, _i64, _P = C.c_void_p, C.c_int32, C.c_int64, C.POINTER
_PROTOTYPES = {
    "rrt_batch_reroot_poses": [_vp, _i32, _i32, _i64, _vp, _i32, _P(_i32), _vp, _P(_i32)],
    "rrt_plan_reroot_poses": [_vp, _i32, _i64, _vp, _i32, _P(_i32), _vp, _P(_ffi.Result)],
    "rrt_batch_reroot_poses_ms": [_vp, _P(C.c_float * 10), _i32],
    "rrt_plan_reroot_poses_ms": [_vp, _P(C.c_float * 10), _i32],
    "rrt_batch_reroot_poses_stats": [_vp, _P(_i64 * 4)],
    "rrt_plan_reroot_poses_stats": [_vp, _P(_i64 * 4)],
}
_lib, _tree_of = _ffi._side_binding(_PROTOTYPES)


def batch_reroot_poses(batch, q, root, r2, samples=()):
    """rrt_batch_reroot_poses: re-root the finished Dubins tree of query q (the alive vertices of its keep_pose_tree view, else the whole
    tree) at its vertex `root`, a number of the tree as get_result gave it, then seed and arm it like grow_poses() for len(samples)
    more iterations.  r2 >= 0: the threshold of the squared distance of the swept candidate edges (hostprep.radius_threshold); 0: the
    old edges alone.  Returns (j0, old_id int32[j0], log0) as Batch.relax_poses."""
    _lib()
    return batch._seed(q, "reroot_poses", (int(root), int(r2)), samples, True)


def context_reroot_poses(ctx, root, r2, samples, n, logs=False):
    """rrt_plan_reroot_poses: batch_reroot_poses on the Dubins tree of this context's last plan(), launch and result (headings
    included) as Context.relax_poses.  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
    _lib()
    return ctx._seed("reroot_poses", (int(root), int(r2)), samples, n, logs, True)


def reroot_poses_ms(handle):
    """time in ms of the stages of the last reroot_poses on a Batch or a Context: (buckets, start, rounds, parents, alive and depth,
    order, costs) and the seed's three"""
    return _tree_of(handle).stage_ms("reroot_poses", 10, 10)


def reroot_poses_stats(handle):
    """of the last reroot_poses: dict(rounds, reached, sweeps, words) -- rounds run, vertices reached (the root among them), sweeps
    run, words evaluated"""
    return _tree_of(handle).relax_stats("reroot_poses", POSE_REROOT_STATS)


def reroot_poses(planner, vertex, r=None, m=0):
    """The start moved: re-root the Dubins tree of planner's last plan() at one of its vertices.  `vertex` is a number of the T the
    caller holds; after a keep_pose_tree those are still the original numbers, and the vertex must be alive.

    The pose of that vertex becomes the start and vertex 0 of a new tree: the shortest-path tree from it over the poses of the old
    tree, whose edges are the words between poses within r cells that sweep free on the current grid, and every old parent edge but
    the root's own.  Vertices that nothing reaches from the new root are cut.  The others are renumbered by (depth, previous
    number) and priced from the root down; then m more pose samples are spent exactly as grow_poses(m) spends them, and the goal
    decision connects plan()'s goal pose.

    r defaults to planner.r_rewire; RRTDubins has none and must pass it.  r = 0 keeps only what hangs below the vertex.  Returns
    (T, gv) as grow_poses.  planner.last_grow_ids[k] is the number vertex k had before the call; planner.last_relax holds dict(rounds,
    reached, sweeps, words).  Raises as grow_poses; ValueError for a straight-line planner (use reroot), a missing or negative r, a
    vertex outside the tree or one that is not alive (the generator's state is restored: a refused vertex spends no draws)."""
    if not hasattr(planner, "n_headings"):
        raise ValueError("reroot_poses: this planner's vertices are cells and its edges straight lines: use reroot (poses belong to RRTDubins "
                         "and RRTStarDubins)")
    if r is None:
        r = getattr(planner, "r_rewire", None)
    if r is None:
        raise ValueError("reroot_poses: this planner has no r_rewire: pass r, the radius of the candidate edges in cells")
    if not (float(r) >= 0):
        raise ValueError(f"reroot_poses: r={r}")
    r2 = hostprep.radius_threshold(r) if float(r) > 0 else 0
    return planner._tree_call("reroot_poses", m, vertex, r2, call=context_reroot_poses, stats=reroot_poses_stats)
