"""ctypes binding of the C ABI in include/rrt_hip.h (librrt_hip.so).

There is no CPU fallback: if the HIP library is missing or cannot be loaded, or no GPU
is visible, the functions here raise.  The library is built in-tree by
``__graft_entry__.build()`` / ``make -C rrtplanner_amd/csrc``.
"""
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RRT_HIP_LIB", os.path.join(_HERE, "librrt_hip.so"))  # override: diagnostic builds only

RRT_OK = 0
RRT_NEED_UNITBALL = 1
RRT_E_ARG = -1
RRT_E_GOAL_UNREACHABLE = -2
RRT_E_HIP = -3
RRT_E_NOGRID = -4
RRT_E_UNSUPPORTED = -5
RRT_E_COMM = -6
RRT_E_INTERNAL = -7

ALG_STANDARD, ALG_STAR, ALG_INFORMED = 0, 1, 2
ALG_DUBINS, ALG_DUBINS_STAR = 3, 4  # no reference counterpart (README only), see include/rrt_dubins.h
FLAG_LOGS = 1
FLAG_SERIAL = 2
FLAG_NOTEAM = 4
FLAG_TEAM_FAULT = 8
FLAG_NOPIPE = 16
FLAG_REWIRE = 32
FLAG_DUBINS = 64
FLAG_ONEBODY = 128
FLAG_NOPIPE1 = 32768
FLAG_LARGE_GRID = 65536
RRT_ROUTES_SHORTCUT = 1  # flags of rrt_batch_routes / rrt_plan_routes
RRT_POSE_ROUTES_POINTS = 1  # flags of rrt_batch_pose_routes / rrt_plan_pose_routes
WALK_AUTO, WALK_U24, WALK_U26, WALK_WIDE = 0, 1, 2, 3  # rrt_prim_collisionfree_walk


def kernel_flags(logs=False, serial=False, team=None, team_fault=False, pipe=True, rewire=False, dubins=False, pipe1=True, onebody=False,
                 large_grid=False):
    """flags word of rrt_plan / rrt_batch_create.  team: None = as many CUs per query as fit (up to 64), 1 = one CU,
    2..64 = cap on the team's workers; pipe = False: no pipelined teams (workers + one committing CU); team_fault = the
    fault-injection flag of the tests; large_grid = grids up to 4096 x 4096, RRTStandard / RRTStar on one CU per query
    (rrt_pipe_large_kernel)."""
    f = (FLAG_LOGS if logs else 0) | (FLAG_SERIAL if serial else 0) | (FLAG_TEAM_FAULT if team_fault else 0) | (0 if pipe else FLAG_NOPIPE)
    f |= FLAG_REWIRE if rewire else 0  # the opt-in true rewire (not the reference's behaviour)
    f |= FLAG_DUBINS if dubins else 0
    f |= 0 if pipe1 else FLAG_NOPIPE1  # one CU per query: the block kernel instead of the barrier-free pipeline (a cross-check)
    f |= FLAG_LARGE_GRID if large_grid else 0
    f |= FLAG_ONEBODY if onebody else 0  # pipelined teams of 8+: committer and workers as one kernel instead of two (a cross-check)
    if team == 1:
        f |= FLAG_NOTEAM
    elif team is not None:
        if team not in (2, 3, 4, 8, 16, 32, 64):
            raise ValueError("team must be None, 1, 2, 3, 4, 8, 16, 32 or 64")
        f |= int(team) << 8
    return f

# every symbol include/rrt_hip.h declares (tests/test_capi_symbols.py checks the library exports them)
SYMBOLS = (
    "rrt_ctx_create", "rrt_ctx_destroy", "rrt_last_error_string", "rrt_set_grid", "rrt_noise_grids", "rrt_select_frame",
    "rrt_grid_generation", "rrt_ctx_sync",
    "rrt_comm_use_library", "rrt_comm_unique_id", "rrt_comm_init", "rrt_comm_destroy", "rrt_comm_allreduce_f64", "rrt_gather", "rrt_gather_fetch",
    "rrt_batch_create", "rrt_batch_destroy", "rrt_batch_set_query", "rrt_batch_set_unitball",
    "rrt_batch_rearm", "rrt_batch_launch", "rrt_batch_sync", "rrt_batch_team", "rrt_batch_team_info", "rrt_batch_pipelined", "rrt_batch_kernel_name", "rrt_batch_elapsed_ms",
    "rrt_batch_get_result", "rrt_batch_result_block", "rrt_batch_debug_cycles",
    "rrt_plan", "rrt_plan_resume", "rrt_plan_batch",
    "rrt_tree_create", "rrt_tree_destroy", "rrt_tree_reset", "rrt_tree_append", "rrt_tree_query",
    "rrt_prim_collisionfree", "rrt_prim_nearest_within", "rrt_prim_sqrt_u32", "rrt_prim_sqrt_u24", "rrt_prim_sqrt_f64",
    "rrt_prim_collisionfree_walk", "rrt_prim_sqrt_u25",
    "rrt_batch_connect_goals", "rrt_plan_connect_goals",
    "rrt_batch_routes", "rrt_batch_routes_rows", "rrt_plan_routes", "rrt_plan_routes_rows",
    "rrt_batch_keep_tree", "rrt_batch_keep_tree_ms", "rrt_plan_keep_tree", "rrt_plan_keep_tree_ms", "rrt_plan_tree_size",
    "rrt_batch_grow", "rrt_batch_grow_ms", "rrt_plan_grow", "rrt_plan_grow_ms",
    "rrt_batch_grow_poses", "rrt_plan_grow_poses",
    "rrt_batch_reroot", "rrt_batch_reroot_ms", "rrt_plan_reroot", "rrt_plan_reroot_ms",
    "rrt_batch_relax", "rrt_batch_relax_ms", "rrt_batch_relax_stats", "rrt_plan_relax", "rrt_plan_relax_ms", "rrt_plan_relax_stats",
    "rrt_batch_relax_poses", "rrt_batch_relax_poses_ms", "rrt_batch_relax_poses_stats",
    "rrt_plan_relax_poses", "rrt_plan_relax_poses_ms", "rrt_plan_relax_poses_stats",
    "rrt_batch_connect_poses", "rrt_plan_connect_poses", "rrt_batch_connect_poses_counts",
    "rrt_batch_keep_pose_tree", "rrt_plan_keep_pose_tree",
    "rrt_batch_pose_routes", "rrt_batch_pose_routes_rows", "rrt_batch_pose_routes_points", "rrt_batch_pose_routes_ms",
    "rrt_plan_pose_routes", "rrt_plan_pose_routes_rows", "rrt_plan_pose_routes_points", "rrt_plan_pose_routes_ms",
    "rrt_batch_pose_shortcuts", "rrt_batch_pose_shortcuts_ms", "rrt_plan_pose_shortcuts", "rrt_plan_pose_shortcuts_ms",
)


class RRTError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"librrt_hip error {code}: {msg}")
        self.code = code


class Query(C.Structure):
    _fields_ = [
        ("alg", C.c_int32), ("n", C.c_int32),
        ("xs", C.c_int32 * 2), ("xg", C.c_int32 * 2),
        ("r2_rewire", C.c_int64), ("goal_d2", C.c_int64),
        ("samples", C.c_void_p),
        ("C", C.c_double * 4),
        ("headings", C.c_void_p), ("rho", C.c_double), ("nh", C.c_int32), ("hs", C.c_int32), ("hg", C.c_int32), ("pad_", C.c_int32),
        ("samples_packed", C.c_void_p),
    ]


class Result(C.Structure):
    _fields_ = [
        ("pts", C.c_void_p), ("vcost", C.c_void_p), ("parent", C.c_void_p),
        ("nearest_log", C.c_void_p), ("accept_log", C.c_void_p), ("cbest_log", C.c_void_p), ("j_log", C.c_void_p),
        ("status", C.c_int32), ("j", C.c_int32), ("vgoal", C.c_int32), ("found", C.c_int32),
        ("i_switch", C.c_int32), ("rows", C.c_int32),
        ("sum_j", C.c_int64), ("sum_cells_nn", C.c_int64), ("sum_near", C.c_int64), ("sum_cells_cand", C.c_int64),
        ("n_los_cand", C.c_int64), ("n_rewired", C.c_int64), ("n_propagated", C.c_int64),
        ("head", C.c_void_p),
        ("n_words", C.c_int64),
    ]


_lib = None


def lib():
    """Load librrt_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  rrtplanner_amd has no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        vp, i32, u32, i64 = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64
        sig = {
            "rrt_ctx_create": ([i32, C.POINTER(vp)], C.c_int),
            "rrt_ctx_destroy": ([vp], C.c_int),
            "rrt_last_error_string": ([vp], C.c_char_p),
            "rrt_set_grid": ([vp, vp, i32, i32], C.c_int),
            "rrt_noise_grids": ([vp, i32, i32, i32, C.c_float, i32, vp, vp, vp, vp, vp], C.c_int),
            "rrt_select_frame": ([vp, i32], C.c_int),
            "rrt_grid_generation": ([vp, C.POINTER(C.c_uint64)], C.c_int),
            "rrt_ctx_sync": ([vp], C.c_int),
            "rrt_comm_use_library": ([C.c_char_p], C.c_int),
            "rrt_comm_unique_id": ([vp], C.c_int),
            "rrt_comm_init": ([vp, i32, i32, vp], C.c_int),
            "rrt_comm_destroy": ([vp], C.c_int),
            "rrt_comm_allreduce_f64": ([vp, vp, i32, i32], C.c_int),
            "rrt_gather": ([vp, C.POINTER(vp), C.POINTER(i64)], C.c_int),
            "rrt_gather_fetch": ([vp, i32, i32, C.POINTER(Result)], C.c_int),
            "rrt_batch_create": ([vp, i32, i32, u32, C.POINTER(vp)], C.c_int),
            "rrt_batch_destroy": ([vp], C.c_int),
            "rrt_batch_set_query": ([vp, i32, C.POINTER(Query)], C.c_int),
            "rrt_batch_set_unitball": ([vp, i32, vp, i32, i32], C.c_int),
            "rrt_batch_rearm": ([vp], C.c_int),
            "rrt_batch_launch": ([vp], C.c_int),
            "rrt_batch_sync": ([vp], C.c_int),
            "rrt_batch_team": ([vp, C.POINTER(i32), C.POINTER(i32)], C.c_int),
            "rrt_batch_team_info": ([vp, C.POINTER(i32 * 4)], C.c_int),
            "rrt_batch_pipelined": ([vp, C.POINTER(i32)], C.c_int),
            "rrt_batch_kernel_name": ([vp, C.c_char_p, i32], C.c_int),
            "rrt_batch_elapsed_ms": ([vp, C.POINTER(C.c_float)], C.c_int),
            "rrt_batch_get_result": ([vp, i32, C.POINTER(Result)], C.c_int),
            "rrt_batch_result_block": ([vp, C.POINTER(vp), C.POINTER(i64)], C.c_int),
            "rrt_batch_debug_cycles": ([vp, i32, C.POINTER(C.c_uint64 * 38)], C.c_int),
            "rrt_plan": ([vp, C.POINTER(Query), u32, C.POINTER(Result)], C.c_int),
            "rrt_plan_resume": ([vp, vp, i32, C.POINTER(Result)], C.c_int),
            "rrt_plan_batch": ([vp, i32, C.POINTER(Query), C.POINTER(Result)], C.c_int),
            "rrt_tree_create": ([vp, i32, C.POINTER(vp)], C.c_int),
            "rrt_tree_destroy": ([vp], C.c_int),
            "rrt_tree_reset": ([vp], C.c_int),
            "rrt_tree_append": ([vp, i32, i32, C.POINTER(i32)], C.c_int),
            "rrt_tree_query": ([vp, i32, i32, i64, C.POINTER(i32), C.POINTER(i32), vp, vp, i32], C.c_int),
            "rrt_prim_collisionfree": ([vp, vp, i32, vp, vp], C.c_int),
            "rrt_prim_nearest_within": ([vp, vp, i32, vp, i32, i64, vp, vp, vp], C.c_int),
            "rrt_prim_sqrt_u32": ([vp, u32, u32, vp], C.c_int),
            "rrt_prim_sqrt_u24": ([vp, u32, u32, vp], C.c_int),
            "rrt_prim_sqrt_f64": ([vp, vp, u32, vp], C.c_int),
            "rrt_prim_collisionfree_walk": ([vp, vp, i32, i32, vp, vp], C.c_int),
            "rrt_prim_sqrt_u25": ([vp, u32, u32, vp], C.c_int),
            "rrt_batch_connect_goals": ([vp, i32, vp, i32, vp, vp], C.c_int),
            "rrt_plan_connect_goals": ([vp, vp, i32, vp, vp], C.c_int),
            "rrt_batch_routes": ([vp, i32, vp, i32, u32, vp, vp, vp, vp], C.c_int),
            "rrt_batch_routes_rows": ([vp, vp, vp, C.c_int64], C.c_int),
            "rrt_plan_routes": ([vp, vp, i32, u32, vp, vp, vp, vp], C.c_int),
            "rrt_plan_routes_rows": ([vp, vp, vp, C.c_int64], C.c_int),
            "rrt_batch_keep_tree": ([vp, i32, C.POINTER(i32), vp], C.c_int),
            "rrt_batch_keep_tree_ms": ([vp, C.POINTER(C.c_float * 3)], C.c_int),
            "rrt_plan_keep_tree": ([vp, C.POINTER(i32), vp], C.c_int),
            "rrt_plan_keep_tree_ms": ([vp, C.POINTER(C.c_float * 3)], C.c_int),
            "rrt_plan_tree_size": ([vp, C.POINTER(i32)], C.c_int),
            "rrt_batch_grow": ([vp, i32, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)], C.c_int),
            "rrt_batch_grow_ms": ([vp, C.POINTER(C.c_float * 3), i32], C.c_int),
            "rrt_plan_grow": ([vp, vp, i32, C.POINTER(i32), vp, C.POINTER(Result)], C.c_int),
            "rrt_plan_grow_ms": ([vp, C.POINTER(C.c_float * 3), i32], C.c_int),
            "rrt_batch_grow_poses": ([vp, i32, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)], C.c_int),
            "rrt_plan_grow_poses": ([vp, vp, i32, C.POINTER(i32), vp, C.POINTER(Result)], C.c_int),
            "rrt_batch_reroot": ([vp, i32, i32, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)], C.c_int),
            "rrt_batch_reroot_ms": ([vp, C.POINTER(C.c_float * 8), i32], C.c_int),
            "rrt_plan_reroot": ([vp, i32, vp, i32, C.POINTER(i32), vp, C.POINTER(Result)], C.c_int),
            "rrt_plan_reroot_ms": ([vp, C.POINTER(C.c_float * 8), i32], C.c_int),
            "rrt_batch_relax": ([vp, i32, i64, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)], C.c_int),
            "rrt_batch_relax_ms": ([vp, C.POINTER(C.c_float * 9), i32], C.c_int),
            "rrt_batch_relax_stats": ([vp, C.POINTER(i64 * 4)], C.c_int),
            "rrt_plan_relax": ([vp, i64, vp, i32, C.POINTER(i32), vp, C.POINTER(Result)], C.c_int),
            "rrt_plan_relax_ms": ([vp, C.POINTER(C.c_float * 9), i32], C.c_int),
            "rrt_plan_relax_stats": ([vp, C.POINTER(i64 * 4)], C.c_int),
            "rrt_batch_relax_poses": ([vp, i32, i64, vp, i32, C.POINTER(i32), vp, C.POINTER(i32)], C.c_int),
            "rrt_batch_relax_poses_ms": ([vp, C.POINTER(C.c_float * 9), i32], C.c_int),
            "rrt_batch_relax_poses_stats": ([vp, C.POINTER(i64 * 4)], C.c_int),
            "rrt_plan_relax_poses": ([vp, i64, vp, i32, C.POINTER(i32), vp, C.POINTER(Result)], C.c_int),
            "rrt_plan_relax_poses_ms": ([vp, C.POINTER(C.c_float * 9), i32], C.c_int),
            "rrt_plan_relax_poses_stats": ([vp, C.POINTER(i64 * 4)], C.c_int),
            "rrt_batch_connect_poses": ([vp, i32, vp, i32, vp, vp], C.c_int),
            "rrt_plan_connect_poses": ([vp, vp, i32, vp, vp], C.c_int),
            "rrt_batch_connect_poses_counts": ([vp, C.POINTER(C.c_int64 * 2)], C.c_int),
            "rrt_batch_keep_pose_tree": ([vp, i32, C.POINTER(i32), vp], C.c_int),
            "rrt_plan_keep_pose_tree": ([vp, C.POINTER(i32), vp], C.c_int),
            "rrt_batch_pose_routes": ([vp, i32, vp, i32, u32, vp, vp, vp, vp, vp], C.c_int),
            "rrt_batch_pose_routes_rows": ([vp, vp, vp, C.c_int64], C.c_int),
            "rrt_batch_pose_routes_points": ([vp, vp, C.c_int64], C.c_int),
            "rrt_batch_pose_routes_ms": ([vp, C.POINTER(C.c_float * 4)], C.c_int),
            "rrt_plan_pose_routes": ([vp, vp, i32, u32, vp, vp, vp, vp, vp], C.c_int),
            "rrt_plan_pose_routes_rows": ([vp, vp, vp, C.c_int64], C.c_int),
            "rrt_plan_pose_routes_points": ([vp, vp, C.c_int64], C.c_int),
            "rrt_plan_pose_routes_ms": ([vp, C.POINTER(C.c_float * 4)], C.c_int),
            "rrt_batch_pose_shortcuts": ([vp, i32, vp, i32, u32, vp, vp, vp, vp, vp], C.c_int),
            "rrt_batch_pose_shortcuts_ms": ([vp, C.POINTER(C.c_float * 5)], C.c_int),
            "rrt_plan_pose_shortcuts": ([vp, vp, i32, u32, vp, vp, vp, vp, vp], C.c_int),
            "rrt_plan_pose_shortcuts_ms": ([vp, C.POINTER(C.c_float * 5)], C.c_int),
        }
        for name, (argtypes, restype) in sig.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = restype
        _lib = L
    return _lib


def _check(ctx_handle, rc, ok=(RRT_OK,)):
    if rc in ok:
        return rc
    msg = lib().rrt_last_error_string(ctx_handle)
    raise RRTError(rc, msg.decode() if msg else "")


COMM_ID_BYTES = 128


def comm_use_library(path):
    """Before the first communicator of the process: open `path` instead of librccl.so.1 (None: the default).  For ranks that
    share one GPU (tests/fake_rccl); see include/rrt_hip.h."""
    _check(None, lib().rrt_comm_use_library(None if path is None else os.fsencode(path)))


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (rank 0 creates it and ships it to the other ranks, see multi.exchange_unique_id)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(None, lib().rrt_comm_unique_id(C.cast(buf, C.c_void_p)))
    return bytes(buf)


def _goal_arrays(goals, cols=2):
    """(goals as contiguous int32 (M, cols), vertex int32[M], cost float64[M]) for the connect_goals (cols = 2: cells) and
    connect_poses (cols = 3: poses) calls and the routes calls; a single goal is M = 1"""
    g = np.asarray(goals)
    if g.ndim == 1 and g.shape == (cols,):
        g = g[np.newaxis, :]
    if g.ndim != 2 or g.shape[1] != cols:
        raise ValueError(f"{'goals' if cols == 2 else 'poses'} must have shape (M, {cols}) or ({cols},), got {g.shape}")
    g = np.ascontiguousarray(g, dtype=np.int32)
    return g, np.full(g.shape[0], -1, dtype=np.int32), np.full(g.shape[0], np.inf, dtype=np.float64)


def _pose_arrays(poses):
    return _goal_arrays(poses, 3)


def _routes(handle, call, rows_call, goals, shortcut):
    """the two steps of a routes call: `call` decides and builds the routes on the device and gives the CSR offsets, `rows_call`
    copies the rows out.  (vertex, cost, length, offsets int64[M + 1], xy int32[(rows, 2)], ids int32[rows])"""
    g, vertex, cost = _goal_arrays(goals)
    m = g.shape[0]
    length = np.full(m, np.inf, dtype=np.float64)
    offsets = np.zeros(m + 1, dtype=np.int64)
    _check(handle, call(g.ctypes.data, m, RRT_ROUTES_SHORTCUT if shortcut else 0, vertex.ctypes.data, cost.ctypes.data, length.ctypes.data, offsets.ctypes.data))
    rows = int(offsets[m])
    xy = np.empty((rows, 2), dtype=np.int32)
    ids = np.empty(rows, dtype=np.int32)
    _check(handle, rows_call(xy.ctypes.data, ids.ctypes.data, rows))
    return vertex, cost, length, offsets, xy, ids


def _pose_routes(handle, call, rows_call, points_call, poses, points):
    """the steps of a pose routes call: `call` decides and builds the routes on the device and gives the CSR offsets, `rows_call` and,
    with points, `points_call` copy the rows and the points out.  (vertex, cost, length, offsets int64[M + 1], xyh int32[(rows, 3)],
    ids int32[rows]) and with points (point_offsets int64[M + 1], pts float64[(P, 2)]) behind them"""
    g, vertex, cost = _pose_arrays(poses)
    m = g.shape[0]
    length = np.full(m, np.inf, dtype=np.float64)
    offsets = np.zeros(m + 1, dtype=np.int64)
    point_offsets = np.zeros(m + 1, dtype=np.int64) if points else None
    _check(handle, call(g.ctypes.data, m, RRT_POSE_ROUTES_POINTS if points else 0, vertex.ctypes.data, cost.ctypes.data, length.ctypes.data,
                        offsets.ctypes.data, point_offsets.ctypes.data if points else None))
    rows = int(offsets[m])
    xyh = np.empty((rows, 3), dtype=np.int32)
    ids = np.empty(rows, dtype=np.int32)
    _check(handle, rows_call(xyh.ctypes.data, ids.ctypes.data, rows))
    if not points:
        return vertex, cost, length, offsets, xyh, ids
    pts = np.empty((int(point_offsets[m]), 2), dtype=np.float64)
    _check(handle, points_call(pts.ctypes.data, pts.shape[0]))
    return vertex, cost, length, offsets, xyh, ids, point_offsets, pts


def _keep_tree(handle, call, size, j):
    """a keep_tree call: `call` takes (n_alive, alive) and fills one flag per vertex of the tree.  `size` bounds them and comes from
    the library: the capacity the batch was created with, or the tree size the library reports for the query.  j() is asked for the
    vertices of the tree after the call has accepted the query.  bool[j]"""
    alive = np.zeros(max(int(size), 1), dtype=np.uint8)
    n_alive = C.c_int32(-1)
    _check(handle, call(C.byref(n_alive), alive.ctypes.data))
    alive = alive[:int(j())].astype(bool)
    if int(alive.sum()) != n_alive.value:
        raise RRTError(RRT_E_HIP, f"keep_tree: {n_alive.value} vertices alive, {int(alive.sum())} flags set")
    return alive


def _grow_samples(samples, poses=False):
    """the samples of a grow call as contiguous int32 (m, 2), packed uint32 samples (x | y << 16) unpacked; of a grow_poses call
    (poses) as contiguous int32 (m, 3): rows (x, y, heading index)"""
    s = np.asarray(samples)
    if not poses and s.dtype == np.uint32 and s.ndim == 1:
        s = np.stack([s & 0xFFFF, s >> 16], axis=1)
    if poses and s.size and (s.ndim != 2 or s.shape[1] != 3):
        raise ValueError(f"pose samples must have shape (m, 3), got {s.shape}")
    return np.ascontiguousarray(s, dtype=np.int32).reshape(-1, 3 if poses else 2)


def _grow_pose_samples(samples):
    return _grow_samples(samples, True)


def _stage_ms(handle, call, stages, *count):
    """a *_ms call: the kernel time in ms of the `stages` stages of the last call it reports on, as a tuple"""
    ms = (C.c_float * stages)()
    _check(handle, call(C.byref(ms), *count))
    return tuple(ms)


def _relax_stats(handle, call, names=("rounds", "fell", "los", "priced")):
    out = (C.c_int64 * 4)()
    _check(handle, call(C.byref(out)))
    return dict(zip(names, (int(v) for v in out)))


POSE_RELAX_STATS = ("rounds", "fell", "sweeps", "words")


class ResultArrays:
    """Host buffers for one query's result + the filled-in rrt_result."""

    def __init__(self, n, logs=False, headings=False):
        self.n = n
        if headings:
            self.head = np.zeros(n + 1, dtype=np.int32)
        self.pts = np.zeros((n + 1, 2), dtype=np.int32)
        self.vcost = np.zeros(n + 1, dtype=np.float64)
        self.parent = np.full(n + 1, -1, dtype=np.int32)
        self.c = Result()
        self.c.pts, self.c.vcost, self.c.parent = self.pts.ctypes.data, self.vcost.ctypes.data, self.parent.ctypes.data
        if headings:
            self.c.head = self.head.ctypes.data
        if logs:
            self.nearest_log = np.full(n, -1, dtype=np.int32)
            self.accept_log = np.zeros(n, dtype=np.uint8)
            self.cbest_log = np.full(n, np.nan)
            self.j_log = np.zeros(n, dtype=np.int32)
            self.c.nearest_log, self.c.accept_log = self.nearest_log.ctypes.data, self.accept_log.ctypes.data
            self.c.cbest_log, self.c.j_log = self.cbest_log.ctypes.data, self.j_log.ctypes.data

    def __getattr__(self, k):  # scalars live in the C struct
        if k in ("status", "j", "vgoal", "found", "i_switch", "rows", "sum_j", "sum_cells_nn", "sum_near",
                 "sum_cells_cand", "n_los_cand", "n_rewired", "n_propagated", "n_words"):
            return getattr(self.c, k)
        raise AttributeError(k)


def make_query(alg, n, xs, xg, samples, r2_rewire=0, goal_d2=0, Cmat=None, headings=None, rho=0.0, nh=0):
    """Build an rrt_query; returns (Query, keepalive).  Dubins queries (alg 3 / 4): xs / xg are (x, y, heading index),
    `headings` the heading index of every sample, rho the turning radius in cells, nh the number of headings."""
    q = Query()
    if isinstance(samples, np.ndarray) and samples.dtype == np.uint32 and samples.shape == (n,):
        s = np.ascontiguousarray(samples)  # already packed: x | y << 16
        q.samples_packed = s.ctypes.data
    else:
        s = np.ascontiguousarray(samples, dtype=np.int32)
        if s.shape != (n, 2):
            raise ValueError(f"samples must have shape ({n}, 2), got {s.shape}")
        q.samples = s.ctypes.data
    q.alg, q.n = int(alg), int(n)
    q.xs[0], q.xs[1] = int(xs[0]), int(xs[1])
    q.xg[0], q.xg[1] = int(xg[0]), int(xg[1])
    q.r2_rewire, q.goal_d2 = int(r2_rewire), int(goal_d2)
    if Cmat is not None:
        cm = np.asarray(Cmat, dtype=np.float64).reshape(4)
        for k in range(4):
            q.C[k] = float(cm[k])
    if headings is not None:
        hd = np.ascontiguousarray(headings, dtype=np.int32)
        if hd.shape != (n,):
            raise ValueError(f"headings must have shape ({n},), got {hd.shape}")
        q.headings, q.rho, q.nh, q.hs, q.hg = hd.ctypes.data, float(rho), int(nh), int(xs[2]), int(xg[2])
        return q, (s, hd)
    return q, s


def _adopt(ctx, child, destroy):
    """A batch or a device tree holds a pointer to its context and has to be destroyed before it.  The context knows its live
    children (weakly, to close the Python objects) and their native handles (to destroy them itself when the objects are already
    beyond reach); a child destroys its handle only while the context still lists it."""
    if not hasattr(ctx, "_batches"):
        ctx._batches = weakref.WeakSet()
        ctx._natives = {}
    ctx._batches.add(child)
    ctx._natives[id(child)] = (destroy, child._h.value)


def _disown(child, destroy):
    if child._h:
        if getattr(child.ctx, "_natives", {}).pop(id(child), None) is not None:
            getattr(lib(), destroy)(child._h)
        child._h = C.c_void_p()


class Context:
    """One device context: a HIP stream + the device-resident occupancy grid."""

    def __init__(self, device_id=0):
        self._h = C.c_void_p()
        rc = lib().rrt_ctx_create(int(device_id), C.byref(self._h))
        _check(None, rc)
        self.shape = None

    @property
    def handle(self):
        return self._h

    def close(self):
        for b in list(getattr(self, "_batches", ())):  # batches hold a pointer to the context: they go first
            b.close()
        # ... also those that the garbage collector finalises in the same pass as this context: their weak references are
        # cleared before any __del__ runs, so the set above no longer names them, and their own __del__ may come after this one
        natives = getattr(self, "_natives", {})
        for destroy, h in list(natives.values()):
            getattr(lib(), destroy)(C.c_void_p(h))
        natives.clear()
        if self._h:
            lib().rrt_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_grid(self, og_nonzero):
        g = np.ascontiguousarray(og_nonzero, dtype=np.uint8)
        if g.ndim != 2:
            raise ValueError("occupancy grid must be 2-D")
        _check(self._h, lib().rrt_set_grid(self._h, g.ctypes.data, g.shape[0], g.shape[1]))
        self.shape = g.shape

    def noise_grids(self, W, H, frames, thresh, dims, cells, amps, grads):
        """Generate `frames` noise grids on the device; returns the host copy (frames, W, H) uint8."""
        dims = np.ascontiguousarray(dims, dtype=np.int32).reshape(-1, 3)
        cells = np.ascontiguousarray(cells, dtype=np.float64)
        amps = np.ascontiguousarray(amps, dtype=np.float64)
        grads = np.ascontiguousarray(grads, dtype=np.float64)
        out = np.zeros((frames, W, H), dtype=np.uint8)
        _check(self._h, lib().rrt_noise_grids(self._h, int(W), int(H), int(frames), float(thresh), dims.shape[0], dims.ctypes.data,
                                              cells.ctypes.data, amps.ctypes.data, grads.ctypes.data, out.ctypes.data))
        self.shape = (W, H)
        return out

    def select_frame(self, k):
        _check(self._h, lib().rrt_select_frame(self._h, int(k)))

    def grid_generation(self):
        """How often the context's grid storage has been rewritten (set_grid / noise_grids); resident frames are only
        valid while this has the value it had right after they were generated."""
        g = C.c_uint64(0)
        _check(self._h, lib().rrt_grid_generation(self._h, C.byref(g)))
        return g.value

    def sync(self):
        _check(self._h, lib().rrt_ctx_sync(self._h))

    # ---- multi-GPU (RCCL) ----
    def comm_init(self, rank, world, unique_id: bytes):
        """Collective: join the communicator `unique_id` (comm_unique_id() of rank 0) as `rank` of `world`."""
        if len(unique_id) != COMM_ID_BYTES:
            raise ValueError(f"unique id must have {COMM_ID_BYTES} bytes")
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(self._h, lib().rrt_comm_init(self._h, int(rank), int(world), C.cast(buf, C.c_void_p)))
        self.rank, self.world = int(rank), int(world)

    def comm_destroy(self):
        _check(self._h, lib().rrt_comm_destroy(self._h))

    def allreduce(self, values, op="sum"):
        """All-reduce a few float64 values over the ranks (sum / max / min); synchronous, so it doubles as the barrier."""
        v = np.ascontiguousarray(values, dtype=np.float64).copy()
        _check(self._h, lib().rrt_comm_allreduce_f64(self._h, v.ctypes.data, v.size, {"sum": 0, "max": 1, "min": 2}[op]))
        return v

    def barrier(self):
        self.allreduce([0.0])

    # ---- one-shot ----
    def plan(self, query, n, logs=False, serial=False, team=None, team_fault=False, pipe=True, rewire=False, pipe1=True, onebody=False,
             large_grid=False):
        res = ResultArrays(n, logs, headings=query.alg >= ALG_DUBINS)
        flags = kernel_flags(logs, serial, team, team_fault, pipe, rewire, pipe1=pipe1, onebody=onebody, large_grid=large_grid)
        rc = lib().rrt_plan(self._h, C.byref(query), flags, C.byref(res.c))
        _check(self._h, rc, ok=(RRT_OK, RRT_NEED_UNITBALL, RRT_E_GOAL_UNREACHABLE))
        return rc, res

    def plan_resume(self, unitball, res):
        ub = np.ascontiguousarray(unitball, dtype=np.float64)
        rc = lib().rrt_plan_resume(self._h, ub.ctypes.data, ub.shape[0], C.byref(res.c))
        _check(self._h, rc, ok=(RRT_OK, RRT_NEED_UNITBALL, RRT_E_GOAL_UNREACHABLE))
        return rc

    def connect_goals(self, goals):
        """rrt_plan_connect_goals: Batch.connect_goals on the tree of this context's last plan() / plan_resume()"""
        g, vertex, cost = _goal_arrays(goals)
        _check(self._h, lib().rrt_plan_connect_goals(self._h, g.ctypes.data, g.shape[0], vertex.ctypes.data, cost.ctypes.data))
        return vertex, cost

    def connect_poses(self, poses):
        """rrt_plan_connect_poses: Batch.connect_poses on the Dubins tree of this context's last plan()"""
        g, vertex, cost = _pose_arrays(poses)
        _check(self._h, lib().rrt_plan_connect_poses(self._h, g.ctypes.data, g.shape[0], vertex.ctypes.data, cost.ctypes.data))
        return vertex, cost

    def routes(self, goals, shortcut=False):
        """rrt_plan_routes + rrt_plan_routes_rows: Batch.routes on the tree of this context's last plan() / plan_resume()"""
        L = lib()
        return _routes(self._h, lambda *a: L.rrt_plan_routes(self._h, *a), lambda *a: L.rrt_plan_routes_rows(self._h, *a), goals, shortcut)

    def pose_routes(self, poses, points=False, shortcut=False):
        """rrt_plan_pose_routes (shortcut=True: rrt_plan_pose_shortcuts) + rrt_plan_pose_routes_rows (+ rrt_plan_pose_routes_points):
        Batch.pose_routes on the Dubins tree of this context's last plan()"""
        L = lib()
        call = L.rrt_plan_pose_shortcuts if shortcut else L.rrt_plan_pose_routes
        return _pose_routes(self._h, lambda *a: call(self._h, *a), lambda *a: L.rrt_plan_pose_routes_rows(self._h, *a),
                            lambda *a: L.rrt_plan_pose_routes_points(self._h, *a), poses, points)

    def pose_shortcuts_ms(self):
        """kernel time in ms of the last pose_routes(shortcut=True): (decision, depth and scan, rows + shortcuts + scan + pack, legs +
        lengths, points)"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_pose_shortcuts_ms(self._h, *a), 5)

    def pose_routes_ms(self):
        """kernel time in ms of the last pose_routes(): (decision, depth and scan, rows + legs + lengths, points)"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_pose_routes_ms(self._h, *a), 4)

    def keep_tree(self):
        """rrt_plan_keep_tree: Batch.keep_tree on the tree of this context's last plan() / plan_resume()"""
        L = lib()
        j = C.c_int32(0)
        _check(self._h, L.rrt_plan_tree_size(self._h, C.byref(j)))
        return _keep_tree(self._h, lambda *a: L.rrt_plan_keep_tree(self._h, *a), j.value, lambda: j.value)

    def keep_pose_tree(self):
        """rrt_plan_keep_pose_tree: Batch.keep_pose_tree on the Dubins tree of this context's last plan()"""
        L = lib()
        j = C.c_int32(0)
        _check(self._h, L.rrt_plan_tree_size(self._h, C.byref(j)))
        return _keep_tree(self._h, lambda *a: L.rrt_plan_keep_pose_tree(self._h, *a), j.value, lambda: j.value)

    def keep_tree_ms(self):
        """kernel time in ms of the last keep_tree() or keep_pose_tree(): (edge test, pointer jumping, compaction)"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_keep_tree_ms(self._h, *a), 3)

    def grow(self, samples, n, logs=False):
        """rrt_plan_grow: Batch.grow on the tree of this context's last plan() / plan_resume(), launch and result included.  n: the
        n of that plan (the result arrays are sized by it).  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
        return self._grow(samples, n, logs, False)

    def _grow(self, samples, n, logs, poses, root=None, r2=None):
        s = _grow_samples(samples, poses)
        res = ResultArrays(int(n), logs, headings=poses)
        j0 = C.c_int32(-1)
        old_id = np.full(int(n) + 1, -1, dtype=np.int32)
        if r2 is not None:
            call = lib().rrt_plan_relax_poses if poses else lib().rrt_plan_relax
            rc = call(self._h, int(r2), s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(res.c))
        elif root is not None:
            rc = lib().rrt_plan_reroot(self._h, int(root), s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(res.c))
        else:
            call = lib().rrt_plan_grow_poses if poses else lib().rrt_plan_grow
            rc = call(self._h, s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(res.c))
        try:
            _check(self._h, rc, ok=(RRT_OK, RRT_E_GOAL_UNREACHABLE))
        except RRTError as e:
            e.seeded = j0.value >= 0  # False: the call refused before the seed and changed nothing
            raise
        return rc, res, j0.value, old_id[:j0.value].copy()

    def grow_poses(self, samples, n, logs=False):
        """rrt_plan_grow_poses: Batch.grow_poses on the Dubins tree of this context's last plan(), launch and result (headings
        included) as grow().  samples: (m, 3) rows (x, y, heading index).  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
        return self._grow(samples, n, logs, True)

    def grow_ms(self):
        """kernel time in ms of the seed stages of the last grow(): (renumbering and node slots, bitmap, cell records)"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_grow_ms(self._h, *a), 3, 3)

    def reroot(self, root, samples, n, logs=False):
        """rrt_plan_reroot: Batch.reroot on the tree of this context's last plan() / plan_resume(), launch and result included.
        root: a vertex number of that tree; n: the n of that plan.  Returns (rc, ResultArrays, j0, old_id int32[j0]) as grow()."""
        return self._grow(samples, n, logs, False, root=root)

    def reroot_ms(self):
        """kernel time in ms of the stages of the last reroot(): (path, reversed edges, alive and depth, order, costs) and the
        seed's three as grow_ms() gives them"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_reroot_ms(self._h, *a), 8, 8)

    def relax(self, r2, samples, n, logs=False):
        """rrt_plan_relax: Batch.relax on the tree of this context's last plan() / plan_resume(), launch and result included.
        r2: the threshold of the squared distance (hostprep.radius_threshold(r)); n: the n of that plan.  Returns (rc, ResultArrays, j0,
        old_id int32[j0]) as grow()."""
        return self._grow(samples, n, logs, False, r2=r2)

    def relax_ms(self):
        """time in ms of the stages of the last relax(): (buckets, rounds, parents, alive and depth, order, costs) and the seed's three
        as grow_ms() gives them"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_relax_ms(self._h, *a), 9, 9)

    def relax_stats(self):
        """of the last relax(): dict(rounds, fell, los, priced)"""
        return _relax_stats(self._h, lambda *a: lib().rrt_plan_relax_stats(self._h, *a))

    def relax_poses(self, r2, samples, n, logs=False):
        """rrt_plan_relax_poses: Batch.relax_poses on the Dubins tree of this context's last plan(), launch and result (headings
        included) as grow_poses().  samples: (m, 3) rows (x, y, heading index).  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
        return self._grow(samples, n, logs, True, r2=r2)

    def relax_poses_ms(self):
        """time in ms of the stages of the last relax_poses(): (buckets, rounds, parents, alive and depth, order, costs) and the seed's
        three as grow_ms() gives them"""
        return _stage_ms(self._h, lambda *a: lib().rrt_plan_relax_poses_ms(self._h, *a), 9, 9)

    def relax_poses_stats(self):
        """of the last relax_poses(): dict(rounds, fell, sweeps, words)"""
        return _relax_stats(self._h, lambda *a: lib().rrt_plan_relax_poses_stats(self._h, *a), POSE_RELAX_STATS)

    def plan_batch(self, queries, ns):
        """rrt_plan_batch: Q independent queries on this context's grid in one call (RRTStandard / RRTStar; an Informed
        query stops at RRT_NEED_UNITBALL -- use Batch for the staged hand-over).  Returns (rc, [ResultArrays])."""
        Q = len(queries)
        qarr = (Query * Q)(*queries)
        res = [ResultArrays(int(n)) for n in ns]
        rarr = (Result * Q)(*[r.c for r in res])
        rc = lib().rrt_plan_batch(self._h, Q, qarr, rarr)
        _check(self._h, rc, ok=(RRT_OK, RRT_NEED_UNITBALL, RRT_E_GOAL_UNREACHABLE))
        for r, c in zip(res, rarr):
            r.c = c
        return rc, res

    # ---- primitives ----
    def prim_collisionfree(self, ab, walk=WALK_AUTO):
        """walk: which closed form of the line walk the device runs (WALK_AUTO: by the grid's size; WALK_U26: the large-grid kernel's)"""
        ab = np.ascontiguousarray(ab, dtype=np.int32).reshape(-1, 4)
        m = ab.shape[0]
        free = np.zeros(m, dtype=np.uint8)
        cells = np.zeros(m, dtype=np.int32)
        if walk == WALK_AUTO:
            _check(self._h, lib().rrt_prim_collisionfree(self._h, ab.ctypes.data, m, free.ctypes.data, cells.ctypes.data))
        else:
            _check(self._h, lib().rrt_prim_collisionfree_walk(self._h, ab.ctypes.data, m, int(walk), free.ctypes.data, cells.ctypes.data))
        return free.astype(bool), cells

    def prim_nearest_within(self, pts, xq, r2):
        pts = np.ascontiguousarray(pts, dtype=np.int32).reshape(-1, 2)
        xq = np.ascontiguousarray(xq, dtype=np.int32).reshape(-1, 2)
        m = xq.shape[0]
        nn = np.zeros(m, dtype=np.int32)
        cnt = np.zeros(m, dtype=np.int32)
        isum = np.zeros(m, dtype=np.int64)
        _check(self._h, lib().rrt_prim_nearest_within(self._h, pts.ctypes.data, pts.shape[0], xq.ctypes.data, m, int(r2),
                                                      nn.ctypes.data, cnt.ctypes.data, isum.ctypes.data))
        return nn, cnt, isum

    def prim_sqrt_u32(self, lo, count):
        out = np.zeros(count, dtype=np.float64)
        _check(self._h, lib().rrt_prim_sqrt_u32(self._h, int(lo), int(count), out.ctypes.data))
        return out

    def prim_sqrt_u24(self, lo, count):
        out = np.zeros(count, dtype=np.float64)
        _check(self._h, lib().rrt_prim_sqrt_u24(self._h, int(lo), int(count), out.ctypes.data))
        return out

    def prim_sqrt_u25(self, lo, count):
        out = np.zeros(count, dtype=np.float64)
        _check(self._h, lib().rrt_prim_sqrt_u25(self._h, int(lo), int(count), out.ctypes.data))
        return out

    def prim_sqrt_f64(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.zeros_like(x)
        _check(self._h, lib().rrt_prim_sqrt_f64(self._h, x.ctypes.data, x.size, out.ctypes.data))
        return out


class DeviceTree:
    """The device-resident vertex list of a host-driven planner (rrt_tree_*): the planner keeps its loop -- and its Python
    cost function -- on the host and asks the device once per iteration for near()[0], within() and the lines of sight."""

    def __init__(self, ctx: Context, capacity: int):
        self.ctx, self.capacity = ctx, int(capacity)
        self._h = C.c_void_p()
        _check(ctx.handle, lib().rrt_tree_create(ctx.handle, self.capacity, C.byref(self._h)))
        _adopt(ctx, self, "rrt_tree_destroy")  # closed before the context, like a batch
        self._idx = np.zeros(self.capacity, dtype=np.int32)
        self._los = np.zeros(self.capacity + 1, dtype=np.uint8)

    def close(self):
        _disown(self, "rrt_tree_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        _check(self.ctx.handle, lib().rrt_tree_reset(self._h))

    def append(self, x, y) -> int:
        j = C.c_int32(-1)
        _check(self.ctx.handle, lib().rrt_tree_append(self._h, int(x), int(y), C.byref(j)))
        return j.value

    def query(self, x, y, r2):
        """(nearest vertex, ascending indices of the vertices with d2 < r2, line of sight nearest -> (x, y),
        lines of sight of those vertices -> (x, y))"""
        nn, cnt = C.c_int32(-1), C.c_int32(0)
        _check(self.ctx.handle, lib().rrt_tree_query(self._h, int(x), int(y), int(r2), C.byref(nn), C.byref(cnt), self._idx.ctypes.data,
                                                     self._los.ctypes.data, self.capacity))
        m = cnt.value
        return nn.value, self._idx[:m].copy(), bool(self._los[0]), self._los[1:1 + m].astype(bool)


class Batch:
    """Q independent queries resident on the device (rrt_batch_*)."""

    def __init__(self, ctx: Context, Q: int, n_cap: int, logs: bool = False, serial: bool = False, team=None, team_fault: bool = False,
                 pipe: bool = True, rewire: bool = False, dubins: bool = False, pipe1: bool = True, onebody: bool = False, large_grid: bool = False):
        self.ctx, self.Q, self.n_cap, self.logs, self.dubins = ctx, int(Q), int(n_cap), logs, dubins
        self._h = C.c_void_p()
        flags = kernel_flags(logs, serial, team, team_fault, pipe, rewire, dubins, pipe1, onebody, large_grid)
        _check(ctx.handle, lib().rrt_batch_create(ctx.handle, self.Q, self.n_cap, flags, C.byref(self._h)))
        _adopt(ctx, self, "rrt_batch_destroy")
        self._n = [0] * self.Q

    def close(self):
        _disown(self, "rrt_batch_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_query(self, q, query):
        _check(self.ctx.handle, lib().rrt_batch_set_query(self._h, int(q), C.byref(query)))
        self._n[q] = query.n

    def set_unitball(self, q, unitball, ub_offset):
        ub = np.ascontiguousarray(unitball, dtype=np.float64)
        _check(self.ctx.handle, lib().rrt_batch_set_unitball(self._h, int(q), ub.ctypes.data, ub.shape[0], int(ub_offset)))

    def rearm(self):
        _check(self.ctx.handle, lib().rrt_batch_rearm(self._h))

    def launch(self):
        _check(self.ctx.handle, lib().rrt_batch_launch(self._h))

    def sync(self):
        _check(self.ctx.handle, lib().rrt_batch_sync(self._h))

    def team(self):
        """(CUs per query, launches repeated with one CU per query after a team hand-off timed out)"""
        g, f = C.c_int32(0), C.c_int32(0)
        _check(self.ctx.handle, lib().rrt_batch_team(self._h, C.byref(g), C.byref(f)))
        return g.value, f.value

    def team_info(self):
        """dict: workers per query at creation / of the last launch (128 = two shifts of 64), hand-off timeouts, launches that ran
        fewer workers than `created` (a smaller team, or one shift of two) because other launches held compute units of the device"""
        out = (C.c_int32 * 4)()
        _check(self.ctx.handle, lib().rrt_batch_team_info(self._h, C.byref(out)))
        return dict(created=out[0], last=out[1], timeouts=out[2], shrunk=out[3])

    def pipelined(self):
        """True if the last launch ran the pipelined team kernel"""
        v = C.c_int32(0)
        _check(self.ctx.handle, lib().rrt_batch_pipelined(self._h, C.byref(v)))
        return bool(v.value)

    def kernel_name(self):
        """the expansion kernel of the last launch, as rocprofv3 names it"""
        buf = C.create_string_buffer(128)
        _check(self.ctx.handle, lib().rrt_batch_kernel_name(self._h, buf, 128))
        return buf.value.decode()

    def elapsed_ms(self):
        ms = C.c_float(0)
        _check(self.ctx.handle, lib().rrt_batch_elapsed_ms(self._h, C.byref(ms)))
        return ms.value

    def get_result(self, q, arrays=True):
        res = ResultArrays(self._n[q], self.logs, headings=self.dubins) if arrays else None
        if res is None:
            res = ResultArrays.__new__(ResultArrays)
            res.n = self._n[q]
            res.c = Result()
        rc = lib().rrt_batch_get_result(self._h, int(q), C.byref(res.c))
        _check(self.ctx.handle, rc, ok=(RRT_OK, RRT_E_GOAL_UNREACHABLE))
        return res

    def connect_goals(self, q, goals):
        """rrt_batch_connect_goals: connect the goals (M, 2) to the finished tree of query q in one launch.  Returns
        (vertex int32[M], cost float64[M]): per goal the first vertex of [0, j), in stable (cost, index) order of
        cost = vcost[k] + dist(k, goal), with a free line of sight to it, and that cost; (-1, inf) where no vertex connects."""
        g, vertex, cost = _goal_arrays(goals)
        _check(self.ctx.handle, lib().rrt_batch_connect_goals(self._h, int(q), g.ctypes.data, g.shape[0], vertex.ctypes.data, cost.ctypes.data))
        return vertex, cost

    def connect_poses(self, q, poses):
        """rrt_batch_connect_poses: connect the goal poses (M, 3) = (x, y, heading index) to the finished Dubins tree of query q in one
        launch.  Returns (vertex int32[M], cost float64[M]): per pose the first vertex of [0, j), in stable (cost, index) order of
        cost = vcost[k] + length of the Dubins word from vertex k's pose to it, whose sweep is free, and that cost; (-1, inf) where
        no vertex connects."""
        g, vertex, cost = _pose_arrays(poses)
        _check(self.ctx.handle, lib().rrt_batch_connect_poses(self._h, int(q), g.ctypes.data, g.shape[0], vertex.ctypes.data, cost.ctypes.data))
        return vertex, cost

    def connect_poses_counts(self):
        """rrt_batch_connect_poses_counts: (words evaluated, sweeps run) summed over the goals of the last connect_poses"""
        out = (C.c_int64 * 2)()
        _check(self.ctx.handle, lib().rrt_batch_connect_poses_counts(self._h, C.byref(out)))
        return int(out[0]), int(out[1])

    def routes(self, q, goals, shortcut=False):
        """rrt_batch_routes + rrt_batch_routes_rows: finished routes from the start to the goals (M, 2) over the tree of query q, built
        on the device.  Returns (vertex, cost, length float64[M], offsets int64[M + 1], xy int32[(rows, 2)], ids int32[rows]): vertex
        and cost as connect_goals gives them; the route of goal g is xy[offsets[g]:offsets[g + 1]], the points root .. vertex[g] along
        the tree and then the goal, ids the tree vertices and -1 for the goal row; no rows and length inf where vertex is -1.
        shortcut=True: from each emitted row the route jumps to the farthest later row it has a free line of sight to."""
        L = lib()
        return _routes(self.ctx.handle, lambda *a: L.rrt_batch_routes(self._h, int(q), *a), lambda *a: L.rrt_batch_routes_rows(self._h, *a), goals, shortcut)

    def pose_routes(self, q, poses, points=False, shortcut=False):
        """rrt_batch_pose_routes + rrt_batch_pose_routes_rows (+ rrt_batch_pose_routes_points): finished routes from the start pose to
        the goal poses (M, 3) over the Dubins tree of query q, built on the device.  Returns (vertex, cost, length float64[M], offsets
        int64[M + 1], xyh int32[(rows, 3)], ids int32[rows]): vertex and cost as connect_poses gives them; the route of pose g is
        xyh[offsets[g]:offsets[g + 1]], the poses root .. vertex[g] along the tree and then the goal pose, ids the tree vertices and -1
        for the goal row; no rows and length inf where vertex is -1; length == cost bit for bit elsewhere.  points=True: two more,
        (point_offsets int64[M + 1], pts float64[(P, 2)]): the vehicle's path of pose g is pts[point_offsets[g]:point_offsets[g + 1]],
        per leg the samples every 0.5 cells of arc length of its Dubins word that the planner tested, then the goal cell.
        shortcut=True (rrt_batch_pose_shortcuts): from each kept row the route jumps to the farthest later row of the raw route to
        which the shortest Dubins word from the kept row's pose sweeps free on the active grid (the next row is never tested); the
        poses stay, the words between them change.  The rows are a subsequence of the raw rows with their ids, length the sum of the
        kept legs' words (<= cost up to rounding), the points those of the kept legs."""
        L = lib()
        call = L.rrt_batch_pose_shortcuts if shortcut else L.rrt_batch_pose_routes
        return _pose_routes(self.ctx.handle, lambda *a: call(self._h, int(q), *a), lambda *a: L.rrt_batch_pose_routes_rows(self._h, *a),
                            lambda *a: L.rrt_batch_pose_routes_points(self._h, *a), poses, points)

    def pose_shortcuts_ms(self):
        """kernel time in ms of the last pose_routes(shortcut=True): (decision, depth and scan, rows + shortcuts + scan + pack, legs +
        lengths, points)"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_pose_shortcuts_ms(self._h, *a), 5)

    def pose_routes_ms(self):
        """kernel time in ms of the last pose_routes(): (decision, depth and scan, rows + legs + lengths, points)"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_pose_routes_ms(self._h, *a), 4)

    def keep_tree(self, q):
        """rrt_batch_keep_tree: keep the finished tree of query q on the context's CURRENT grid (set_grid / select_frame since the
        query ran; same shape).  Returns alive bool[j]: the vertices whose edges up to the root are all free on it, each edge walked
        from the parent to the child.  Afterwards connect_goals / routes of query q run on the new grid over the alive vertices only
        and answer in the original vertex numbers; the tree arrays (get_result) are untouched.  Not cumulative: every call starts
        from the whole tree.  rearm, launch and set_query drop the view."""
        L = lib()
        return _keep_tree(self.ctx.handle, lambda *a: L.rrt_batch_keep_tree(self._h, int(q), *a), self.n_cap, lambda: self.get_result(q, arrays=False).j)

    def keep_pose_tree(self, q):
        """rrt_batch_keep_pose_tree: keep_tree for a Dubins batch.  An edge is the shortest Dubins word from the parent's pose to the
        child's, free if its sweep is (include/rrt_dubins.h) -- the test plan() accepted it by, so an unchanged grid keeps every
        vertex.  Returns alive bool[j].  Afterwards connect_poses of query q runs on the new grid over the alive vertices only and
        answers in the original vertex numbers; everything else as keep_tree."""
        L = lib()
        return _keep_tree(self.ctx.handle, lambda *a: L.rrt_batch_keep_pose_tree(self._h, int(q), *a), self.n_cap, lambda: self.get_result(q, arrays=False).j)

    def keep_pose_tree_resident(self, grids, k, q=0):
        """keep_pose_tree(q) on frame k of grids generated on this batch's context (oggen.DeviceGrids): the frame becomes the
        context's active grid without an upload.  RuntimeError when the frames are no longer on the device."""
        if grids.ctx is not self.ctx:
            raise ValueError("grids were generated on a different device context")
        grids.select(k)
        return self.keep_pose_tree(q)

    def keep_tree_ms(self):
        """kernel time in ms of the last keep_tree() or keep_pose_tree(): (edge test, pointer jumping, compaction)"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_keep_tree_ms(self._h, *a), 3)

    def grow(self, q, samples):
        """rrt_batch_grow: seed query q from its finished tree (the alive vertices of its keep_tree view, else the whole tree) and arm
        it for len(samples) more iterations on the context's current grid; then launch() / sync() / get_result(q) as after set_query.
        Returns (j0, old_id int32[j0], log0): the seed's vertices, the original number of each, the log row of the first new
        iteration."""
        return self._grow(q, samples, False)

    def _grow(self, q, samples, poses):
        s = _grow_samples(samples, poses)
        j0, log0 = C.c_int32(-1), C.c_int32(-1)
        old_id = np.full(self.n_cap + 1, -1, dtype=np.int32)
        call = lib().rrt_batch_grow_poses if poses else lib().rrt_batch_grow
        _check(self.ctx.handle, call(self._h, int(q), s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(log0)))
        return j0.value, old_id[:j0.value].copy(), log0.value

    def grow_poses(self, q, samples):
        """rrt_batch_grow_poses: grow() for a Dubins batch.  samples: (m, 3) rows (x, y, heading index); the seed keeps every vertex's
        heading (the view of keep_pose_tree, else the whole tree).  Returns (j0, old_id int32[j0], log0) as grow()."""
        return self._grow(q, samples, True)

    def grow_ms(self):
        """kernel time in ms of the seed stages of the last grow(): (renumbering and node slots, bitmap, cell records)"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_grow_ms(self._h, *a), 3, 3)

    def reroot(self, q, root, samples=()):
        """rrt_batch_reroot: re-root the finished tree of query q at its vertex `root` (a number of the tree as get_result gave it;
        alive, if the query has a keep_tree view), then seed and arm it like grow() for len(samples) more iterations.  The reversed
        edges are tested on the context's current grid; what hangs behind a blocked one is cut.  Returns (j0, old_id int32[j0],
        log0): the vertices of the re-rooted tree, the number each had before, the log row of the first new iteration."""
        s = _grow_samples(np.zeros((0, 2), dtype=np.int32) if len(samples) == 0 else samples)
        j0, log0 = C.c_int32(-1), C.c_int32(-1)
        old_id = np.full(self.n_cap + 1, -1, dtype=np.int32)
        _check(self.ctx.handle, lib().rrt_batch_reroot(self._h, int(q), int(root), s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(log0)))
        return j0.value, old_id[:j0.value].copy(), log0.value

    def reroot_ms(self):
        """kernel time in ms of the stages of the last reroot(): (path, reversed edges, alive and depth, order, costs) and the
        seed's three as grow_ms() gives them"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_reroot_ms(self._h, *a), 8, 8)

    def relax(self, q, r2, samples=()):
        """rrt_batch_relax: the finished tree of query q (the alive vertices of its keep_tree view, else the whole tree) relaxed to the
        shortest-path tree from its root over its own vertices and the free edges with d2 < r2 (hostprep.radius_threshold(r)), every
        old parent edge included; then seeded and armed like grow() for len(samples) more iterations.  Returns (j0, old_id int32[j0],
        log0): the vertices (all of them), the number each had before, the log row of the first new iteration."""
        s = _grow_samples(np.zeros((0, 2), dtype=np.int32) if len(samples) == 0 else samples)
        j0, log0 = C.c_int32(-1), C.c_int32(-1)
        old_id = np.full(self.n_cap + 1, -1, dtype=np.int32)
        _check(self.ctx.handle, lib().rrt_batch_relax(self._h, int(q), int(r2), s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(log0)))
        return j0.value, old_id[:j0.value].copy(), log0.value

    def relax_ms(self):
        """time in ms of the stages of the last relax(): (buckets, rounds, parents, alive and depth, order, costs) and the seed's three
        as grow_ms() gives them"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_relax_ms(self._h, *a), 9, 9)

    def relax_stats(self):
        """of the last relax(): dict(rounds, fell, los, priced) -- rounds run, vertices whose cost fell, lines of sight walked,
        candidate pairs priced"""
        return _relax_stats(self.ctx.handle, lambda *a: lib().rrt_batch_relax_stats(self._h, *a))

    def relax_poses(self, q, r2, samples=()):
        """rrt_batch_relax_poses: relax() for a Dubins batch.  The finished tree of query q (the alive vertices of its keep_pose_tree
        view, else the whole tree) relaxed to the shortest-path tree from its root over its own poses: the edges u -> v with d2 < r2
        whose shortest Dubins word sweeps free, every old parent edge included; then seeded with its headings and armed like
        grow_poses() for len(samples) more iterations.  samples: (m, 3) rows (x, y, heading index).  Returns (j0, old_id int32[j0],
        log0) as relax()."""
        s = _grow_samples(np.zeros((0, 3), dtype=np.int32) if len(samples) == 0 else samples, True)
        j0, log0 = C.c_int32(-1), C.c_int32(-1)
        old_id = np.full(self.n_cap + 1, -1, dtype=np.int32)
        _check(self.ctx.handle, lib().rrt_batch_relax_poses(self._h, int(q), int(r2), s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, C.byref(log0)))
        return j0.value, old_id[:j0.value].copy(), log0.value

    def relax_poses_ms(self):
        """time in ms of the stages of the last relax_poses(): (buckets, rounds, parents, alive and depth, order, costs) and the seed's
        three as grow_ms() gives them"""
        return _stage_ms(self.ctx.handle, lambda *a: lib().rrt_batch_relax_poses_ms(self._h, *a), 9, 9)

    def relax_poses_stats(self):
        """of the last relax_poses(): dict(rounds, fell, sweeps, words) -- rounds run, vertices whose cost fell, sweeps run, words
        evaluated"""
        return _relax_stats(self.ctx.handle, lambda *a: lib().rrt_batch_relax_poses_stats(self._h, *a), POSE_RELAX_STATS)

    def pose_routes_rows(self, rows):
        """rrt_batch_pose_routes_rows alone: (xyh, ids) of the last pose_routes() call, with shortcuts or without, which left `rows` rows"""
        xyh = np.empty((int(rows), 3), dtype=np.int32)
        ids = np.empty(int(rows), dtype=np.int32)
        _check(self.ctx.handle, lib().rrt_batch_pose_routes_rows(self._h, xyh.ctypes.data, ids.ctypes.data, int(rows)))
        return xyh, ids

    def pose_routes_points(self, points):
        """rrt_batch_pose_routes_points alone: the points of the last pose_routes(points=True) call, which left `points` points"""
        pts = np.empty((int(points), 2), dtype=np.float64)
        _check(self.ctx.handle, lib().rrt_batch_pose_routes_points(self._h, pts.ctypes.data, int(points)))
        return pts

    def routes_rows(self, rows):
        """rrt_batch_routes_rows alone: (xy, ids) of the last routes() call, which left `rows` rows"""
        xy = np.empty((int(rows), 2), dtype=np.int32)
        ids = np.empty(int(rows), dtype=np.int32)
        _check(self.ctx.handle, lib().rrt_batch_routes_rows(self._h, xy.ctypes.data, ids.ctypes.data, int(rows)))
        return xy, ids

    def debug_cycles(self, q):
        out = (C.c_uint64 * 38)()
        _check(self.ctx.handle, lib().rrt_batch_debug_cycles(self._h, int(q), C.byref(out)))
        return list(out)

    def result_block(self):
        p, nbytes = C.c_void_p(), C.c_int64()
        _check(self.ctx.handle, lib().rrt_batch_result_block(self._h, C.byref(p), C.byref(nbytes)))
        return p.value, nbytes.value

    def gather(self):
        """All-gather the result slabs of this batch over the context's communicator (asynchronous on its stream).
        Returns (device pointer of the gathered slabs, bytes per rank)."""
        p, nbytes = C.c_void_p(), C.c_int64()
        _check(self.ctx.handle, lib().rrt_gather(self._h, C.byref(p), C.byref(nbytes)))
        return p.value, nbytes.value

    def gather_fetch(self, rank, q):
        """Query q of rank `rank` out of the gathered slabs (host arrays; status / j / vgoal / found filled).  The arrays
        always hold the batch's full capacity (n_cap + 1 rows): how many rows the remote query has is only known from its
        slab, and the C side refuses to write more rows than `rows` announces."""
        res = ResultArrays(self.n_cap)
        res.c.rows = self.n_cap + 1
        _check(self.ctx.handle, lib().rrt_gather_fetch(self._h, int(rank), int(q), C.byref(res.c)))
        return res
