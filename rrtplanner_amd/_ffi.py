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


_vp, _i32, _u32, _i64, _P = C.c_void_p, C.c_int32, C.c_uint32, C.c_int64, C.POINTER


def _ms(stages, *count):
    return [_P(C.c_float * stages), *count]


# The argument types of every symbol include/rrt_hip.h declares, the handle included (tests/test_capi_symbols.py checks the names
# against the header and that the library exports them).  All return int but _RESTYPE's.
_SIG = {
    "rrt_ctx_create": [_i32, _P(_vp)],
    "rrt_ctx_destroy": [_vp],
    "rrt_last_error_string": [_vp],
    "rrt_set_grid": [_vp, _vp, _i32, _i32],
    "rrt_noise_grids": [_vp, _i32, _i32, _i32, C.c_float, _i32, _vp, _vp, _vp, _vp, _vp],
    "rrt_select_frame": [_vp, _i32],
    "rrt_grid_generation": [_vp, _P(C.c_uint64)],
    "rrt_ctx_sync": [_vp],
    "rrt_comm_use_library": [C.c_char_p],
    "rrt_comm_unique_id": [_vp],
    "rrt_comm_init": [_vp, _i32, _i32, _vp],
    "rrt_comm_destroy": [_vp],
    "rrt_comm_allreduce_f64": [_vp, _vp, _i32, _i32],
    "rrt_gather": [_vp, _P(_vp), _P(_i64)],
    "rrt_gather_fetch": [_vp, _i32, _i32, _P(Result)],
    "rrt_batch_create": [_vp, _i32, _i32, _u32, _P(_vp)],
    "rrt_batch_destroy": [_vp],
    "rrt_batch_set_query": [_vp, _i32, _P(Query)],
    "rrt_batch_set_unitball": [_vp, _i32, _vp, _i32, _i32],
    "rrt_batch_rearm": [_vp],
    "rrt_batch_launch": [_vp],
    "rrt_batch_sync": [_vp],
    "rrt_batch_team": [_vp, _P(_i32), _P(_i32)],
    "rrt_batch_team_info": [_vp, _P(_i32 * 4)],
    "rrt_batch_pipelined": [_vp, _P(_i32)],
    "rrt_batch_kernel_name": [_vp, C.c_char_p, _i32],
    "rrt_batch_elapsed_ms": [_vp, _P(C.c_float)],
    "rrt_batch_get_result": [_vp, _i32, _P(Result)],
    "rrt_batch_result_block": [_vp, _P(_vp), _P(_i64)],
    "rrt_batch_debug_cycles": [_vp, _i32, _P(C.c_uint64 * 38)],
    "rrt_plan": [_vp, _P(Query), _u32, _P(Result)],
    "rrt_plan_resume": [_vp, _vp, _i32, _P(Result)],
    "rrt_plan_batch": [_vp, _i32, _P(Query), _P(Result)],
    "rrt_tree_create": [_vp, _i32, _P(_vp)],
    "rrt_tree_destroy": [_vp],
    "rrt_tree_reset": [_vp],
    "rrt_tree_append": [_vp, _i32, _i32, _P(_i32)],
    "rrt_tree_query": [_vp, _i32, _i32, _i64, _P(_i32), _P(_i32), _vp, _vp, _i32],
    "rrt_prim_collisionfree": [_vp, _vp, _i32, _vp, _vp],
    "rrt_prim_nearest_within": [_vp, _vp, _i32, _vp, _i32, _i64, _vp, _vp, _vp],
    "rrt_prim_sqrt_u32": [_vp, _u32, _u32, _vp],
    "rrt_prim_sqrt_u24": [_vp, _u32, _u32, _vp],
    "rrt_prim_sqrt_f64": [_vp, _vp, _u32, _vp],
    "rrt_prim_collisionfree_walk": [_vp, _vp, _i32, _i32, _vp, _vp],
    "rrt_prim_sqrt_u25": [_vp, _u32, _u32, _vp],
    "rrt_plan_tree_size": [_vp, _P(_i32)],  # the two tree calls without a twin
    "rrt_batch_connect_poses_counts": [_vp, _P(_i64 * 2)],
}
_RESTYPE = {"rrt_last_error_string": C.c_char_p}

# The tree calls come as rrt_batch_X / rrt_plan_X, one row each; the arguments behind the handle (and q).
# ... on the tree of a query: (b, q, args...) / (ctx, args...)
_TREE_CALLS = {
    "connect_goals": [_vp, _i32, _vp, _vp],
    "connect_poses": [_vp, _i32, _vp, _vp],
    "routes": [_vp, _i32, _u32, _vp, _vp, _vp, _vp],
    "pose_routes": [_vp, _i32, _u32, _vp, _vp, _vp, _vp, _vp],
    "pose_shortcuts": [_vp, _i32, _u32, _vp, _vp, _vp, _vp, _vp],
    "keep_tree": [_P(_i32), _vp],
    "keep_pose_tree": [_P(_i32), _vp],
}
# ... reports on the last such call: (handle, args...) in both forms
_REPORT_CALLS = {
    "routes_rows": [_vp, _vp, _i64],
    "pose_routes_rows": [_vp, _vp, _i64],
    "pose_routes_points": [_vp, _i64],
    "pose_routes_ms": _ms(4),
    "pose_shortcuts_ms": _ms(5),
    "keep_tree_ms": _ms(3),
    "grow_ms": _ms(3, _i32),
    "reroot_ms": _ms(8, _i32),
    "relax_ms": _ms(9, _i32),
    "relax_poses_ms": _ms(9, _i32),
    "relax_stats": [_P(_i64 * 4)],
    "relax_poses_stats": [_P(_i64 * 4)],
}
# ... the seed family: (b, q, lead..., samples, m, j0, old_id, int32 *log0) / (ctx, lead..., samples, m, j0, old_id, rrt_result *out)
_SEED_CALLS = {"grow": [], "grow_poses": [], "reroot": [_i32], "relax": [_i64], "relax_poses": [_i64]}
for _name, _args in _TREE_CALLS.items():
    _SIG["rrt_batch_" + _name], _SIG["rrt_plan_" + _name] = [_vp, _i32] + _args, [_vp] + _args
for _name, _args in _REPORT_CALLS.items():
    _SIG["rrt_batch_" + _name] = _SIG["rrt_plan_" + _name] = [_vp] + _args
for _name, _args in _SEED_CALLS.items():
    _SIG["rrt_batch_" + _name] = [_vp, _i32] + _args + [_vp, _i32, _P(_i32), _vp, _P(_i32)]
    _SIG["rrt_plan_" + _name] = [_vp] + _args + [_vp, _i32, _P(_i32), _vp, _P(Result)]
del _name, _args

SYMBOLS = tuple(_SIG)

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
        for name, argtypes in _SIG.items():
            fn = getattr(L, name)
            fn.argtypes = argtypes
            fn.restype = _RESTYPE.get(name, C.c_int)
        _lib = L
    return _lib


def _side_binding(prototypes):
    """For a module whose symbols stay outside SYMBOLS (moving, field, posefield): its (_lib, _tree_of).  _lib() is lib() with
    `prototypes` declared on it, once per library; a library without them is an error.  _tree_of(handle, *q) is the _Tree of a Batch
    (with its query, or without one for the reports) or a Context, with the prototypes declared."""
    bound = None

    def _lib():
        nonlocal bound
        L = lib()
        if bound is not L:
            for name, argtypes in prototypes.items():
                fn = getattr(L, name)
                fn.argtypes, fn.restype = argtypes, C.c_int
            bound = L
        return L

    def _tree_of(handle, *q):
        _lib()
        return handle._tree(*q)

    return _lib, _tree_of


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


POSE_RELAX_STATS = ("rounds", "fell", "sweeps", "words")


class _Tree:
    """How the C ABI addresses one finished tree, and the marshalling of every tree call written against it: `err` the handle the
    error string is read from, `h` the native handle, `prefix` "rrt_plan_" (the tree of a context's last plan) or "rrt_batch_"
    (then q = (query,))."""

    def __init__(self, err, h, prefix, q=()):
        self.err, self.h, self.prefix, self.q = err, h, prefix, q

    def call(self, name, *args, ok=(RRT_OK,)):
        """a call on the tree: rrt_batch_<name>(b, q, args...) / rrt_plan_<name>(ctx, args...)"""
        return _check(self.err, getattr(lib(), self.prefix + name)(self.h, *self.q, *args), ok)

    def report(self, name, *args):
        """a call that reports on the last call: (handle, args...) in both forms"""
        return _check(self.err, getattr(lib(), self.prefix + name)(self.h, *args))

    def connect(self, name, goals, cols):
        """connect_goals (cols = 2) / connect_poses (cols = 3): (vertex int32[M], cost float64[M])"""
        g, vertex, cost = _goal_arrays(goals, cols)
        self.call(name, g.ctypes.data, g.shape[0], vertex.ctypes.data, cost.ctypes.data)
        return vertex, cost

    def rows(self, name, cols, rows):
        """<name>_rows: the rows the last routes call left, (xy int32[(rows, cols)], ids int32[rows])"""
        xy = np.empty((int(rows), cols), dtype=np.int32)
        ids = np.empty(int(rows), dtype=np.int32)
        self.report(name + "_rows", xy.ctypes.data, ids.ctypes.data, int(rows))
        return xy, ids

    def points(self, points):
        """pose_routes_points: the points the last pose routes call left, float64[(points, 2)]"""
        pts = np.empty((int(points), 2), dtype=np.float64)
        self.report("pose_routes_points", pts.ctypes.data, int(points))
        return pts

    def routes(self, name, goals, cols, flags, points=False):
        """the steps of a routes call (cols = 2: name "routes") or a pose routes call (cols = 3: "pose_routes" / "pose_shortcuts"):
        `name` decides and builds the routes on the device and gives the CSR offsets, then the rows and, with points, the points are
        copied out.  (vertex, cost, length, offsets int64[M + 1], xy or xyh int32[(rows, cols)], ids int32[rows]) and with points
        (point_offsets int64[M + 1], pts float64[(P, 2)]) behind them"""
        g, vertex, cost = _goal_arrays(goals, cols)
        m = g.shape[0]
        length = np.full(m, np.inf, dtype=np.float64)
        offsets = np.zeros(m + 1, dtype=np.int64)
        point_offsets = np.zeros(m + 1, dtype=np.int64) if points else None
        pose_args = () if cols == 2 else (point_offsets.ctypes.data if points else None,)
        self.call(name, g.ctypes.data, m, flags, vertex.ctypes.data, cost.ctypes.data, length.ctypes.data, offsets.ctypes.data, *pose_args)
        out = (vertex, cost, length, offsets) + self.rows("routes" if cols == 2 else "pose_routes", cols, offsets[m])
        return out + (point_offsets, self.points(point_offsets[m])) if points else out

    def keep(self, name, size, j):
        """keep_tree / keep_pose_tree: the call fills one flag per vertex of the tree.  `size` bounds them and comes from the library:
        the capacity the batch was created with, or the tree size the library reports for the query.  j() is asked for the vertices
        of the tree after the call has accepted the query.  bool[j]"""
        alive = np.zeros(max(int(size), 1), dtype=np.uint8)
        n_alive = C.c_int32(-1)
        self.call(name, C.byref(n_alive), alive.ctypes.data)
        alive = alive[:int(j())].astype(bool)
        if int(alive.sum()) != n_alive.value:
            raise RRTError(RRT_E_HIP, f"keep_tree: {n_alive.value} vertices alive, {int(alive.sum())} flags set")
        return alive

    def seed(self, name, lead, samples, poses, rows, j0, tail, ok=(RRT_OK,)):
        """the seed family (grow, grow_poses, reroot, relax, relax_poses): `lead` its arguments ahead of the samples, `rows` the rows
        old_id may need, j0 the caller's c_int32 (it stays below 0 when the call refuses before the seed), `tail` the last argument
        (the batch's log0, the context's result).  (rc, old_id int32[j0])"""
        s = _grow_samples(samples, poses)
        old_id = np.full(int(rows) + 1, -1, dtype=np.int32)
        rc = self.call(name, *lead, s.ctypes.data, s.shape[0], C.byref(j0), old_id.ctypes.data, tail, ok=ok)
        return rc, old_id[:j0.value].copy()

    def stage_ms(self, name, stages, *count):
        """<name>_ms: the kernel time in ms of the `stages` stages of the last call it reports on, as a tuple"""
        ms = (C.c_float * stages)()
        self.report(name + "_ms", C.byref(ms), *count)
        return tuple(ms)

    def relax_stats(self, name, names=("rounds", "fell", "los", "priced")):
        out = (C.c_int64 * 4)()
        self.report(name + "_stats", C.byref(out))
        return dict(zip(names, (int(v) for v in out)))


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


class _TreeReports:
    """What Context and Batch report about their last tree call: the same methods on self._tree()."""

    def pose_shortcuts_ms(self):
        """kernel time in ms of the last pose_routes(shortcut=True): (decision, depth and scan, rows + shortcuts + scan + pack, legs +
        lengths, points)"""
        return self._tree().stage_ms("pose_shortcuts", 5)

    def pose_routes_ms(self):
        """kernel time in ms of the last pose_routes(): (decision, depth and scan, rows + legs + lengths, points)"""
        return self._tree().stage_ms("pose_routes", 4)

    def keep_tree_ms(self):
        """kernel time in ms of the last keep_tree() or keep_pose_tree(): (edge test, pointer jumping, compaction)"""
        return self._tree().stage_ms("keep_tree", 3)

    def grow_ms(self):
        """kernel time in ms of the seed stages of the last grow(): (renumbering and node slots, bitmap, cell records)"""
        return self._tree().stage_ms("grow", 3, 3)

    def reroot_ms(self):
        """kernel time in ms of the stages of the last reroot(): (path, reversed edges, alive and depth, order, costs) and the
        seed's three as grow_ms() gives them"""
        return self._tree().stage_ms("reroot", 8, 8)

    def relax_ms(self):
        """time in ms of the stages of the last relax(): (buckets, rounds, parents, alive and depth, order, costs) and the seed's three
        as grow_ms() gives them"""
        return self._tree().stage_ms("relax", 9, 9)

    def relax_stats(self):
        """of the last relax(): dict(rounds, fell, los, priced) -- rounds run, vertices whose cost fell, lines of sight walked,
        candidate pairs priced"""
        return self._tree().relax_stats("relax")

    def relax_poses_ms(self):
        """time in ms of the stages of the last relax_poses(): (buckets, rounds, parents, alive and depth, order, costs) and the seed's
        three as grow_ms() gives them"""
        return self._tree().stage_ms("relax_poses", 9, 9)

    def relax_poses_stats(self):
        """of the last relax_poses(): dict(rounds, fell, sweeps, words) -- rounds run, vertices whose cost fell, sweeps run, words
        evaluated"""
        return self._tree().relax_stats("relax_poses", POSE_RELAX_STATS)


class Context(_TreeReports):
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

    def _tree(self):
        return _Tree(self._h, self._h, "rrt_plan_")

    def connect_goals(self, goals):
        """rrt_plan_connect_goals: Batch.connect_goals on the tree of this context's last plan() / plan_resume()"""
        return self._tree().connect("connect_goals", goals, 2)

    def connect_poses(self, poses):
        """rrt_plan_connect_poses: Batch.connect_poses on the Dubins tree of this context's last plan()"""
        return self._tree().connect("connect_poses", poses, 3)

    def routes(self, goals, shortcut=False):
        """rrt_plan_routes + rrt_plan_routes_rows: Batch.routes on the tree of this context's last plan() / plan_resume()"""
        return self._tree().routes("routes", goals, 2, RRT_ROUTES_SHORTCUT if shortcut else 0)

    def pose_routes(self, poses, points=False, shortcut=False):
        """rrt_plan_pose_routes (shortcut=True: rrt_plan_pose_shortcuts) + rrt_plan_pose_routes_rows (+ rrt_plan_pose_routes_points):
        Batch.pose_routes on the Dubins tree of this context's last plan()"""
        return self._tree().routes("pose_shortcuts" if shortcut else "pose_routes", poses, 3, RRT_POSE_ROUTES_POINTS if points else 0, points)

    def _keep(self, name):
        j = C.c_int32(0)
        _check(self._h, lib().rrt_plan_tree_size(self._h, C.byref(j)))
        return self._tree().keep(name, j.value, lambda: j.value)

    def keep_tree(self):
        """rrt_plan_keep_tree: Batch.keep_tree on the tree of this context's last plan() / plan_resume()"""
        return self._keep("keep_tree")

    def keep_pose_tree(self):
        """rrt_plan_keep_pose_tree: Batch.keep_pose_tree on the Dubins tree of this context's last plan()"""
        return self._keep("keep_pose_tree")

    def _seed(self, name, lead, samples, n, logs, poses=False):
        """the seed family on the tree of the last plan, launch and result included: (rc, ResultArrays, j0, old_id int32[j0])"""
        res = ResultArrays(int(n), logs, headings=poses)
        j0 = C.c_int32(-1)
        try:
            rc, old_id = self._tree().seed(name, lead, samples, poses, n, j0, C.byref(res.c), ok=(RRT_OK, RRT_E_GOAL_UNREACHABLE))
        except RRTError as e:
            e.seeded = j0.value >= 0  # False: the call refused before the seed and changed nothing
            raise
        return rc, res, j0.value, old_id

    def grow(self, samples, n, logs=False):
        """rrt_plan_grow: Batch.grow on the tree of this context's last plan() / plan_resume(), launch and result included.  n: the
        n of that plan (the result arrays are sized by it).  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
        return self._seed("grow", (), samples, n, logs)

    def grow_poses(self, samples, n, logs=False):
        """rrt_plan_grow_poses: Batch.grow_poses on the Dubins tree of this context's last plan(), launch and result (headings
        included) as grow().  samples: (m, 3) rows (x, y, heading index).  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
        return self._seed("grow_poses", (), samples, n, logs, True)

    def reroot(self, root, samples, n, logs=False):
        """rrt_plan_reroot: Batch.reroot on the tree of this context's last plan() / plan_resume(), launch and result included.
        root: a vertex number of that tree; n: the n of that plan.  Returns (rc, ResultArrays, j0, old_id int32[j0]) as grow()."""
        return self._seed("reroot", (int(root),), samples, n, logs)

    def relax(self, r2, samples, n, logs=False):
        """rrt_plan_relax: Batch.relax on the tree of this context's last plan() / plan_resume(), launch and result included.
        r2: the threshold of the squared distance (hostprep.radius_threshold(r)); n: the n of that plan.  Returns (rc, ResultArrays, j0,
        old_id int32[j0]) as grow()."""
        return self._seed("relax", (int(r2),), samples, n, logs)

    def relax_poses(self, r2, samples, n, logs=False):
        """rrt_plan_relax_poses: Batch.relax_poses on the Dubins tree of this context's last plan(), launch and result (headings
        included) as grow_poses().  samples: (m, 3) rows (x, y, heading index).  Returns (rc, ResultArrays, j0, old_id int32[j0])."""
        return self._seed("relax_poses", (int(r2),), samples, n, logs, True)

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


class Batch(_TreeReports):
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

    def _tree(self, q=None):
        return _Tree(self.ctx.handle, self._h, "rrt_batch_", () if q is None else (int(q),))

    def connect_goals(self, q, goals):
        """rrt_batch_connect_goals: connect the goals (M, 2) to the finished tree of query q in one launch.  Returns
        (vertex int32[M], cost float64[M]): per goal the first vertex of [0, j), in stable (cost, index) order of
        cost = vcost[k] + dist(k, goal), with a free line of sight to it, and that cost; (-1, inf) where no vertex connects."""
        return self._tree(q).connect("connect_goals", goals, 2)

    def connect_poses(self, q, poses):
        """rrt_batch_connect_poses: connect the goal poses (M, 3) = (x, y, heading index) to the finished Dubins tree of query q in one
        launch.  Returns (vertex int32[M], cost float64[M]): per pose the first vertex of [0, j), in stable (cost, index) order of
        cost = vcost[k] + length of the Dubins word from vertex k's pose to it, whose sweep is free, and that cost; (-1, inf) where
        no vertex connects."""
        return self._tree(q).connect("connect_poses", poses, 3)

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
        return self._tree(q).routes("routes", goals, 2, RRT_ROUTES_SHORTCUT if shortcut else 0)

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
        return self._tree(q).routes("pose_shortcuts" if shortcut else "pose_routes", poses, 3, RRT_POSE_ROUTES_POINTS if points else 0, points)

    def _keep(self, q, name):
        return self._tree(q).keep(name, self.n_cap, lambda: self.get_result(q, arrays=False).j)

    def keep_tree(self, q):
        """rrt_batch_keep_tree: keep the finished tree of query q on the context's CURRENT grid (set_grid / select_frame since the
        query ran; same shape).  Returns alive bool[j]: the vertices whose edges up to the root are all free on it, each edge walked
        from the parent to the child.  Afterwards connect_goals / routes of query q run on the new grid over the alive vertices only
        and answer in the original vertex numbers; the tree arrays (get_result) are untouched.  Not cumulative: every call starts
        from the whole tree.  rearm, launch and set_query drop the view."""
        return self._keep(q, "keep_tree")

    def keep_pose_tree(self, q):
        """rrt_batch_keep_pose_tree: keep_tree for a Dubins batch.  An edge is the shortest Dubins word from the parent's pose to the
        child's, free if its sweep is (include/rrt_dubins.h) -- the test plan() accepted it by, so an unchanged grid keeps every
        vertex.  Returns alive bool[j].  Afterwards connect_poses of query q runs on the new grid over the alive vertices only and
        answers in the original vertex numbers; everything else as keep_tree."""
        return self._keep(q, "keep_pose_tree")

    def keep_pose_tree_resident(self, grids, k, q=0):
        """keep_pose_tree(q) on frame k of grids generated on this batch's context (oggen.DeviceGrids): the frame becomes the
        context's active grid without an upload.  RuntimeError when the frames are no longer on the device."""
        if grids.ctx is not self.ctx:
            raise ValueError("grids were generated on a different device context")
        grids.select(k)
        return self.keep_pose_tree(q)

    def _seed(self, q, name, lead, samples, poses=False):
        """the seed family on the tree of query q: (j0, old_id int32[j0], log0)"""
        j0, log0 = C.c_int32(-1), C.c_int32(-1)
        old_id = self._tree(q).seed(name, lead, samples, poses, self.n_cap, j0, C.byref(log0))[1]
        return j0.value, old_id, log0.value

    def grow(self, q, samples):
        """rrt_batch_grow: seed query q from its finished tree (the alive vertices of its keep_tree view, else the whole tree) and arm
        it for len(samples) more iterations on the context's current grid; then launch() / sync() / get_result(q) as after set_query.
        Returns (j0, old_id int32[j0], log0): the seed's vertices, the original number of each, the log row of the first new
        iteration."""
        return self._seed(q, "grow", (), samples)

    def grow_poses(self, q, samples):
        """rrt_batch_grow_poses: grow() for a Dubins batch.  samples: (m, 3) rows (x, y, heading index); the seed keeps every vertex's
        heading (the view of keep_pose_tree, else the whole tree).  Returns (j0, old_id int32[j0], log0) as grow()."""
        return self._seed(q, "grow_poses", (), samples, True)

    def reroot(self, q, root, samples=()):
        """rrt_batch_reroot: re-root the finished tree of query q at its vertex `root` (a number of the tree as get_result gave it;
        alive, if the query has a keep_tree view), then seed and arm it like grow() for len(samples) more iterations.  The reversed
        edges are tested on the context's current grid; what hangs behind a blocked one is cut.  Returns (j0, old_id int32[j0],
        log0): the vertices of the re-rooted tree, the number each had before, the log row of the first new iteration."""
        return self._seed(q, "reroot", (int(root),), samples)

    def relax(self, q, r2, samples=()):
        """rrt_batch_relax: the finished tree of query q (the alive vertices of its keep_tree view, else the whole tree) relaxed to the
        shortest-path tree from its root over its own vertices and the free edges with d2 < r2 (hostprep.radius_threshold(r)), every
        old parent edge included; then seeded and armed like grow() for len(samples) more iterations.  Returns (j0, old_id int32[j0],
        log0): the vertices (all of them), the number each had before, the log row of the first new iteration."""
        return self._seed(q, "relax", (int(r2),), samples)

    def relax_poses(self, q, r2, samples=()):
        """rrt_batch_relax_poses: relax() for a Dubins batch.  The finished tree of query q (the alive vertices of its keep_pose_tree
        view, else the whole tree) relaxed to the shortest-path tree from its root over its own poses: the edges u -> v with d2 < r2
        whose shortest Dubins word sweeps free, every old parent edge included; then seeded with its headings and armed like
        grow_poses() for len(samples) more iterations.  samples: (m, 3) rows (x, y, heading index).  Returns (j0, old_id int32[j0],
        log0) as relax()."""
        return self._seed(q, "relax_poses", (int(r2),), samples, True)

    def pose_routes_rows(self, rows):
        """rrt_batch_pose_routes_rows alone: (xyh, ids) of the last pose_routes() call, with shortcuts or without, which left `rows` rows"""
        return self._tree().rows("pose_routes", 3, rows)

    def pose_routes_points(self, points):
        """rrt_batch_pose_routes_points alone: the points of the last pose_routes(points=True) call, which left `points` points"""
        return self._tree().points(points)

    def routes_rows(self, rows):
        """rrt_batch_routes_rows alone: (xy, ids) of the last routes() call, which left `rows` rows"""
        return self._tree().rows("routes", 2, rows)

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
