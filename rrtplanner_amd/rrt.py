"""Planner classes with the reference's surface, running the expansion loop on an MI355X.

Mirrors rrtplanner/rrt.py of the reference: ``RRT`` (:50), ``RRTStandard`` (:375), ``RRTStar``
(:453), ``RRTStarInformed`` (:562), ``r2norm`` (:11), ``random_point_og`` (:27).  ``plan()`` keeps
the reference's contract -- ``(networkx.DiGraph, goal_vertex)`` with node attribute ``pt`` and edge
attributes ``dist`` / ``cost`` (rrt.py:334-369) -- but its body is one call into the HIP engine
(include/rrt_hip.h) instead of the Python loop.  The numpy ``Generator`` stays the source of
randomness on the host, so the sample stream is the reference's bit for bit.

A caller-supplied ``costfn`` keeps the loop on the host (``hostloop.py``) with the device answering its per-iteration questions;
so does a problem the kernels do not take (grids beyond 2048 x 2048 -- for RRTStandard / RRTStar beyond 4096 x 4096 -- or n beyond
262 143).  ``planner.last_route`` says which way a ``plan()`` went.
There is no CPU fallback for ``plan()``: without the HIP library or a GPU it raises.
Tie policy: nearest node / goal connection pick the lowest index among
equal distance / cost (== a stable argsort in rrt.py:154 and :317).
"""
import itertools
import math
from collections.abc import Mapping
from typing import List, Tuple

import networkx as nx
import numpy as np
from tqdm import tqdm

from . import _ffi, hostprep
from .hostprep import INT64_MIN

__all__ = ["r2norm", "random_point_og", "RRT", "RRTStandard", "RRTStar", "RRTStarInformed", "TreeDiGraph"]


def _networkx_layout_ok() -> bool:
    """The fast graph construction below writes networkx's private dictionaries (`_node`, `_adj` / `_succ`, `_pred`).  Check on
    a scratch graph that they are laid out the way this file assumes (true for networkx 2.x and 3.x as tested; the reference pins
    2.6.3): plain dicts, `_succ` the same object as `_adj`, add_node / add_edge filling them as dict-of-dict with ONE shared
    attribute dict per edge.  Anything else (a future networkx) switches to the public add_node / add_edge calls."""
    try:
        g = nx.DiGraph()
        g.add_node(7, pt=1)
        g.add_edge(7, 8, dist=1.0, cost=2.0)
        return (type(g._node) is dict and type(g._adj) is dict and type(g._pred) is dict and g._succ is g._adj and g._node[7] == {"pt": 1}
                and g._adj[7][8] is g._pred[8][7] and g._adj[7][8] == {"dist": 1.0, "cost": 2.0} and g._adj[8] == {} and g._pred[7] == {})
    except Exception:
        return False


_NX_FAST = _networkx_layout_ok()


def _fill_graph_public(T, vgoal, points, parents, vcosts):
    """build_graph of the reference call by call (rrt.py:357-369), through networkx's public interface only."""
    T.add_node(vgoal, pt=points[vgoal])
    for i, p in enumerate(points):
        T.add_node(i, pt=p)
    for child, parent in parents.items():
        if parent is not None:
            T.add_edge(parent, child, dist=r2norm(points[child] - points[parent]), cost=vcosts[child])


def _fill_graph(T, vgoal, points, parents, vcosts, node_dicts=None, edge_dicts=None):
    """Fill the node / adjacency dictionaries of DiGraph `T` like build_graph of the reference (rrt.py:357-369): node order
    [vgoal, 0, 1, ...], one edge per tree link in the order of `parents`, attributes `pt` (int64 row view), `dist` (float),
    `cost` (np.float64).  The dictionaries are written directly (same dict-of-dict layout `add_node` / `add_edge` produce, one
    shared attribute dict per edge in `_succ` and `_pred`), ~3x faster than 100 000 add_node / add_edge calls;
    tests/test_host_logic.py compares it with the call-by-call construction.
    node_dicts / edge_dicts: attribute dictionaries the array-backed views of a TreeDiGraph have already handed out (by vertex /
    by child); they become the graph's own, so that whatever a caller wrote into them stays."""
    if not _NX_FAST:
        return _fill_graph_public(T, vgoal, points, parents, vcosts)
    rows = len(points)
    order = [vgoal] + [i for i in range(rows) if i != vgoal] if 0 <= vgoal < rows else [vgoal] + list(range(rows))
    node, succ, pred = T._node, T._succ, T._pred
    if node_dicts is None:
        pts = list(points)  # row views, like `for i, p in enumerate(points)`
        for v in order:
            node[v] = {"pt": pts[v]}
            succ[v] = {}
            pred[v] = {}
    else:
        for v in order:
            node[v] = node_dicts[v]
            succ[v] = {}
            pred[v] = {}
    kids = [c for c, p in parents.items() if p is not None]
    if kids:
        ch = np.asarray(kids, dtype=np.int64)
        pa = np.asarray([parents[c] for c in kids], dtype=np.int64)
        if edge_dicts is None:
            for p, c, e in zip(pa.tolist(), kids, _edge_attr_dicts(points, pa, ch, vcosts)):
                succ[p][c] = e
                pred[c][p] = e
        else:
            for p, c in zip(pa.tolist(), kids):
                e = edge_dicts[c]
                succ[p][c] = e
                pred[c][p] = e


def _edge_attr_dicts(points, pa, ch, vcosts):
    """{"dist": float, "cost": np.float64} of the edges pa[k] -> ch[k] (rrt.py:366-369)"""
    d = points[ch] - points[pa]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(np.float64)).tolist()
    return [{"dist": dd, "cost": cc} for dd, cc in zip(dist, vcosts[ch])]


class _ArrayNodeView(Mapping):
    """`T.nodes` of a TreeDiGraph that still only holds arrays: order [vgoal, 0, 1, ...], `T.nodes[v]` -> {"pt": row v}
    (rrt.py:357-361).  The attribute dictionaries are made once and become the graph's own when it is materialised; whatever this
    class does not serve itself (set algebra, data="pt", ...) goes to networkx's NodeView of the materialised graph, and so does
    every call once the graph has been materialised (a view somebody kept)."""

    __slots__ = ("_g", "_nd", "_rows", "_vgoal")

    def __init__(self, g):
        self._g = g
        self._nd = None  # attribute dictionaries by vertex, made on first use
        self._vgoal, points = g.__dict__["_lazy"][0], g.__dict__["_lazy"][1]
        self._rows = len(points)

    def _real(self):
        return nx.reportviews.NodeView(self._g)  # (reads g._node: materialises)

    def _stale(self):
        return self._g.__dict__["_lazy"] is None

    def __len__(self):
        return len(self._real()) if self._stale() else self._rows

    def __iter__(self):
        if self._stale():
            return iter(self._real())
        vgoal, rows = self._vgoal, self._rows
        return itertools.chain((vgoal,), range(vgoal), range(vgoal + 1, rows))

    def __contains__(self, v):
        if self._stale():
            return v in self._real()
        try:
            return 0 <= v < self._rows and int(v) == v
        except (TypeError, ValueError):
            return False

    def __getitem__(self, v):
        nd = self._nd
        if nd is None or self._g.__dict__["_lazy"] is None or v.__class__ is not int or v < 0:
            return self._getitem_slow(v)
        try:
            return nd[v]
        except IndexError:
            raise KeyError(v) from None

    def _getitem_slow(self, v):
        if self._stale() or isinstance(v, slice):
            return self._real()[v]  # (networkx raises its own error for slices)
        if v not in self:
            raise KeyError(v)
        if self._nd is None:
            self._nd = self._g._arr_node_dicts()
        return self._nd[int(v)]

    def __call__(self, data=False, default=None):
        if self._stale() or (data is not False and data is not True):
            return self._real()(data=data, default=default)
        return _ArrayNodeDataView(self) if data else self

    def data(self, data=True, default=None):
        return self(data=data, default=default)

    def __getattr__(self, name):  # anything else NodeView offers
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self._real(), name)

    def __repr__(self):
        return f"NodeView({tuple(self)})"


class _ArrayNodeDataView:
    __slots__ = ("_v",)

    def __init__(self, v):
        self._v = v

    def __len__(self):
        return len(self._v)

    def __iter__(self):
        v = self._v
        if v._stale():
            return iter(v._real()(data=True))
        nd = v._g._arr_node_dicts()
        return zip(v, map(nd.__getitem__, v))

    def __contains__(self, item):
        try:
            v, d = item
            return v in self._v and self._v[v] == d
        except (TypeError, ValueError):
            return False

    def __getitem__(self, v):
        return self._v[v]


class _ArrayEdgeView:
    """`T.edges` of a TreeDiGraph that still only holds arrays: the edges parent -> child in networkx's order (by source vertex in
    node order, then by insertion = child index), `T.edges[u, v]` -> {"dist", "cost"} (rrt.py:363-369), `T.edges(data=True)`.
    An edge (u, v) exists iff u is v's parent, so lookups need no table.  Everything else goes to networkx's OutEdgeView of the
    materialised graph, and so does every call once the graph has been materialised."""

    __slots__ = ("_g", "_par", "_ed")

    def __init__(self, g):
        self._g = g
        self._par = None  # parent of every live vertex as a list, the edges' attribute dictionaries by child: made on first use
        self._ed = None

    def _real(self):
        return nx.reportviews.OutEdgeView(self._g)

    def _stale(self):
        return self._g.__dict__["_lazy"] is None

    def __len__(self):
        return len(self._real()) if self._stale() else max(self._g._arr_live() - 1, 0)

    def __iter__(self):
        if self._stale():
            return iter(self._real())
        us, vs = self._g._arr_edge_order()
        return zip(us, vs)

    def _child_of(self, e):
        try:
            u, v = e
            if self._par is None:
                self._par = self._g.__dict__["_lazy"][2].tolist()
            if 1 <= v < len(self._par) and int(v) == v and self._par[int(v)] == u:
                return int(v)
        except (TypeError, ValueError):
            pass
        return None

    def __contains__(self, e):
        return (e in self._real()) if self._stale() else self._child_of(e) is not None

    def __getitem__(self, e):
        if self._g.__dict__["_lazy"] is None or isinstance(e, slice):
            return self._real()[e]
        par, ed = self._par, self._ed
        if ed is not None and e.__class__ is tuple and len(e) == 2:  # fast path: plain ints, as the views' own iteration hands out
            v = e[1]
            if v.__class__ is int and 0 < v < len(par) and par[v] == e[0]:
                return ed[v]
        c = self._child_of(e)
        if c is None:
            raise KeyError(e)
        if self._ed is None:
            self._ed = self._g._arr_edge_dicts()
        return self._ed[c]

    def __call__(self, nbunch=None, data=False, default=None):
        if self._stale() or nbunch is not None or (data is not False and data is not True):
            return self._real()(nbunch=nbunch, data=data, default=default)
        return _ArrayEdgeDataView(self) if data else self

    def data(self, data=True, default=None, nbunch=None):
        return self(nbunch=nbunch, data=data, default=default)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return getattr(self._real(), name)

    def __repr__(self):
        return f"OutEdgeView({list(self)})"


class _ArrayEdgeDataView:
    __slots__ = ("_v",)

    def __init__(self, v):
        self._v = v

    def __len__(self):
        return len(self._v)

    def __iter__(self):
        v = self._v
        if v._stale():
            return iter(v._real()(data=True))
        us, vs = v._g._arr_edge_order()
        ed = v._g._arr_edge_dicts()
        return zip(us, vs, map(ed.__getitem__, vs))

    def __contains__(self, item):
        try:
            u, v, d = item
            return (u, v) in self._v and self._v[u, v] == d
        except (TypeError, ValueError):
            return False


class TreeDiGraph(nx.DiGraph):
    """The nx.DiGraph that plan() returns, with its dictionaries filled on first use.

    At n = 50 000 building 100 000 Python dictionaries takes several times as long as the whole expansion on the device, and
    the usual next calls only need the parent pointers and the coordinates.  The instance therefore keeps the result arrays:
    route2gv / vertices_as_ndarray read them directly, and `T.nodes` / `T.edges` -- what the reference's consumers use
    (plots.py:27-29, :40-41; anim.py:101-102) -- are array-backed views (`for u, v in T.edges`, `T.edges(data=True)`, `T.nodes[v]["pt"]`,
    `T.edges[u, v]["cost"]`) that make each attribute dictionary once and never build the adjacency structure.  Anything else
    (adjacency, mutation, copy, algorithms) first materialises `_node` / `_adj` / `_succ` / `_pred` with exactly the content
    build_graph gives (tests compare both), reusing the dictionaries already handed out; from then on it is an ordinary DiGraph."""

    def __init__(self, incoming_graph_data=None, **attr):
        self.__dict__["_lazy"] = None
        super().__init__(incoming_graph_data, **attr)

    @classmethod
    def from_arrays(cls, vgoal, points, parent, vcosts):
        """points (rows, 2) int64, parent (live,) int (-1 for the root), vcosts (rows,) float64; rows >= live"""
        if not _NX_FAST:  # unknown networkx layout: an ordinary, eagerly built DiGraph (same content, see _networkx_layout_ok)
            T = nx.DiGraph()
            parents = {0: None}
            for child, p in enumerate(np.asarray(parent).tolist()):
                if child > 0:
                    parents[child] = p
            _fill_graph_public(T, int(vgoal), points, parents, vcosts)
            return T
        T = cls()
        T.__dict__["_lazy"] = (int(vgoal), points, parent, vcosts)
        return T

    def _materialise(self):
        lazy = self.__dict__.get("_lazy")
        if lazy is not None:
            self.__dict__["_lazy"] = None
            vgoal, points, parent, vcosts = lazy
            parents = {0: None}
            par = parent.tolist()
            for child in range(1, len(par)):
                parents[child] = par[child]
            _fill_graph(self, vgoal, points, parents, vcosts, self.__dict__.pop("_arr_nd", None), self.__dict__.pop("_arr_ed", None))
            for k in ("_arr_eo", "_arr_nv", "_arr_ev"):
                self.__dict__.pop(k, None)

    def __getstate__(self):  # (the cached views point back at the graph and are remade on demand)
        return {k: v for k, v in self.__dict__.items() if k not in ("_arr_nv", "_arr_ev")}

    def __setstate__(self, state):
        self.__dict__.update(state)

    # ---- array-backed views (only while the graph is lazy, and only for the plain tree: subclasses add attributes) ----
    def _arr_views(self):
        lazy = self.__dict__.get("_lazy")
        return type(self) is TreeDiGraph and lazy is not None and 0 <= lazy[0] < len(lazy[1])

    def _arr_vgoal(self):
        return self.__dict__["_lazy"][0]

    def _arr_rows(self):
        return len(self.__dict__["_lazy"][1])

    def _arr_live(self):
        return len(self.__dict__["_lazy"][2])

    def _arr_node_dicts(self):
        nd = self.__dict__.get("_arr_nd")
        if nd is None:
            nd = self.__dict__["_arr_nd"] = [{"pt": p} for p in self.__dict__["_lazy"][1]]  # row views, like build_graph's
        return nd

    def _arr_edge_dicts(self):
        """by child vertex (entry 0: the root has no edge)"""
        ed = self.__dict__.get("_arr_ed")
        if ed is None:
            _, points, parent, vcosts = self.__dict__["_lazy"]
            ch = np.arange(1, len(parent), dtype=np.int64)
            ed = self.__dict__["_arr_ed"] = [None] + _edge_attr_dicts(points, np.asarray(parent[1:], dtype=np.int64), ch, vcosts)
        return ed

    def _arr_edge_order(self):
        """(sources, targets) of all edges in networkx's iteration order: sources in node order [vgoal, 0, 1, ...], the out-edges
        of one source in insertion order (ascending child)"""
        eo = self.__dict__.get("_arr_eo")
        if eo is None:
            vgoal, _, parent, _ = self.__dict__["_lazy"]
            pa = np.asarray(parent[1:], dtype=np.int64)
            rank = np.where(pa == vgoal, 0, np.where(pa < vgoal, pa + 1, pa))
            o = np.argsort(rank * len(parent) + np.arange(len(pa)))  # (unique keys: any sort is the stable sort by rank)
            eo = self.__dict__["_arr_eo"] = (pa[o].tolist(), (o + 1).tolist())
        return eo

    @property
    def nodes(self):
        d = self.__dict__
        if d.get("_lazy") is None:
            return nx.reportviews.NodeView(self)
        v = d.get("_arr_nv")
        if v is None:
            if not self._arr_views():
                return nx.reportviews.NodeView(self)
            v = d["_arr_nv"] = _ArrayNodeView(self)
        return v

    @property
    def edges(self):
        d = self.__dict__
        if d.get("_lazy") is None:
            return nx.reportviews.OutEdgeView(self)
        v = d.get("_arr_ev")
        if v is None:
            if not self._arr_views():
                return nx.reportviews.OutEdgeView(self)
            v = d["_arr_ev"] = _ArrayEdgeView(self)
        return v

    out_edges = edges

    def root_path(self, gv):
        """[0, ..., gv] from the parent array while the graph is still lazy, else None"""
        lazy = self.__dict__.get("_lazy")
        if lazy is None:
            return None
        parent = lazy[2]
        gv = int(gv)
        if not 0 <= gv < len(parent):
            return None
        path, v = [gv], gv
        while v != 0:
            v = int(parent[v])
            if v < 0 or len(path) > len(parent):
                return None
            path.append(v)
        path.reverse()
        return path

    def lazy_points(self):
        lazy = self.__dict__.get("_lazy")
        return None if lazy is None else lazy[1]


def _lazy_dict(name, aliases=()):
    """Data descriptor for one of DiGraph's dictionaries: reading it materialises a lazy tree first.  (networkx keeps `_succ`
    as an alias of `_adj`, set together; both names are served from the same slot.)"""
    keys = ("_td" + name,) + tuple("_td" + a for a in aliases)

    def get(self):
        self._materialise()
        return self.__dict__[keys[0]]

    def set_(self, value):
        for k in keys:
            self.__dict__[k] = value

    return property(get, set_)


TreeDiGraph._node = _lazy_dict("_node")
TreeDiGraph._pred = _lazy_dict("_pred")
TreeDiGraph._adj = _lazy_dict("_adj", aliases=("_succ",))
TreeDiGraph._succ = _lazy_dict("_succ", aliases=("_adj",))


def r2norm(x) -> float:
    """2-norm of a (2,) vector (reference rrt.py:10-24)."""
    return math.sqrt(x[0] * x[0] + x[1] * x[1])


def random_point_og(og: np.ndarray, rnd_gen: np.random.Generator = None) -> np.ndarray:
    """A uniformly random free cell of the occupancy grid (reference rrt.py:27-44)."""
    free = np.argwhere(og == 0)
    draw = np.random.randint if rnd_gen is None else rnd_gen.integers
    return free[draw(low=0, high=free.shape[0])]


class RRT(object):
    """Base class: holds the grid, the sample budget and the RNG (reference rrt.py:50-86)."""

    _ALG = None
    _GROWS = False  # does grow() take this class's trees?  (RRTStandard and RRTStar)
    _STATS = ("j", "i_switch", "sum_j", "sum_cells_nn", "sum_near", "sum_cells_cand", "n_los_cand", "n_rewired", "n_propagated")  # last_stats
    _TREE_ROUTE = "kernel"  # last_route after a tree call (the Dubins planners keep none)
    _TREE = TreeDiGraph  # what _materialise returns

    def __init__(self, og: np.ndarray, n: int, costfn: callable = None, pbar: bool = True, seed: int = 0):
        self.pbar = pbar
        self.n = n
        self.free = np.argwhere(og == 0)
        self.og = og
        self._custom_cost = costfn is not None
        if costfn is None:

            def costfn(vcosts: np.ndarray, points: np.ndarray, v: int, x: np.ndarray) -> float:
                return vcosts[v] + r2norm(points[v] - x)

        self.cost = costfn
        self.not_a_point = [np.inf, np.inf]
        self.not_a_dist = np.inf
        self.rand_gen = np.random.default_rng(seed)
        # device side, created on first plan()
        self._ctx = None
        self._grid_dirty = True
        self.device_id = 0
        self.last_stats = None
        self.last_relax = None  # dict(rounds, fell, los, priced) of the last relax(); dict(rounds, fell, sweeps, words) of the last relax_poses()
        self.last_route = None  # which way the last plan() went: "kernel", "kernel-large" (grids up to 4096 x 4096) or "host" (hostloop.py)
        self._tree_resident = None  # connect_goals: "device" while the tree of the last plan() is on the device for this grid and n, "host" after the host route

    # ------------------------------------------------------------------ graph helpers
    def route2gv(self, T: nx.DiGraph, gv) -> List[int]:
        """Vertices of the shortest path root -> gv (reference rrt.py:87-107: Dijkstra on `dist`).

        In the tree `plan()` returns every vertex has one parent, so the shortest path is the unique root path and is read
        off the parent pointers; any other graph goes through networkx like the reference."""
        if isinstance(T, TreeDiGraph):
            fast = T.root_path(gv)
            if fast is not None:
                return fast
        path, v, pred = [gv], gv, T.pred
        while v != 0:
            ps = pred[v] if v in pred else ()
            if len(ps) != 1 or len(path) > len(pred):
                return nx.shortest_path(T, source=0, target=gv, weight="dist")  # not our tree (or unreachable: raises like the reference)
            (v,) = ps
            path.append(v)
        path.reverse()
        return path

    def vertices_as_ndarray(self, T: nx.DiGraph, path: list) -> np.ndarray:
        """(M-1, 2, 2) array of consecutive path segment endpoints (reference rrt.py:109-129)."""
        lazy_pts = T.lazy_points() if isinstance(T, TreeDiGraph) else None
        pts = [lazy_pts[v] for v in path] if lazy_pts is not None else [T.nodes[v]["pt"] for v in path]
        return np.array([[pts[k], pts[k + 1]] for k in range(len(path) - 1)])

    # ------------------------------------------------------------------ static primitives
    @staticmethod
    def near(points: np.ndarray, x: np.ndarray) -> np.ndarray:
        """Indices of `points` by ascending distance to `x` (reference rrt.py:131-155);
        equal distances keep index order (the canonical tie policy)."""
        return np.argsort(np.linalg.norm(points - x, axis=1), kind="stable")

    @staticmethod
    def within(points: np.ndarray, x: np.ndarray, r: float) -> np.ndarray:
        """Indices of `points` strictly closer than `r` to `x` (reference rrt.py:157-181)."""
        d = points - x
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        return np.atleast_1d(np.squeeze(np.argwhere(d2 < r * r)))

    @staticmethod
    def collisionfree(og, a, b) -> bool:
        """True iff every cell of the reference's line walk a -> b (rrt.py:183-229) is free.
        Uses the closed form of that walk (include/rrt_line.h)."""
        x0, y0, x1, y1 = int(a[0]), int(a[1]), int(b[0]), int(b[1])
        adx, ady = abs(x1 - x0), abs(y1 - y0)
        sx = 1 if x0 < x1 else -1
        sy = 1 if y0 < y1 else -1
        major, minor = max(adx, ady), min(adx, ady)
        k = np.arange(major + 1, dtype=np.int64)
        m = (2 * minor * k + major) // (2 * major) if major > 0 else np.zeros(1, dtype=np.int64)
        if adx >= ady:
            xs, ys = x0 + sx * k, y0 + sy * m
        else:
            xs, ys = x0 + sx * m, y0 + sy * k
        return not np.any(np.asarray(og)[xs, ys] != 0)

    # ------------------------------------------------------------------ sampling / setters
    def sample_all_free(self):
        """One uniform free-space sample (reference rrt.py:231-240)."""
        return self.free[self.rand_gen.choice(self.free.shape[0])]

    def plan(self, xstart: np.ndarray, xgoal: np.ndarray):
        raise NotImplementedError("This method is not implemented in the base class.")

    def set_og(self, og_new: np.ndarray):
        """New occupancy grid; free space is recomputed (reference rrt.py:261-272) and the grid
        is re-uploaded to the device before the next plan()."""
        self.og = og_new
        self.free = np.argwhere(og_new == 0)
        self._grid_dirty = True
        self._tree_resident = None

    def set_n(self, n: int):
        self.n = n
        self._tree_resident = None

    def set_og_resident(self, grids, k: int = 0):
        """Like set_og(grids.host[k]) for grids generated on this planner's device (oggen.DeviceGrids): frame k
        becomes the active grid without an upload.  Raises RuntimeError when the frames are no longer on the device
        (a set_og() + plan() or another DeviceGrids on the same context replaced them)."""
        if self._ctx is None or grids.ctx is not self._ctx:
            raise ValueError("grids were generated on a different device context: use oggen.DeviceGrids(planner.device_context(), ...)")
        grids.select(k)  # checks the context's grid generation
        self.og = grids.host[k]
        self.free = np.argwhere(self.og == 0)
        self._grid_dirty = False
        self._tree_resident = None

    def _keep_guard(self, who: str, shape=None):
        """`who` needs the tree of the last plan() on the device (and, with a shape, a grid of the shape it was planned on)"""
        if self._tree_resident is None:
            raise RuntimeError(f"{who}: no tree on the device: call plan() first (and again after set_og, set_og_resident or set_n)")
        if self._tree_resident == "host":
            raise ValueError(f"{who}: the last plan() ran on the host route (a custom cost function has no device cost; a grid or n beyond "
                             "the kernels' range is not planned on the device), so its tree is not resident on the device")
        if shape is not None and tuple(shape) != tuple(np.asarray(self.og).shape):
            raise ValueError(f"{who}: the new grid is {tuple(shape)}, the tree was planned on {tuple(np.asarray(self.og).shape)}")

    def keep_tree(self, og_new: np.ndarray) -> np.ndarray:
        """The map changed: keep the tree of the last plan() instead of planning again (rrt_plan_keep_tree).  Like set_og(og_new)
        -- og, free, the upload; a later plan() plans on og_new -- except that the tree stays on the device.  Returns alive bool[j]:
        the vertices whose every edge on the way to the root is free on og_new, each edge walked from the parent to the child
        (collisionfree(og_new, points[parent[k]], points[k])); the root's cell must be free.  From here on connect_goals, paths_to
        and routes_to take their lines of sight on og_new and consider only the alive vertices; the vertex numbers they return are
        those of the T plan() returned, and no cost changes.  No vertex alive: every goal answers -1 / inf.  Not cumulative: every
        call starts from the whole tree, so keeping it for the first map again restores every vertex.

        On a tree of RRTStar(rewire="correct") an edge may be cut even on an unchanged map: its rewire tested the edge from the
        child's side, and the line walk is not symmetric.

        ValueError if og_new has another shape than the grid of the last plan(); RuntimeError / ValueError as connect_goals."""
        return self._keep_on("keep_tree", og_new)

    def _keep_on(self, who: str, og_new) -> np.ndarray:
        """the host steps of keep_tree and of the Dubins planners' keep_pose_tree; `who` is also the context's call"""
        og_new = np.asarray(og_new)
        self._keep_guard(who, og_new.shape)
        return self._keep_call(who, og_new, True)

    def _keep_call(self, who: str, og_new, upload: bool) -> np.ndarray:
        """og_new becomes the planner's grid (upload=False: it is the context's active grid already) and the context keeps the tree on it"""
        self._tree_resident = None  # (until the call below has succeeded: a failure leaves no tree for this grid)
        self.og = og_new
        self.free = np.argwhere(og_new == 0)
        self._grid_dirty = upload
        alive = getattr(self._device() if upload else self._ctx, who)()
        self._tree_resident = "device"
        self._grow_j0 = int(alive.sum())
        return alive

    def keep_tree_resident(self, grids, k: int = 0) -> np.ndarray:
        """keep_tree(grids.host[k]) for grids generated on this planner's device (oggen.DeviceGrids): frame k becomes the active
        grid without an upload, and the tree of the last plan() is kept on it.  Raises like keep_tree and set_og_resident."""
        return self._keep_on_resident("keep_tree", grids, k)

    def _keep_on_resident(self, who: str, grids, k: int) -> np.ndarray:
        """the host steps of keep_tree_resident and of the Dubins planners' keep_pose_tree_resident; `who` is the context's call"""
        if self._ctx is None or grids.ctx is not self._ctx:
            raise ValueError("grids were generated on a different device context: use oggen.DeviceGrids(planner.device_context(), ...)")
        self._keep_guard(who + "_resident", grids.host[k].shape)
        grids.select(k)  # checks the context's grid generation; when it raises nothing has changed and the tree stays
        return self._keep_call(who, grids.host[k], False)

    def grow(self, m: int) -> Tuple[nx.DiGraph, int]:
        """Spend m more samples on the tree of the last plan() (rrt_plan_grow): after keep_tree the region behind a new obstacle has
        no vertices and its goals answer -1 / inf; grow puts vertices there again without planning from scratch.  RRT* is an anytime
        algorithm: the same call refines an uncut tree.

        The alive vertices (all of them without a keep_tree) become vertices 0 .. j0-1 of a new tree, in their original order and
        with their costs unchanged; `sampled` is the set of their cells without xstart's, so the cell of a cut vertex can be drawn
        again; then m iterations of plan()'s loop run on the current grid with m samples drawn from self.free exactly as plan()
        draws its n, and go2goal connects plan()'s xgoal.  m must fit: j0 + m <= self.n.

        Returns (T, gv) with the row contract of plan() for self.n.  self.last_grow_ids[k] is the number vertex k had in the tree
        before the call; last_stats counts the m iterations.  connect_goals, routes_to, keep_tree and a further grow work on the
        grown tree in its new numbering.

        RuntimeError / ValueError as connect_goals; ValueError when m does not fit (it names the room), for RRTStarInformed, the
        Dubins planners, rewire="correct", the large-grid route and a custom cost function."""
        return self._tree_call("grow", m)

    def reroot(self, vertex: int, m: int = 0) -> Tuple[nx.DiGraph, int]:
        """The start moved: re-root the tree of the last plan() at one of its vertices instead of planning again (rrt_plan_reroot).
        A vehicle that drives a route stands on a vertex whose number the route rows carry (routes_to, paths_to).  `vertex` is a
        number of the T the caller holds; after a keep_tree those are still the original numbers, and the vertex must be alive.

        The point of that vertex becomes the start and vertex 0 of a new tree: the parent pointers on its way to the old root are
        reversed, every other vertex keeps its parent.  The line walk is not symmetric, so each reversed edge is walked again on
        the current grid from its new parent to its new child; a vertex stays iff every edge on its new way to the root holds, so
        a blocked reversed edge cuts what hangs behind it (m > 0 repairs the gap).  The vertices are renumbered by (depth,
        previous number) and repriced from the new root down, cost[k] = cost[parent[k]] + |edge|, in the loop's own arithmetic.
        Then m more samples are spent exactly as grow(m) spends them, and go2goal connects plan()'s xgoal.  The room is checked
        with the vertices before the call: they + m <= self.n.

        Returns (T, gv) with the row contract of plan() for self.n, as grow.  self.last_grow_ids[k] is the number vertex k had
        before the call.  connect_goals, paths_to, routes_to, keep_tree, grow and a further reroot work on the re-rooted tree in its
        new numbering; a later plan() takes its own xstart as ever.

        Raises as grow; ValueError for a vertex outside the tree or one that is not alive."""
        return self._tree_call("reroot", m, vertex)

    def relax(self, r: float = None, m: int = 0) -> Tuple[nx.DiGraph, int]:
        """Choose every parent of the tree of the last plan() again (rrt_plan_relax): the vertices stay, and the tree becomes the
        shortest-path tree from its root over the graph of its own vertices with the edges that are shorter than r and free on the
        current grid, each walked from the parent to the child, and every old parent edge (however long).  That is the limit the
        rewire of RRT* approaches.  It is what makes the routes over a re-rooted tree short again: reroot reprices the edges that
        were chosen for the old start, relax chooses them for the new one.

        r defaults to self.r_rewire; RRTStandard has none and must pass it.  cost[v] = min over the candidate parents u of
        cost[u] + |uv| in the loop's own f64 sum; among the parents that give a vertex its cost the one nearest the root wins
        (smallest (cost, number)).  The vertices are renumbered by (depth, previous number) as reroot numbers them, then m more samples
        are spent exactly as grow(m) spends them, and go2goal connects plan()'s xgoal.

        Returns (T, gv) with the row contract of plan() for self.n, as grow.  self.last_grow_ids[k] is the number vertex k had before
        the call; self.last_relax holds dict(rounds, fell, los, priced): rounds run, vertices whose cost fell, lines of sight
        walked, candidate pairs priced.  Raises as grow; ValueError for a missing or non-positive r."""
        if r is None:
            r = getattr(self, "r_rewire", None)
        if r is None:
            raise ValueError("relax: this planner has no r_rewire: pass r, the radius of the candidate edges in cells")
        if not (float(r) > 0):
            raise ValueError(f"relax: r={r}")
        return self._tree_call("relax", m, hostprep.radius_threshold(r))

    def _tree_call_refusals(self, who: str):
        """the trees of this class that the tree call `who` does not take"""
        if not self._GROWS:
            if who == "relax":
                raise ValueError(f"{who}: RRTStandard and RRTStar only (an Informed tree carries ellipse state, which is not rebuilt)")
            raise ValueError(f"{who}: RRTStandard and RRTStar only (an Informed tree carries ellipse state, a Dubins tree headings, which the seed does not rebuild)"
                             if who == "grow" else
                             f"{who}: RRTStandard and RRTStar only (an Informed tree carries ellipse state, which is not rebuilt; a Dubins word is not reversible)")
        if self._custom_cost:
            raise ValueError(f"{who}: a custom cost function runs on the host route: its tree is not resident on the device")
        if _rewire_mode(getattr(self, "rewire", "reference")):
            raise ValueError(f'{who}: rewire="correct" keeps child lists on the device, which the seed does not rebuild')
        if self.last_route == "kernel-large" or self._on_the_large_grid_kernel():
            raise ValueError(f"{who}: the large-grid route (grids beyond 2048 cells a side) is not {'relaxed' if who == 'relax' else 'grown' if who == 'grow' else 're-rooted'}")

    def _draw_samples(self, m: int):
        """m samples drawn from self.free as plan() draws its n: packed cells"""
        if getattr(self, "_free_packed_of", None) is not self.free:  # (free is replaced, never edited in place: set_og / set_og_resident)
            self._free_packed, self._free_packed_of = hostprep.pack_cells(self.free), self.free
        return hostprep.draw_free_samples_packed(self.rand_gen, self._free_packed, m)

    def _tree_call(self, who: str, m: int, *lead, call=None, stats=None):
        """The calls that replace the tree of the last plan() by one seeded from it -- grow, reroot (lead: the vertex), relax (lead: the
        threshold r2), the Dubins planners' grow_poses and relax_poses, and moving.reroot_poses (lead: the vertex, the threshold r2):
        the refusals of the classes, the draws and the context's call of that name, or `call(ctx, *lead, samples, n)` for a call that is
        no method of the context; stats(ctx): what such a call leaves in last_relax"""
        self._tree_call_refusals(who)
        self._keep_guard(who)
        m = int(m)
        if m < 0:
            raise ValueError(f"{who}: m={m}")
        j0 = int(self._grow_j0)  # the vertices of the last plan() or tree call, or the alive ones of the last keep_tree / keep_pose_tree
        if j0 == 0:
            raise ValueError(f"{who}: no vertex of the tree is alive on this grid (xstart is blocked): there is nothing to grow from")
        if j0 + m > int(self.n):
            raise ValueError(f"{who}: the tree holds {j0} vertices and n={int(self.n)}: room for {int(self.n) - j0} more samples, not {m}")
        if who.startswith("reroot"):
            lead = (int(lead[0]),) + lead[1:]
            if lead[0] < 0:
                raise ValueError(f"{who}: vertex={lead[0]}")
        ctx = self._device()
        state0 = self.rand_gen.bit_generator.state
        samples = self._draw_samples(m)
        bar = tqdm(total=m) if self.pbar else None
        try:
            self._tree_resident = None  # (until the call below has succeeded, or has refused and so changed nothing)
            try:
                rc, res, j0, old_id = (call(ctx, *lead, samples, int(self.n)) if call else getattr(ctx, who)(*lead, samples, int(self.n)))
            except _ffi.RRTError as e:
                if e.code in (_ffi.RRT_E_ARG, _ffi.RRT_E_UNSUPPORTED) and not getattr(e, "seeded", True):
                    self._tree_resident = "device"
                    if who.startswith("reroot") and e.code == _ffi.RRT_E_ARG and "root=" in str(e):
                        self.rand_gen.bit_generator.state = state0  # (a refused vertex spends no draws)
                        raise ValueError(f"{who}: {str(e).split(': ', 2)[-1]}") from e
                raise
            self._tree_resident = "device"
            self.last_route = self._TREE_ROUTE or self.last_route
            self.last_grow_ids = old_id
            if who.startswith("relax"):
                self.last_relax = getattr(ctx, who + "_stats")()
            elif stats:
                self.last_relax = stats(ctx)
            self._grow_j0 = int(res.j)
            self.last_stats = {k: getattr(res, k) for k in self._STATS}
            if rc == _ffi.RRT_E_GOAL_UNREACHABLE:  # (as plan(): the grown tree is complete and resident all the same)
                raise IndexError(f"index {INT64_MIN} is out of bounds for axis 0 with size {np.asarray(self.og).shape[0]}")
            res.xg = self._grow_xg
            out = self._materialise(res)
            if bar is not None:
                bar.update(m)
        finally:
            if bar is not None:
                bar.close()
        return out

    def grow_poses(self, m: int):
        raise ValueError("grow_poses: this planner's samples are cells and its edges straight lines: use grow (pose samples belong to "
                         "RRTDubins and RRTStarDubins)")

    def relax_poses(self, r=None, m=0):
        raise ValueError("relax_poses: this planner's vertices are cells and its edges straight lines: use relax (poses belong to RRTDubins "
                         "and RRTStarDubins)")

    def device_context(self) -> "_ffi.Context":
        """The planner's device context (created on demand, without uploading a grid)."""
        if self._ctx is None:
            self._ctx = _ffi.Context(self.device_id)
            self._grid_dirty = True
        return self._ctx

    # ------------------------------------------------------------------ device plumbing
    def _device(self) -> "_ffi.Context":
        ctx = self.device_context()
        if self._grid_dirty:
            ctx.set_grid(hostprep.og_nonzero(self.og))
            self._grid_dirty = False
        return ctx

    def _run(self, alg: int, xstart, xgoal, r_rewire=None, r_goal=None, logs=False, rewire=False, large_grid=False):
        """Drive one query through the C ABI.  Returns the ResultArrays (+ ellipse log inputs)."""
        xs = hostprep.as_int_point(xstart, "xstart")
        xg = hostprep.as_int_point(xgoal, "xgoal")
        W, H = np.asarray(self.og).shape
        for p, name in ((xs, "xstart"), (xg, "xgoal")):
            if not (0 <= p[0] < W and 0 <= p[1] < H):
                raise ValueError(f"{name}={p.tolist()} lies outside the {W}x{H} occupancy grid")
        n = int(self.n)
        ctx = self._device()
        self._tree_resident = None
        bitgen = self.rand_gen.bit_generator
        state0 = bitgen.state
        samples = self._draw_samples(n)  # n draws, as rrt.py:421/502/696
        Cm = None
        if alg == _ffi.ALG_INFORMED:
            try:
                with np.errstate(all="ignore"):
                    Cm = hostprep.rotation_to_world_frame(xs, xg)
                if not np.all(np.isfinite(Cm)):
                    Cm = None
            except np.linalg.LinAlgError:
                Cm = None
        query, keep = _ffi.make_query(
            alg, n, xs, xg, samples,
            r2_rewire=hostprep.radius_threshold(r_rewire) if r_rewire is not None else 0,
            goal_d2=hostprep.goal_threshold(r_goal) if r_goal is not None else 0,
            Cmat=Cm,
        )
        kw = {"rewire": True} if rewire else {}
        if large_grid:
            kw["large_grid"] = True
        rc, res = ctx.plan(query, n, logs=logs or alg == _ffi.ALG_INFORMED, **kw)
        if rc == _ffi.RRT_NEED_UNITBALL:
            # The tree reached the goal region at iteration i_switch: from there on the reference
            # draws two uniforms per iteration instead of one free-space index (rrt.py:695-700).
            # Rewind the generator to the state after exactly i_switch free draws, then draw the
            # unit-ball stream for the remaining iterations and resume on the device.
            i_sw = res.i_switch
            bitgen.state = state0
            self._draw_samples(i_sw)
            if Cm is None:
                hostprep.rotation_to_world_frame(xs, xg)  # raises like rrt.py:609-612 would
                raise np.linalg.LinAlgError("rotation_to_world_frame is not finite (xstart == xgoal?)")
            ub = hostprep.draw_unitball(self.rand_gen, n - i_sw)
            rc = ctx.plan_resume(ub, res)
        self._tree_resident = "device"  # (also when the plan's own goal is unreachable: the tree is complete)
        self._grow_xg, self._grow_j0 = xg, int(res.j)  # (grow connects the same goal, also after a plan that did not reach it)
        if rc == _ffi.RRT_E_GOAL_UNREACHABLE:
            # rrt.py:317-318: the next argsort entry is an unfilled row -> og[INT64_MIN, ...]
            raise IndexError(f"index {INT64_MIN} is out of bounds for axis 0 with size {W}")
        res.xs, res.xg, res.Cm = xs, xg, Cm
        self.last_stats = {k: getattr(res, k) for k in self._STATS}
        return res

    def _materialise(self, res) -> Tuple[nx.DiGraph, int]:
        """points / vcosts / parents as the reference's plan() holds them after go2goal
        (rrt.py:320-325), then the DiGraph of build_graph (rrt.py:334-369)."""
        n, j, found = res.n, res.j, bool(res.found)
        rows = n + 1 if found else n
        live = j + 1 if found else j
        points = np.full((rows, 2), INT64_MIN, dtype=np.int64)  # np.full(dtype=int, fill_value=inf) rows
        vcosts = np.full((rows,), np.inf)
        points[:live] = res.pts[:live]
        vcosts[:live] = res.vcost[:live]
        vgoal = int(res.vgoal)
        if found:
            points[n] = res.xg[:2]
            vcosts[n] = vcosts[vgoal]
        return self._TREE.from_arrays(vgoal, points, np.array(res.parent[:live], dtype=np.int64), vcosts), vgoal

    def build_graph(self, vgoal, points, parents, vcosts) -> nx.DiGraph:
        """DiGraph with every row of `points` as a node (`pt`) and one edge per tree link with
        `dist` (float) and `cost` (np.float64) -- node order [vgoal, 0, 1, ...] and edge order of the
        `parents` dict, as reference rrt.py:357-369.

        (The tree plan() returns is a TreeDiGraph, which fills the same dictionaries on first use.)"""
        T = nx.DiGraph()
        _fill_graph(T, vgoal, points, parents, vcosts)
        return T

    def _plan_costfn(self, alg, xstart, xgoal):
        """plan() with a caller-supplied cost function (rrt.py:55, :70-80): the callable stays in Python, so the loop runs on the
        host (rrtplanner_amd/hostloop.py, the reference's statements incl. its real rewire block) and takes near()[0],
        within() and every line of sight from the device, once per iteration (rrt_tree_query).  Not accelerated like the
        default cost, but the same device primitives; there is no CPU path."""
        from . import hostloop

        xs = hostprep.as_int_point(xstart, "xstart")
        xg = hostprep.as_int_point(xgoal, "xgoal")
        W, H = np.asarray(self.og).shape
        for p, name in ((xs, "xstart"), (xg, "xgoal")):
            if not (0 <= p[0] < W and 0 <= p[1] < H):
                raise ValueError(f"{name}={p.tolist()} lies outside the {W}x{H} occupancy grid")
        prov = getattr(self, "_costfn_provider", None)  # (tests: a stand-in for the device primitives)
        own = prov is None
        if own:
            prov = hostloop.DeviceProvider(self._device(), int(self.n))
        bar = tqdm(total=self.n) if self.pbar else None
        try:
            vgoal, points, parents, vcosts = hostloop.plan_with_costfn(self, alg, xs, xg, prov, bar)
        finally:
            if bar is not None:
                bar.close()
            if own:
                prov.close()
        return self.build_graph(vgoal, points, parents, vcosts), vgoal

    FAST_GRID_MAX = 2048    # the expansion kernels: packed 24-bit squared distances
    FAST_N_MAX = 262143     # ... and node index + chunk tag in one 32-bit key

    def _beyond_the_kernels(self) -> bool:
        W, H = np.asarray(self.og).shape
        return W > self.FAST_GRID_MAX or H > self.FAST_GRID_MAX or int(self.n) > self.FAST_N_MAX

    LARGE_GRID_MAX = 4096        # the large-grid form of the one-CU pipeline kernel (RRT_FLAG_LARGE_GRID): 25-bit squared distances
    LARGE_GRID_KERNEL = False    # does this class run on it?  (RRTStandard and RRTStar do)

    def _on_the_large_grid_kernel(self) -> bool:
        """A grid whose longer side is 2049 to 4096 cells, planned on the device all the same: RRTStandard / RRTStar with the
        default cost and the reference's rewire, n within the kernels' range.  One CU runs the query.  It looks at the grid, not at
        _beyond_the_kernels(): whatever else that method refuses still goes to the host loop."""
        side = max(np.asarray(self.og).shape)
        return (self.LARGE_GRID_KERNEL and not self._custom_cost and self.FAST_GRID_MAX < side <= self.LARGE_GRID_MAX
                and int(self.n) <= self.FAST_N_MAX and not _rewire_mode(getattr(self, "rewire", "reference")))

    def _plan(self, alg, xstart, xgoal, **kw):
        large = self._on_the_large_grid_kernel()
        if large:
            kw["large_grid"] = True
        elif self._custom_cost or self._beyond_the_kernels():
            self.last_route = "host"
            self._tree_resident = None
            # the host-driven loop over the device primitives (hostloop.py): a custom cost function, or a problem larger than the
            # expansion kernels take (there with the default cost in numpy form) -- slower, same results, never a refusal
            if kw.get("rewire"):
                raise ValueError('rewire="correct" runs on the expansion kernels only (default cost, grids up to 2048 x 2048, n up to 262143)')
            out = self._plan_costfn(alg, xstart, xgoal)
            self._tree_resident = "host"  # (only a plan that returned: after one that raised there is no tree at all)
            return None, out
        self.last_route = "kernel-large" if large else "kernel"
        bar = tqdm(total=self.n) if self.pbar else None
        try:
            res = self._run(alg, xstart, xgoal, **kw)
            out = self._materialise(res)
            if bar is not None:
                bar.update(self.n)
        finally:
            if bar is not None:
                bar.close()
        return res, out

    # ------------------------------------------------------------------ many goals against the tree of the last plan()
    def _goal_array(self, goals) -> np.ndarray:
        g = np.asarray(goals)
        if g.ndim == 1 and g.shape == (2,):
            g = g[np.newaxis, :]
        if g.ndim != 2 or g.shape[1] != 2:
            raise ValueError(f"goals must be an (M, 2) array of grid cells (or one cell), got shape {g.shape}")
        if not np.issubdtype(g.dtype, np.integer):
            gf = np.asarray(g, dtype=np.float64)
            if not np.all(np.isfinite(gf)) or np.any(gf != np.floor(gf)):
                raise ValueError("goals must be integer grid cells")
            g = gf
        W, H = np.asarray(self.og).shape
        out = (g[:, 0] < 0) | (g[:, 0] >= W) | (g[:, 1] < 0) | (g[:, 1] >= H)
        if np.any(out):
            k = int(np.flatnonzero(out)[0])
            raise ValueError(f"goal {k} = {g[k].astype(np.int64).tolist()} lies outside the {W}x{H} occupancy grid")
        return g.astype(np.int64)

    def connect_goals(self, goals) -> Tuple[np.ndarray, np.ndarray]:
        """Connect many goals to the tree of this planner's last plan(), in one device call (rrt_plan_connect_goals): a tree
        grown from xstart serves every goal, so routes to more goals need no second plan().

        goals: (M, 2) integer cells (a single cell is M = 1).  Returns (vertex int32[M], cost float64[M]): per goal what go2goal
        (rrt.py:311-319) decides over the tree vertices [0, j) -- the tree before the goal row of plan()'s own xgoal -- i.e. the
        first vertex, in stable (cost, index) order of cost = vcosts[k] + dist(k, goal), with a free line of sight to the goal,
        and that cost.  For plan()'s own xgoal this is the parent and the cost of its goal vertex.  Where no vertex connects
        (walled off, or the goal on an obstacle cell): vertex -1, cost inf -- the reference's fall-backs for that case (vgoal = 0,
        the IndexError) are plan()'s and are not reproduced here.

        RuntimeError before any plan() and after set_og / set_og_resident / set_n until the next plan(); ValueError for a goal
        outside the grid and when the last plan() ran on the host (a custom cost function, or a problem beyond the kernels)."""
        g = self._goal_array(goals)
        self._keep_guard("connect_goals")
        return self._device().connect_goals(g)

    def connect_poses(self, poses):
        raise ValueError("connect_poses: a goal pose (x, y, heading) belongs to the Dubins planners (RRTDubins, RRTStarDubins); the goals of "
                         "this planner are cells: use connect_goals")

    def routes_to_poses(self, poses, points=False, shortcut=False):
        raise ValueError("routes_to_poses: a goal pose (x, y, heading) belongs to the Dubins planners (RRTDubins, RRTStarDubins); the goals of "
                         "this planner are cells: use routes_to")

    def keep_pose_tree(self, og_new):
        raise ValueError("keep_pose_tree: an edge that is a Dubins word between poses belongs to the Dubins planners (RRTDubins, RRTStarDubins); "
                         "the edges of this planner are straight lines: use keep_tree")

    def keep_pose_tree_resident(self, grids, k=0):
        return self.keep_pose_tree(None)

    def paths_to(self, T: nx.DiGraph, goals) -> list:
        """Routes from xstart to many goals over the tree T of the last plan(): one connect_goals call, then per goal the (k, 2)
        array of points along the tree to the vertex the goal connects to, followed by the goal itself; None where no vertex
        connects.  (The parent walks run on the host, like route2gv.)"""
        vertex, _ = self.connect_goals(goals)
        g = np.asarray(goals).reshape(-1, 2).astype(np.int64)  # (validated by connect_goals)
        lazy_pts = T.lazy_points() if isinstance(T, TreeDiGraph) else None
        out = []
        for v, goal in zip(vertex.tolist(), g):
            if v < 0:
                out.append(None)
                continue
            path = self.route2gv(T, v)
            pts = [lazy_pts[u] for u in path] if lazy_pts is not None else [T.nodes[u]["pt"] for u in path]
            out.append(np.array(pts + [goal], dtype=np.int64).reshape(-1, 2))
        return out

    def routes_to(self, goals, shortcut: bool = False) -> Tuple[list, np.ndarray]:
        """Finished routes from xstart to many goals over the tree of the last plan(), built on the device in one call
        (rrt_plan_routes): connect_goals' decision, the parent walks, optionally line-of-sight shortcuts, and the lengths.

        Returns (routes, length): routes[g] is the (k, 2) int64 array of points xstart .. goal -- without shortcuts what paths_to
        gives -- or None where no vertex connects; length float64[M] is the sum of the legs' lengths from xstart on, inf for None.
        shortcut=True: starting at xstart, the route goes on to the farthest later point of the raw route that has a free line of
        sight (collisionfree, walked towards the goal) from where it stands; every leg stays free and the route never gets longer.
        It takes no T: the tree is the one resident on the device.  RuntimeError / ValueError as connect_goals."""
        g = self._goal_array(goals)
        self._keep_guard("routes_to")
        vertex, _, length, offsets, xy, _ = self._device().routes(g, shortcut=shortcut)
        if len(vertex) == 0:
            return [], length
        routes = np.split(xy.astype(np.int64), offsets[1:-1])  # (views of one array: no per-goal copies)
        for k in np.flatnonzero(vertex < 0).tolist():
            routes[k] = None
        return routes, length

    def go2goal(self, vcosts, points, xgoal, j, children, parents):
        """Connect the goal to the cheapest tree vertex that sees it (reference rrt.py:284-332), on the host arrays the
        caller passes -- the helper of the reference's public surface; plan() itself does this step on the device.
        Returns (vgoal, children, parents, points, vcosts) with the arrays grown by one row when a vertex was found, else
        vgoal = 0 like rrt.py:330-331.  Equal costs are tried in index order (the canonical tie policy)."""
        costs = np.array([self.cost(vcosts, points, i, xgoal) for i in range(points.shape[0])], dtype=np.float64).reshape(vcosts.shape)
        for idx in np.argsort(costs, kind="stable"):
            if self.collisionfree(self.og, points[idx], xgoal):
                vgoal = j
                points = np.concatenate((points, xgoal[np.newaxis, :]), axis=0)
                vcosts = np.concatenate((vcosts, [costs[idx]]), axis=0)
                points[vgoal], vcosts[vgoal] = xgoal, costs[idx]
                children[idx].append(vgoal)
                parents[vgoal] = idx
                return vgoal, children, parents, points, vcosts
        return int(np.argmin(np.linalg.norm(points - xgoal))), children, parents, points, vcosts


class RRTStandard(RRT):
    """Plain RRT: the parent of a new node is its nearest node (reference rrt.py:375-447)."""

    LARGE_GRID_KERNEL = True
    _GROWS = True

    def __init__(self, og: np.ndarray, n: int, costfn: callable = None, pbar=True, seed: int = 0):
        super().__init__(og, n, costfn=costfn, pbar=pbar, seed=seed)

    def plan(self, xstart: np.ndarray, xgoal: np.ndarray) -> Tuple[nx.DiGraph, int]:
        return self._plan(_ffi.ALG_STANDARD, xstart, xgoal)[1]


def _rewire_mode(rewire) -> bool:
    if rewire not in ("reference", "correct"):
        raise ValueError('rewire must be "reference" (the reference\'s behaviour, default) or "correct"')
    return rewire == "correct"


class RRTStar(RRT):
    """RRT with choose-parent inside r_rewire (reference rrt.py:453-556; its rewire step never
    fires with the default cost).

    ``rewire="correct"`` (not in the reference, default ``"reference"``) opts into a true RRT* rewire with cost propagation:
    after an insertion every near vertex that gets cheaper through the new node and sees it is re-parented, and the costs
    of its descendants are recomputed.  Trees then differ from the reference's on purpose; everything else (sampling,
    acceptance, choose-parent, go2goal, the returned graph) is unchanged."""

    LARGE_GRID_KERNEL = True
    _GROWS = True

    def __init__(self, og: np.ndarray, n: int, r_rewire: float, costfn: callable = None, pbar=True, seed: int = 0, rewire: str = "reference"):
        super().__init__(og, n, costfn=costfn, pbar=pbar, seed=seed)
        self.r_rewire = r_rewire
        self.rewire = rewire
        _rewire_mode(rewire)

    def plan(self, xstart: np.ndarray, xgoal: np.ndarray):
        return self._plan(_ffi.ALG_STAR, xstart, xgoal, r_rewire=self.r_rewire, rewire=_rewire_mode(self.rewire))[1]


class RRTStarInformed(RRT):
    """RRT* that samples the start/goal ellipse once a node lies within r_goal of the goal
    (reference rrt.py:562-758)."""

    def __init__(self, og: np.ndarray, n: int, r_rewire: float, r_goal: float, costfn: callable = None,
                 pbar: bool = True, seed: int = 0, rewire: str = "reference"):
        super().__init__(og, n, costfn=costfn, pbar=pbar, seed=seed)
        self.r_rewire = r_rewire
        self.r_goal = r_goal
        self.ellipses = {}  # j -> (xcent, major axis, minor axis, angle in degrees), for plotting
        self.rewire = rewire  # "correct": opt-in true rewire, see RRTStar
        _rewire_mode(rewire)

    def plan(self, xstart: np.ndarray, xgoal: np.ndarray):
        res, out = self._plan(_ffi.ALG_INFORMED, xstart, xgoal, r_rewire=self.r_rewire, r_goal=self.r_goal, rewire=_rewire_mode(self.rewire))
        if res is not None:  # (a custom costfn records self.ellipses in its host loop, rrt.py:701)
            self._record_ellipses(res)
        return out

    # ---- the sampler's helpers of the reference's public surface (rrt.py:579-651), on the host.  plan() draws the same
    # numbers in blocks (hostprep.draw_unitball) and applies the ellipse transform on the device.
    def unitball(self) -> np.ndarray:
        """One point of the unit disc, two uniform draws from the planner's generator (rrt.py:579-587)."""
        return hostprep.draw_unitball(self.rand_gen, 1)[0]

    def rotation_to_world_frame(self, xstart, xgoal) -> np.ndarray:
        return hostprep.rotation_to_world_frame(np.asarray(xstart), np.asarray(xgoal))

    def get_ellipse_xform(self, xstart, xgoal, cmax) -> np.ndarray:
        """C @ diag(cmax / 2, sqrt(|cmax^2 - |xstart - xgoal|^2|) / 2)   (rrt.py:615-625)"""
        d = np.asarray(xstart) - np.asarray(xgoal)
        return np.dot(self.rotation_to_world_frame(xstart, xgoal), np.diag([cmax / 2, np.sqrt(abs(cmax * cmax - np.dot(d.T, d))) / 2]))

    def sample_ellipse(self, xstart, xgoal, c, clamp=True) -> np.ndarray:
        """A sample of the ellipse with foci xstart / xgoal and path length c, clamped to the grid (rrt.py:589-599)."""
        x, y = tuple(np.dot(self.get_ellipse_xform(xstart, xgoal, c), self.unitball()) + (np.asarray(xstart) + np.asarray(xgoal)) / 2)
        if clamp:
            x = int(max(0, min(self.og.shape[0] - 1, x)))
            y = int(max(0, min(self.og.shape[1] - 1, y)))
        return np.array((x, y))

    @staticmethod
    def least_cost(vcosts, vsoln):
        """(vertex, cost) of the cheapest solution vertex, the first one among equals (rrt.py:627-633)."""
        k = int(np.argmin(vcosts[vsoln])) if len(vsoln) > 1 else 0
        return vsoln[k], vcosts[vsoln[k]]

    @staticmethod
    def rad2deg(a):
        return a * 180 / np.pi

    def get_ellipse_for_plt(self, xstart, xgoal, cmax):
        """(centre, major axis, minor axis, angle in degrees) for matplotlib's Ellipse (rrt.py:639-651)."""
        CL = self.get_ellipse_xform(xstart, xgoal, cmax)
        a, b = CL[:, 0], CL[:, 1]
        return (np.asarray(xgoal) + np.asarray(xstart)) / 2, 2 * np.linalg.norm(a), 2 * np.linalg.norm(b), self.rad2deg(np.arctan2(a[1], a[0]))

    def _record_ellipses(self, res):
        """self.ellipses[j] = get_ellipse_for_plt(...) of every ellipse iteration (rrt.py:701); a
        later iteration with the same j overwrites the value, the key keeps its first position."""
        i_sw, n = res.i_switch, res.n
        if i_sw >= n:
            return
        jl = res.j_log[i_sw:n]
        cl = res.cbest_log[i_sw:n]
        last = np.flatnonzero(np.r_[jl[1:] != jl[:-1], True])  # last iteration of each run of equal j
        xcent, maj, mnr, ang = hostprep.ellipse_plot_params(res.Cm, res.xs, res.xg, cl[last])
        for k, a, b, g in zip(jl[last].tolist(), maj, mnr, ang):
            self.ellipses[k] = (xcent.copy(), a, b, g)
