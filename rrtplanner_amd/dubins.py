"""Dubins-vehicle RRT / RRT* planners on the MI355X (BASELINE.json configs[4]).

The reference advertises a "Dubins Vehicle RRT Planner" and a "Dubins Vehicle RRT(star) Planner"
(/root/reference/README.md:12,18-19) but ships no such module, so there is NO REFERENCE PARITY
here: the semantics are this build's own (include/rrt_dubins.h).  The classes
follow the reference's planner surface -- ``RRTDubins(og, n, rho, ...)`` /
``RRTStarDubins(og, n, r_rewire, rho, ...)``, ``plan(xstart, xgoal) -> (nx.DiGraph, goal_vertex)``,
``route2gv`` -- with poses ``(x, y, h)``: an integer grid cell and one of ``n_headings`` discrete
headings (``theta = 2 pi h / n_headings``).  A tree edge is the shortest Dubins word of turning
radius ``rho`` (cells) from the parent's pose to the child's; its ``dist`` is the arc length.

Nearest vertex, near set, accept test and the choose-parent walk are the reference's
(rrt.py:418-437, :498-548) on the (x, y) part of the poses; the expansion loop runs on the device
(no CPU fallback).  The numpy geometry in this file (``dubins_shortest``, ``dubins_polyline``)
serves the host side only: edge lengths of the returned graph and polylines for plotting / path
following.  It uses libm, so it agrees with the device's fixed-order arithmetic to ~1e-12, not bit
for bit (tests/test_dubins.py compares the two).
"""
import math
from typing import Tuple

import networkx as nx
import numpy as np
from tqdm import tqdm

from . import _ffi, hostprep
from .rrt import RRT, TreeDiGraph

__all__ = ["RRTDubins", "RRTStarDubins", "dubins_shortest", "dubins_polyline", "WORDS"]

WORDS = ("LSL", "LSR", "RSL", "RSR", "RLR", "LRL")
_KINDS = {"L": 1, "S": 0, "R": -1}
_TWOPI = 2.0 * math.pi


def _mod2pi(a):
    return a - _TWOPI * np.floor(a / _TWOPI)


def dubins_shortest(x0, y0, th0, x1, y1, th1, rho):
    """Shortest Dubins word between poses (vectorised over numpy arrays).  Returns (t, p, q, length, word index into
    WORDS); t, p, q in units of rho.  Ties between words go to the first in WORDS order."""
    x0, y0, th0, x1, y1, th1 = np.broadcast_arrays(*[np.asarray(v, dtype=np.float64) for v in (x0, y0, th0, x1, y1, th1)])
    dx, dy = x1 - x0, y1 - y0
    d = np.hypot(dx, dy) / rho
    theta = _mod2pi(np.arctan2(dy, dx))
    al, be = _mod2pi(th0 - theta), _mod2pi(th1 - theta)
    sa, ca, sb, cb, cab = np.sin(al), np.cos(al), np.sin(be), np.cos(be), np.cos(al - be)
    dsq = d * d
    cands = []
    with np.errstate(invalid="ignore"):
        psq = 2 + dsq - 2 * cab + 2 * d * (sa - sb)
        tmp = np.arctan2(cb - ca, d + sa - sb)
        cands.append((psq >= 0, _mod2pi(tmp - al), np.sqrt(psq), _mod2pi(be - tmp)))
        psq = -2 + dsq + 2 * cab + 2 * d * (sa + sb)
        p = np.sqrt(psq)
        tmp = np.arctan2(-ca - cb, d + sa + sb) - np.arctan2(-2.0, p)
        cands.append((psq >= 0, _mod2pi(tmp - al), p, _mod2pi(tmp - _mod2pi(be))))
        psq = -2 + dsq + 2 * cab - 2 * d * (sa + sb)
        p = np.sqrt(psq)
        tmp = np.arctan2(ca + cb, d - sa - sb) - np.arctan2(2.0, p)
        cands.append((psq >= 0, _mod2pi(al - tmp), p, _mod2pi(be - tmp)))
        psq = 2 + dsq - 2 * cab + 2 * d * (sb - sa)
        tmp = np.arctan2(ca - cb, d - sa + sb)
        cands.append((psq >= 0, _mod2pi(al - tmp), np.sqrt(psq), _mod2pi(tmp - be)))
        tmp = (6 - dsq + 2 * cab + 2 * d * (sa - sb)) / 8
        p = _mod2pi(_TWOPI - np.arccos(tmp))
        t = _mod2pi(al - np.arctan2(ca - cb, d - sa + sb) + _mod2pi(p / 2))
        cands.append((np.abs(tmp) <= 1, t, p, _mod2pi(al - be - t + _mod2pi(p))))
        tmp = (6 - dsq + 2 * cab + 2 * d * (sb - sa)) / 8
        p = _mod2pi(_TWOPI - np.arccos(tmp))
        t = _mod2pi(-al - np.arctan2(ca - cb, d + sa - sb) + p / 2)
        cands.append((np.abs(tmp) <= 1, t, p, _mod2pi(_mod2pi(be) - al - t + _mod2pi(p))))
    best = np.full(d.shape, np.inf)
    bt, bp, bq = np.zeros(d.shape), np.zeros(d.shape), np.zeros(d.shape)
    bw = np.full(d.shape, len(WORDS), dtype=np.int64)
    for w, (ok, t, p, q) in enumerate(cands):
        s = np.where(ok, t + p + q, np.inf)
        take = s < best
        best, bt, bp, bq, bw = np.where(take, s, best), np.where(take, t, bt), np.where(take, p, bp), np.where(take, q, bq), np.where(take, w, bw)
    return bt, bp, bq, best * rho, bw


def dubins_polyline(pose0, pose1, rho, n_headings, ds=0.5):
    """(M, 2) float array of points every `ds` cells of arc length along the shortest Dubins word from pose0 to pose1
    (poses are (x, y, heading index)), end point included."""
    th0, th1 = _TWOPI * pose0[2] / n_headings, _TWOPI * pose1[2] / n_headings
    t, p, q, length, w = (float(v) for v in dubins_shortest(pose0[0], pose0[1], th0, pose1[0], pose1[1], th1, rho))
    kinds = [_KINDS[c] for c in WORDS[int(w)]]
    s = np.append(np.arange(0.0, length, ds), length) / rho
    out = np.empty((s.size, 2))
    x, y, th, start = 0.0, 0.0, th0, 0.0
    for kind, tau_len in zip(kinds, (t, p, q)):
        m = (s >= start) & (s <= start + tau_len + 1e-12)
        tau = s[m] - start
        if kind == 0:
            out[m, 0], out[m, 1] = x + np.cos(th) * tau, y + np.sin(th) * tau
            x, y = x + math.cos(th) * tau_len, y + math.sin(th) * tau_len
        else:
            out[m, 0] = x + kind * (np.sin(th + kind * tau) - math.sin(th))
            out[m, 1] = y - kind * (np.cos(th + kind * tau) - math.cos(th))
            x, y = x + kind * (math.sin(th + kind * tau_len) - math.sin(th)), y - kind * (math.cos(th + kind * tau_len) - math.cos(th))
            th = th + kind * tau_len
        start += tau_len
    return np.asarray(pose0[:2], dtype=np.float64) + out * rho


class DubinsTree(TreeDiGraph):
    """TreeDiGraph whose nodes also carry `heading` and whose edge `dist` is the Dubins arc length."""

    def _materialise(self):
        dub = self.__dict__.get("_dub")
        lazy = self.__dict__.get("_lazy")
        super()._materialise()
        if lazy is None or dub is None:
            return
        heads, rho, nh = dub
        _, points, parent, _ = lazy
        node, succ = self.__dict__["_td_node"], self.__dict__["_td_adj"]
        for v, a in node.items():
            a["heading"] = int(heads[v])
        ch = np.arange(1, len(parent))
        if ch.size:
            pa = parent[1:]
            L = dubins_shortest(points[pa, 0], points[pa, 1], _TWOPI * heads[pa] / nh, points[ch, 0], points[ch, 1], _TWOPI * heads[ch] / nh, rho)[3]
            for p, c, d in zip(pa.tolist(), ch.tolist(), L.tolist()):
                succ[p][c]["dist"] = d


class _DubinsBase(RRT):
    _STAR = False
    _STATS = ("j", "sum_j", "sum_cells_nn", "sum_near", "sum_cells_cand", "n_los_cand")  # last_stats
    _TREE_ROUTE = None
    _TREE = DubinsTree

    def __init__(self, og: np.ndarray, n: int, rho: float, n_headings: int = 64, costfn: callable = None, pbar: bool = True, seed: int = 0):
        super().__init__(og, n, costfn=costfn, pbar=pbar, seed=seed)
        if not (rho > 0) or not (1 <= int(n_headings) <= 256):
            raise ValueError("rho must be positive and 1 <= n_headings <= 256")
        self.rho = float(rho)
        self.n_headings = int(n_headings)

    def sample_all_free(self):
        """One sample pose: a uniform free cell (rrt.py:231-240) and a uniform heading index."""
        return np.append(super().sample_all_free(), self.rand_gen.integers(0, self.n_headings))

    def _pose(self, x, name):
        p = np.asarray(x)
        if p.shape != (3,):
            raise ValueError(f"{name} must be a pose (x, y, heading index)")
        xy = hostprep.as_int_point(p[:2], name)
        h = int(p[2])
        if h != p[2] or not 0 <= h < self.n_headings:
            raise ValueError(f"{name}: heading index must be an integer in [0, {self.n_headings})")
        W, H = np.asarray(self.og).shape
        if not (0 <= xy[0] < W and 0 <= xy[1] < H):
            raise ValueError(f"{name}={xy.tolist()} lies outside the {W}x{H} occupancy grid")
        return np.array([xy[0], xy[1], h], dtype=np.int64)

    def _run_dubins(self, xstart, xgoal, r_rewire=None, logs=False):
        if self._custom_cost:
            raise NotImplementedError("the Dubins planners run with the arc-length cost on the device; a Python costfn cannot be lowered")
        xs, xg = self._pose(xstart, "xstart"), self._pose(xgoal, "xgoal")
        n = int(self.n)
        ctx = self._device()
        # the sample stream: n free cells (like rrt.py:240, one block), then n heading indices
        samples = hostprep.draw_free_samples(self.rand_gen, self.free, n)
        headings = self.rand_gen.integers(0, self.n_headings, size=n)
        alg = _ffi.ALG_DUBINS_STAR if self._STAR else _ffi.ALG_DUBINS
        query, keep = _ffi.make_query(alg, n, xs, xg, samples, r2_rewire=hostprep.radius_threshold(r_rewire) if r_rewire is not None else 0,
                                      headings=headings, rho=self.rho, nh=self.n_headings)
        self._tree_resident = None
        rc, res = ctx.plan(query, n, logs=logs)
        self._tree_resident = "device"  # (also when the plan's own goal is unreachable: the tree is complete)
        self._grow_xg, self._grow_j0 = xg, int(res.j)  # (grow_poses connects the same goal pose, also after a plan that did not reach it)
        if rc == _ffi.RRT_E_GOAL_UNREACHABLE:
            raise IndexError(f"index {hostprep.INT64_MIN} is out of bounds for axis 0 with size {np.asarray(self.og).shape[0]}")  # as rrt.py:317-318
        res.xs, res.xg = xs, xg
        self.last_stats = {k: getattr(res, k) for k in self._STATS}
        return res

    def _materialise(self, res) -> Tuple[nx.DiGraph, int]:
        """The reference's graph contract (rrt.py:334-369) with poses: node attributes `pt` (int64 (2,)) and `heading` (int),
        edge attributes `dist` (arc length of the Dubins word, float) and `cost` (np.float64)."""
        T, vgoal = super()._materialise(res)
        found = bool(res.found)
        heads = np.zeros(res.n + found, dtype=np.int64)
        heads[:res.j + found] = res.head[:res.j + found]
        if found:
            heads[res.n] = res.xg[2]
        T.__dict__["_dub"] = (heads, self.rho, self.n_headings)
        return T, vgoal

    def _plan_dubins(self, xstart, xgoal, **kw):
        bar = tqdm(total=self.n) if self.pbar else None
        try:
            out = self._materialise(self._run_dubins(xstart, xgoal, **kw))
            if bar is not None:
                bar.update(self.n)
        finally:
            if bar is not None:
                bar.close()
        return out

    def connect_goals(self, goals):
        raise ValueError("connect_goals: a Dubins planner's goal is a pose and its edge a Dubins word; the many-goal kernel prices straight lines "
                         "(RRTStandard, RRTStar, RRTStarInformed only)")

    def paths_to(self, T, goals):
        return self.connect_goals(goals)

    def _pose_array(self, poses):
        """goal poses as int64 (M, 3), validated on the host: integer cells inside the grid, headings in [0, n_headings) or -1"""
        g = np.asarray(poses)
        if g.ndim == 1 and g.shape == (3,):
            g = g[np.newaxis, :]
        if g.ndim != 2 or g.shape[1] != 3:
            raise ValueError(f"poses must have shape (M, 3) or (3,), got {g.shape}")
        if g.dtype.kind not in "iu":
            gf = np.asarray(g, dtype=np.float64)
            if not np.all(np.isfinite(gf)) or np.any(gf != np.floor(gf)):
                raise ValueError("poses must be integer cells and heading indices")
            g = gf
        W, H = np.asarray(self.og).shape
        out = (g[:, 0] < 0) | (g[:, 0] >= W) | (g[:, 1] < 0) | (g[:, 1] >= H)
        if np.any(out):
            k = int(np.flatnonzero(out)[0])
            raise ValueError(f"pose {k} = {g[k].astype(np.int64).tolist()} lies outside the {W}x{H} occupancy grid")
        bad = (g[:, 2] < -1) | (g[:, 2] >= self.n_headings)
        if np.any(bad):
            k = int(np.flatnonzero(bad)[0])
            raise ValueError(f"pose {k}: heading index must be an integer in [0, {self.n_headings}), or -1 for any heading")
        return g.astype(np.int64)

    def connect_poses(self, poses):
        """Connect many goal poses to the tree of this planner's last plan(), in one device call (rrt_plan_connect_poses): the
        vehicle's cost to further poses needs no second plan().

        poses: (M, 3) integer (x, y, heading index), or one pose.  Returns (vertex int32[M], cost float64[M], heading int64[M]): per
        pose what plan() decides for its own goal pose over the tree vertices [0, j): the first vertex, in stable (cost, index) order
        of cost = vcosts[k] + length of the Dubins word from vertex k's pose to the goal pose, whose sweep is free, and that cost.
        For plan()'s own xgoal this is the parent and the cost of its goal vertex.  Nothing connects (or the goal on an obstacle
        cell): vertex -1, cost inf.  Heading -1 asks for any arrival heading: the (cost, heading)-smallest connected one of the
        n_headings poses on that cell is returned, with its heading; -1 if none connects.

        RuntimeError before any plan() and after set_og / set_og_resident / set_n until the next plan(); ValueError for a pose
        outside the grid or a heading outside [0, n_headings) other than -1."""
        g = self._pose_array(poses)
        self._keep_guard("connect_poses")
        nh = self.n_headings
        anyh = g[:, 2] < 0
        rows = np.where(anyh, nh, 1)
        start = np.concatenate([[0], np.cumsum(rows)])
        full = np.repeat(g, rows, axis=0)
        for k in np.flatnonzero(anyh).tolist():
            full[start[k]:start[k + 1], 2] = np.arange(nh)
        v, c = self._device().connect_poses(full)
        vertex, cost, heading = np.full(len(g), -1, dtype=np.int32), np.full(len(g), np.inf), g[:, 2].copy()
        for k in range(len(g)):
            vk, ck = v[start[k]:start[k + 1]], c[start[k]:start[k + 1]]
            e = int(np.argmin(ck))  # (the first among equal costs: the smallest heading)
            if vk[e] >= 0:
                vertex[k], cost[k], heading[k] = vk[e], ck[e], full[start[k] + e, 2]
        return vertex, cost, heading

    def paths_to_poses(self, T, poses):
        """Routes from xstart to many goal poses over the tree T of the last plan(): one connect_poses call, then per pose the (k, 3)
        int64 array of poses (x, y, heading index) along the tree to the vertex the goal connects to, followed by the goal pose (with
        the heading that was chosen, where -1 was asked); None where nothing connects.  (The parent walks run on the host.)"""
        vertex, _, heading = self.connect_poses(poses)
        g = self._pose_array(poses)
        lazy_pts = T.lazy_points() if isinstance(T, TreeDiGraph) else None  # (a tree that was not materialised stays so)
        heads = T.__dict__.get("_dub", (None,))[0]
        out = []
        for v, goal, h in zip(vertex.tolist(), g, heading.tolist()):
            if v < 0:
                out.append(None)
                continue
            path = self.route2gv(T, v)
            if lazy_pts is not None and heads is not None:
                rows = [(int(lazy_pts[u][0]), int(lazy_pts[u][1]), int(heads[u])) for u in path]
            else:
                rows = [(int(T.nodes[u]["pt"][0]), int(T.nodes[u]["pt"][1]), int(T.nodes[u]["heading"])) for u in path]
            out.append(np.array(rows + [(int(goal[0]), int(goal[1]), int(h))], dtype=np.int64).reshape(-1, 3))
        return out

    def poses_polyline(self, route, ds: float = 0.5) -> np.ndarray:
        """(M, 2) float polyline of the vehicle's path along a route of paths_to_poses: the Dubins word of every leg, a point every
        `ds` cells of arc length."""
        route = np.asarray(route)
        legs = [dubins_polyline(a, b, self.rho, self.n_headings, ds) for a, b in zip(route[:-1], route[1:])]
        return np.concatenate(legs) if legs else np.zeros((0, 2))

    def routes_to(self, goals, shortcut=False):
        return self.connect_goals(goals)

    def routes_to_poses(self, poses, points=False, shortcut=False):
        """Finished routes from xstart to many goal poses over the tree of the last plan(), built on the device in one call
        (rrt_plan_pose_routes): connect_poses' decision, the parent walks, the lengths and, with points=True, the path the vehicle
        drives.

        Returns (routes, length) or, with points=True, (routes, length, paths).  routes[g] is the (k, 3) int64 array of poses
        (x, y, heading index) xstart .. goal pose that paths_to_poses gives, or None where no vertex connects; length float64[M] is the
        sum of the legs' Dubins words from xstart on -- equal to connect_poses' cost bit for bit --, inf for None.  paths[g] is the
        (P, 2) float64 path: per leg the points every 0.5 cells of arc length from its start pose on, the very samples whose cells
        plan() / connect_poses / keep_pose_tree tested (floor(p + 0.5) of every point is a free cell), then the goal cell; a leg's end
        pose is the next leg's first point and is not repeated, except where a leg's length is an exact multiple of 0.5: that point
        appears twice.  None where no vertex connects.
        shortcut=True (rrt_plan_pose_shortcuts): the routes are shortened on the device.  Starting at xstart, a route goes on to the
        farthest later pose of the raw route that the shortest Dubins word from the current pose reaches with a free sweep on the
        current map (the sweep of connect_poses); the pose that follows directly is taken as it is.  Every pose that stays keeps its
        cell and heading, so routes[g] is a subsequence of the raw route that begins at xstart and ends at the goal pose; only the
        words between the poses change, and the shortest word is never longer than the legs it replaces: length <= connect_poses'
        cost up to rounding, no longer equal to it.  paths[g] is then the path along the shortened route, under the same rules.
        Heading -1 (any arrival heading) is resolved first, by one connect_poses call for those poses.  It takes no T: the tree is the
        one resident on the device.  RuntimeError / ValueError as connect_poses."""
        g = self._pose_array(poses)
        self._keep_guard("routes_to_poses")
        anyh = np.flatnonzero(g[:, 2] < 0)
        if anyh.size:
            g = g.copy()
            vertex, _, heading = self.connect_poses(g[anyh])
            g[anyh, 2] = np.where(vertex >= 0, heading, 0)  # (nothing connects under any heading: nor under heading 0)
        out = self._device().pose_routes(g, points=points, shortcut=shortcut)
        vertex, length, offsets, xyh = out[0], out[2], out[3], out[4].astype(np.int64)
        routes = [xyh[offsets[k]:offsets[k + 1]] if vertex[k] >= 0 else None for k in range(len(g))]
        if not points:
            return routes, length
        po, pts = out[6], out[7]
        return routes, length, [pts[po[k]:po[k + 1]] if vertex[k] >= 0 else None for k in range(len(g))]

    def keep_tree(self, og_new):
        raise ValueError("keep_tree: a Dubins planner's edge is a Dubins word between poses; the edge test walks straight lines "
                         "(RRTStandard, RRTStar, RRTStarInformed only)")

    def keep_tree_resident(self, grids, k=0):
        return self.keep_tree(None)

    def relax(self, r=None, m=0):
        raise ValueError("relax: the cost of a Dubins word depends on the headings at its ends, and a new parent changes the word: a "
                         "Dubins tree is not relaxed (RRTStandard and RRTStar only)")

    def keep_pose_tree(self, og_new):
        """The map changed: keep the Dubins tree of the last plan() instead of planning again (rrt_plan_keep_pose_tree).  Like
        set_og(og_new) -- og, free, the upload; a later plan() plans on og_new -- except that the tree stays on the device.  Returns
        alive bool[j]: the vertices whose every edge on the way to the root is free on og_new.  An edge is the shortest Dubins word
        from the parent's pose to the child's, swept as plan() swept it when it accepted the edge (a sample every 0.5 cells of arc
        length, each inside the grid and on a free cell, then the child's cell); the root's cell must be free.  The Dubins loop
        has no rewire, so an unchanged map keeps every vertex.  From here on connect_poses and paths_to_poses sweep on og_new and
        consider only the alive vertices; the vertex numbers they return are those of the T plan() returned, and no cost changes.
        No vertex alive: every pose answers -1 / inf.  Not cumulative: every call starts from the whole tree.

        ValueError if og_new has another shape than the grid of the last plan(); RuntimeError as connect_poses."""
        return self._keep_on("keep_pose_tree", og_new)

    def keep_pose_tree_resident(self, grids, k=0):
        """keep_pose_tree(grids.host[k]) for grids generated on this planner's device (oggen.DeviceGrids): frame k becomes the active
        grid without an upload.  Raises like keep_pose_tree and set_og_resident."""
        return self._keep_on_resident("keep_pose_tree", grids, k)

    def grow_poses(self, m: int) -> Tuple[nx.DiGraph, int]:
        """Spend m more pose samples on the Dubins tree of the last plan() (rrt_plan_grow_poses): after keep_pose_tree the region
        behind a new obstacle has no vertices and its poses answer -1 / inf; grow_poses puts vertices there again without planning
        from scratch.  The same call refines an uncut tree.

        The alive vertices (all of them without a keep_pose_tree) become vertices 0 .. j0-1 of a new tree, in their original order
        and with their costs and headings unchanged; `sampled` is the set of their cells without xstart's, so the cell of a cut
        vertex can be drawn again; then m iterations of plan()'s loop run on the current grid with m free cells and then m heading
        indices drawn from self.rand_gen exactly as plan() draws its n and n, and the goal decision connects plan()'s xgoal.  m must
        fit: j0 + m <= self.n.

        Returns (T, gv) with the row contract of plan() for self.n.  self.last_grow_ids[k] is the number vertex k had in the tree
        before the call; last_stats counts the m iterations.  connect_poses, paths_to_poses, routes_to_poses, keep_pose_tree and a
        further grow_poses work on the grown tree in its new numbering.

        RuntimeError / ValueError as connect_poses; ValueError when m does not fit (it names the room); IndexError as plan() when
        the goal pose is unreachable and rows are left (the grown tree stays resident)."""
        return self._tree_call("grow_poses", m)

    def _tree_call_refusals(self, who: str):
        if not who.endswith("_poses"):
            super()._tree_call_refusals(who)  # (grow and reroot take straight-line trees only: refused there)
        if self._custom_cost:
            raise ValueError(f"{who}: the Dubins planners run with the arc-length cost on the device; a Python costfn has no tree there")

    def _draw_samples(self, m: int):
        """m pose samples (x, y, heading index) drawn as plan() draws its n: m free cells (like rrt.py:240, one block), then m heading indices"""
        cells = hostprep.draw_free_samples(self.rand_gen, self.free, m)
        headings = self.rand_gen.integers(0, self.n_headings, size=m)
        return np.column_stack([np.asarray(cells, dtype=np.int64).reshape(m, 2), headings])

    def relax_poses(self, r: float = None, m: int = 0) -> Tuple[nx.DiGraph, int]:
        """Choose every parent of the Dubins tree of the last plan() again (rrt_plan_relax_poses): the vertices and their poses stay,
        and the tree becomes the shortest-path tree from its root over the directed graph of its own poses.  RRTDubins takes the
        nearest vertex as parent and RRTStarDubins chooses among earlier vertices only and never rewires, so their trees are far
        from it.  The word between two poses depends on the two poses alone, so it does not change with the parent's own parent.

        The candidate parents of a vertex are the vertices within r cells (d2 < hostprep.radius_threshold(r)) whose shortest Dubins
        word to it is free on the current grid, swept as plan(), connect_poses and keep_pose_tree sweep, and its old parent, however
        far.  cost[v] = min cost[u] + length of the word u -> v in the loop's own f64 sum; among the parents that give a vertex its
        cost the smallest (cost, number) wins.  The vertices are renumbered by (depth, previous number), then m more pose samples are
        spent exactly as grow_poses(m) spends them, and the goal decision connects plan()'s xgoal.

        r defaults to self.r_rewire; RRTDubins has none and must pass it.  Returns (T, gv) as grow_poses.  self.last_grow_ids[k] is
        the number vertex k had before the call; self.last_relax holds dict(rounds, fell, sweeps, words): rounds run, vertices whose
        cost fell, sweeps run, words evaluated.  connect_poses, paths_to_poses, routes_to_poses, keep_pose_tree, grow_poses and a
        further relax_poses work on the result in its new numbering.  Raises as grow_poses; ValueError for a missing or
        non-positive r."""
        if r is None:
            r = getattr(self, "r_rewire", None)
        if r is None:
            raise ValueError("relax_poses: this planner has no r_rewire: pass r, the radius of the candidate edges in cells")
        if not (float(r) > 0):
            raise ValueError(f"relax_poses: r={r}")
        return self._tree_call("relax_poses", m, hostprep.radius_threshold(r))

    def path_points(self, T: nx.DiGraph, path: list, ds: float = 0.5) -> np.ndarray:
        """(M, 2) float polyline of the vehicle's path along the vertices of `path` (from route2gv)."""
        legs = []
        for u, v in zip(path[:-1], path[1:]):
            a, b = T.nodes[u], T.nodes[v]
            legs.append(dubins_polyline((*a["pt"], a["heading"]), (*b["pt"], b["heading"]), self.rho, self.n_headings, ds))
        return np.concatenate(legs) if legs else np.zeros((0, 2))


class RRTDubins(_DubinsBase):
    """Dubins-vehicle RRT: the parent of a new pose is the nearest vertex (by cell distance), connected by the shortest
    Dubins word (the reference's RRTStandard loop, rrt.py:418-437, with Dubins edges)."""

    def plan(self, xstart: np.ndarray, xgoal: np.ndarray) -> Tuple[nx.DiGraph, int]:
        return self._plan_dubins(xstart, xgoal)


class RRTStarDubins(_DubinsBase):
    """Dubins-vehicle RRT*: choose-parent over the vertices within r_rewire cells (the reference's RRTStar loop,
    rrt.py:498-548, with Dubins edges; like there the rewire scan cannot fire)."""

    _STAR = True

    def __init__(self, og: np.ndarray, n: int, r_rewire: float, rho: float, n_headings: int = 64, costfn: callable = None, pbar: bool = True,
                 seed: int = 0):
        super().__init__(og, n, rho, n_headings=n_headings, costfn=costfn, pbar=pbar, seed=seed)
        self.r_rewire = r_rewire

    def plan(self, xstart: np.ndarray, xgoal: np.ndarray) -> Tuple[nx.DiGraph, int]:
        return self._plan_dubins(xstart, xgoal, r_rewire=self.r_rewire)
