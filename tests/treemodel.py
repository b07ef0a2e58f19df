"""Host model of a context with batches under keep_tree / grow / reroot / relax / connect_goals / routes, and a seeded generator of
operation sequences.

The model is built from oracle.plan, keepref, growref, rerootref, relaxref, goalref and routeref alone; nothing is shortened.  Its state is the active map
(with the grid generation: every set_grid is a new one, whatever the map holds) and, per batch and query, one of
    none     no query set
    set      a query set (or rearmed) and not launched; `buf` is the sample buffer as it stands on the device
    done     finished: the tree arrays, the generation it is known valid on (`ran`; 0: none), a view (keep_tree) or none
    armed    a grow seeded and not launched: the seed, the samples and the generation it was seeded on
For every operation apply() gives the exact expected answer or the expected refusal (Refusal: the RRT_E_* code and one word of the
message).  A refusal changes nothing in the model, with the one exception the engine has: a refused routes call still drops the
rows of the earlier one (rrt_batch_routes clears them first).

The rules are the engine's (rrt_engine.hip):
  * launch and rearm drop every view of the batch and the rows of the last routes call; a query that had a view has no grid it is
    known valid on afterwards ("replaced") until it is kept or launched again;
  * a launch runs the set and the armed queries on the active map and leaves finished ones alone; it is refused while a query is
    armed on another generation than the active one, and then nothing is dropped;
  * set_query drops the view of its query; grow uses up the view; keep_tree always starts from the whole tree and adopts the active map;
  * sync puts the query's own n back; a grow replaces rows [j0, j0 + m) of the sample buffer and rearm replays the buffer as it stands.

Operations are tuples: ("set_grid", k) ("set_query", b, q, spec) ("launch", b) ("rearm", b) ("keep", b, q) ("grow", b, q, samples)
("arm", b, q, samples) ("goals", b, q, goals) ("routes", b, q, goals, shortcut) ("rows", b) ("result", b, q); launch and grow include
the sync, "arm" is the grow call alone.

reroot and relax (rerootref, relaxref, then growref.grow as after a grow's seed) are grow-like calls with rules of their own:
("reroot", b, q, root, samples) ("reroot_arm", ...) ("relax", b, q, r2, samples) ("relax_arm", ...), the launched forms and the
calls alone as "grow" and "arm".
  * they refuse in the engine's order: the finished-tree gate, the grid ("replaced"), "nothing to grow from", "room for" -- with the
    view's count or the tree's count BEFORE the call, though a reroot may leave fewer --, then reroot's root outside [0, j) and a root
    that is not alive in the view, relax's r2 <= 0;
  * a reroot sets the query's start to the new root's cell: rearm + launch plans from it, set_query puts the query's own back, and the
    map that blocks the old start no longer empties the view; the samples go to rows [j0, j0 + m) with j0 the count AFTER the reroot;
  * an armed reroot or relax is held to the generation it was seeded on like an armed grow;
  * per batch, of grow_ms / reroot_ms / relax_ms (with relax_stats) only the one of the last seed call that ran answers (timers()).
("pose_calls", b, q): relax_poses and connect_poses on the straight-line batch, refused with RRT_E_UNSUPPORTED whatever the state."""
import numpy as np

import goalref
import growref
import keepref
import oracle
import relaxref
import rerootref
import routeref
from rrtplanner_amd import hostprep
from rrtplanner_amd.oggen import largest_free_component, perlin_occupancygrid

E_ARG, E_UNSUPPORTED = -1, -5
W, H = 96, 100  # not square, H no multiple of 32
NS = (300, 900, 1400)  # j crosses TPB = 1024 in the compaction and the 64-lane steps of the seed
ALGS = (1, 0, 1)  # RRTStar, RRTStandard, RRTStar
RR = 14
R2 = hostprep.radius_threshold(RR)
N_GOALS = 32
MAP_A, MAP_B, MAP_WALL, MAP_ROOT = 0, 1, 2, 3
SEEDS = (4, 9, 10, 12, 15, 37)  # the sequences of the GPU test: each meets the conditions of test_tree_sequences_cpu.py and grows a seed of more than 1024 vertices
PAIR = (SEEDS[0], SEEDS[3])  # the two sequences that take turns on two batches of one context
ONE_SEEDS = SEEDS[:4]  # the single-query sequences: two through Context, two through the planner classes
PROBE = np.array([(10, 10), (30, 70), (47, 50), (60, 20), (80, 90), (95, 99), (0, 0), (70, 55)], dtype=np.int32)  # the goals every query is asked for after every operation
ARMS = {"arm": "grow", "reroot_arm": "reroot", "relax_arm": "relax"}  # the seed calls alone; "grow", "reroot", "relax" include the launch and the sync
SEED_OPS = ("grow", "reroot", "relax") + tuple(ARMS)
RELAX_R = (4, 6)  # the radii of the sequences' relaxes, in cells: below the rewire radius, so the host's candidate edges stay few
ROOT_SEEDS = (109, 115, 107)  # the sequences with reroot and relax (_GenRoot), each on two of the launch shapes of treecalls.SHAPES, the first on a third (team64); test_tree_sequences_cpu.py holds them to their conditions
# Known gap: a launched grow / reroot / relax of one query while ANOTHER query of its batch is armed on an older grid.  There the call
# answers and the launch behind it is refused ("seeded"), which one expected answer per operation cannot say (Model._apply asserts).
# No single sequence gets there; of two in turns only some pairs do, and the pairs are chosen among those that do not.
ROOT_PAIR = (ROOT_SEEDS[0], ROOT_SEEDS[1])  # the two that take turns on two batches, ...
ROOT_PAIR_OPS = 45  # ... with the first 45 operations of each: the two batches cost the model what one whole sequence does
ROOT_ONE_SEEDS = (101, 102)  # the single-query sequences with reroot1 and relax1: each through Context and through the planner classes
_cache = {}


def workload():
    """(maps uint8 (4, W, H), xs, [xg per query]): two noise frames, the first one with a wall and one gap, the second one with the
    root's cell blocked; the root and the goals are free on the first three and lie in the largest free region of both frames"""
    if "workload" not in _cache:
        a = oracle.og_u8(perlin_occupancygrid(W, H, seed=1))
        b = a.copy()
        other = oracle.og_u8(perlin_occupancygrid(W, H, seed=2))
        b[:, H // 2:] = other[:, H // 2:]  # the second frame: the first one with the other half of another noise field
        wall = a.copy()
        wall[W // 2:W // 2 + 3, :] = 1
        both = largest_free_component(a) & largest_free_component(b) & (wall == 0)
        near = np.argwhere(both[:W // 3, :])
        rng = np.random.default_rng(4)
        xs = near[rng.integers(0, len(near))]
        wall[W // 2:W // 2 + 3, (xs[1] + H // 2) % H - 5:(xs[1] + H // 2) % H + 5] = 0  # the gap, away from the root's column
        cells = np.argwhere(both)
        xgs = [cells[rng.integers(0, len(cells))] for _ in NS]
        root = b.copy()
        root[xs[0], xs[1]] = 1
        maps = np.stack([a, b, wall, root])
        for m in maps[:3]:
            assert m[xs[0], xs[1]] == 0 and all(m[g[0], g[1]] == 0 for g in xgs)
        _cache["workload"] = (maps, xs, xgs)
    return _cache["workload"]


class Refusal:
    def __init__(self, code, word):
        self.code, self.word = code, word

    def __repr__(self):
        return f"Refusal({self.code}, {self.word!r})"


class Tree:
    """a finished query as get_result gives it; log0 / logs / sum_j / sum_near of the iterations of its last run"""

    def __init__(self, n, pts, parent, vcost, j, found, vgoal, status, sum_j, sum_near, log0, nearest_log, accept_log, jlog):
        self.n, self.j, self.found, self.vgoal, self.status = n, int(j), int(found), int(vgoal), int(status)
        self.rows = n + 1 if self.found else n
        self.live = self.j + self.found
        self.pts = np.asarray(pts, dtype=np.int64)
        self.parent = np.asarray(parent, dtype=np.int64)
        self.vcost = np.asarray(vcost, dtype=np.float64)
        self.sum_j, self.sum_near, self.log0 = int(sum_j), int(sum_near), log0
        self.nearest_log, self.accept_log, self.jlog = nearest_log, accept_log, jlog


class QueryState:
    def __init__(self):
        self.kind = "none"
        self.alg = self.n = self.xs = self.xg = self.buf = self.tree = self.view = self.arm = None
        self.made = frozenset()  # the reroots and relaxes the tree has been through since it was planned
        self.ran = 0
        self.version = 0
        self._probe = None


class BatchState:
    def __init__(self, Q):
        self.q = [QueryState() for _ in range(Q)]
        self.route_rows = -1
        self.route_xy = self.route_ids = None
        self.timed = None  # the last seed call that ran: ("grow" | "reroot" | "relax", fell of a relax, its j0); None: none yet


class Model:
    def __init__(self, nbatches=1, Q=3):
        self.maps, self.xs, self.xgs = workload()
        self.gen, self.map = 0, None
        self.b = [BatchState(Q) for _ in range(nbatches)]
        self.notes = []  # what the coverage conditions of the CPU test count, one dict per operation
        self._seen = set()

    @property
    def og(self):
        return self.maps[self.map]

    # ---- the pieces ----
    def _status_refusal(self, s):
        if s.kind == "none":
            return Refusal(E_ARG, "no query set")
        if s.kind in ("set", "armed"):
            return Refusal(E_ARG, "not launched")
        return None

    def _goals_refusal(self, s):
        return self._status_refusal(s) or (Refusal(E_ARG, "replaced") if s.ran != self.gen else None)

    def _touch(self, s):
        s.version += 1
        s._probe = None

    def _drop_view(self, s):
        if s.view is not None:
            s.view = None
            s.ran = 0
            self._touch(s)

    def _connect(self, s, goals):
        t = s.tree
        if s.view is not None:
            _, v, c = keepref.connect(self.og, t.pts, t.parent, t.vcost, t.j, goals)
            return v, c
        v, c, _ = goalref.connect(self.og, t.pts, t.vcost, t.j, goals)
        return v, c

    def _routes(self, s, goals, cut):
        t = s.tree
        if s.view is not None:
            return keepref.routes(self.og, t.pts, t.parent, t.vcost, t.j, goals, cut=cut)[1]
        return routeref.routes(self.og, t.pts, t.vcost, t.parent, t.j, goals, cut=cut)

    def _launch(self, B, note):
        for q, s in enumerate(B.q):
            if s.kind == "armed" and s.arm["gen"] != self.gen:
                return Refusal(E_ARG, "seeded")
        B.route_rows = -1
        for s in B.q:
            self._drop_view(s)
        ran = []
        for q, s in enumerate(B.q):
            if s.kind == "set":
                st, ro = oracle.plan(self.og, s.n, s.alg, s.xs, s.xg, s.buf, r2_rewire=R2 if s.alg else 0)
                if not np.array_equal(s.xs, self.xs):
                    note.setdefault("moved", []).append(q)
                s.made = frozenset()
                s.tree = Tree(s.n, ro.pts, ro.parent, ro.vcost, ro.j, ro.found, ro.vgoal, st, ro.sum_j, ro.sum_near, None, None, None, None)
            elif s.kind == "armed":
                a = s.arm
                g = growref.grow(self.og, s.alg, s.n, s.xg, R2 if s.alg else 0, a["pts"], a["cost"], a["par"], a["samples"])
                s.tree = Tree(s.n, g.pts, g.parent, g.vcost, g.j, g.found, g.vgoal, g.status, g.sum_j, g.sum_near, a["j0"], g.nearest_log, g.accept_log, g.jlog)
                s.arm = None
            else:
                continue
            s.kind, s.ran = "done", self.gen
            self._touch(s)
            ran.append(q)
        note["ran"] = ran
        return ran

    def _seed_refusal(self, s, m, how="grow", arg=None, note=None):
        """the refusals of grow, reroot and relax in the engine's order: the finished-tree gate, the grid, nothing to grow from, the
        room -- with the view's count or the tree's count before the call --, then the call's own"""
        r = self._goals_refusal(s)
        if r:
            return r
        count = s.tree.j if s.view is None else int(s.view.sum())
        if count == 0:
            return Refusal(E_ARG, "nothing to grow from")
        if count + m > s.n:
            if note is not None:
                note["room"] = True
            return Refusal(E_ARG, "room for")
        if how == "reroot":
            if not 0 <= arg < s.tree.j:
                return Refusal(E_ARG, "has the vertices [0,")
            if s.view is not None and not s.view[arg]:
                return Refusal(E_ARG, "is not alive")
        if how == "relax" and arg <= 0:
            return Refusal(E_ARG, "r2=")
        return None

    def grow_refused(self, b, q, m, how="grow", arg=None):
        """the refusal a grow (reroot, relax) of m samples would meet, or None: what a caller that draws its samples only for a call
        that runs needs"""
        return self._seed_refusal(self.b[b].q[q], m, how, arg)

    def _arm(self, B, q, samples, note, how="grow", arg=None):
        s = B.q[q]
        m = len(samples)
        r = self._seed_refusal(s, m, how, arg, note)
        if r:
            return r
        t = s.tree
        count = t.j if s.view is None else int(s.view.sum())
        view = self.og if s.view is not None else None
        if how == "reroot":
            R = rerootref.reroot(self.og, t.pts, t.parent, t.j, arg, og8_view=view)
            ids, p, c, par = R.ids, R.pts, R.vcost, R.parent
            note.update(root=int(arg), depth=R.d)
            s.xs = np.array(t.pts[arg], dtype=np.int64)
        elif how == "relax":
            X = relaxref.relax(self.og, t.pts, t.parent, t.vcost, t.j, arg, og8_view=view)
            ids, p, c, par = X.ids, X.pts, X.vcost, X.parent
            note.update(fell=X.fell)
        else:
            ids, p, c, par = growref.seed(t.pts, t.parent, t.vcost, t.j, og8_view=view)
        j0 = len(ids)
        note.update(view=s.view is not None, m=m, j0=j0, n=s.n, how=how, count=count, on=s.made)
        s.buf = s.buf.copy()
        s.buf[j0:j0 + m] = samples
        s.arm = dict(gen=self.gen, j0=j0, pts=p, cost=c, par=par, samples=np.asarray(samples, dtype=np.int64).reshape(-1, 2))
        s.kind = "armed"
        if how != "grow":
            s.made = s.made | {how}
        if s.view is not None:
            s.view, s.ran = None, 0
        B.route_rows = -1
        B.timed = (how, note.get("fell"), j0)
        self._touch(s)
        return dict(j0=j0, old_id=ids, log0=j0, fell=note.get("fell"))

    # ---- one operation ----
    def apply(self, op):
        note = dict(kind=op[0], map=self.map)
        out = self._apply(op, note)
        note["refused"] = isinstance(out, Refusal)
        # what answers after the operation and did not in this state before: (tree, view, map), for the checks of the CPU tests
        note["answers"] = []
        for B in self.b:
            for s in B.q:
                if s.kind == "done" and s.ran == self.gen and (id(s), s.version, self.gen) not in self._seen:
                    self._seen.add((id(s), s.version, self.gen))
                    note["answers"].append((s.tree, s.view, self.map))
        self.notes.append(note)
        return out

    def _apply(self, op, note):
        kind = op[0]
        if kind == "set_grid":
            self.gen += 1
            self.map = op[1]
            for B in self.b:
                for s in B.q:
                    s._probe = None
            return None
        B = self.b[op[1]]
        if kind == "launch":
            return self._launch(B, note)
        if kind == "rearm":
            B.route_rows = -1
            for s in B.q:
                self._drop_view(s)
                if s.kind != "none":
                    s.kind, s.tree, s.arm, s.made = "set", None, None, frozenset()
                    self._touch(s)
            return None
        if kind == "rows":
            if B.route_rows < 0:
                return Refusal(E_ARG, "no routes")
            return B.route_xy, B.route_ids
        if kind == "pose_calls":  # relax_poses and connect_poses: a straight-line batch takes neither, whatever its query's state
            return Refusal(E_UNSUPPORTED, "not a Dubins batch")
        s = B.q[op[2]]
        if kind == "set_query":
            spec = op[3]
            note["on_kept"] = s.view is not None
            self._drop_view(s)
            s.kind, s.alg, s.n, s.xg, s.buf = "set", spec["alg"], spec["n"], np.asarray(spec["xg"]), np.asarray(spec["samples"], dtype=np.int64).copy()
            s.xs = np.asarray(self.xs, dtype=np.int64)  # (a query brings its own start: a reroot's is gone)
            s.tree = s.arm = None
            s.made = frozenset()
            self._touch(s)
            return None
        if kind == "result":
            return s.tree if s.kind == "done" else Refusal(E_ARG, "has not run")
        if kind == "keep":
            r = self._status_refusal(s)
            if r:
                return r
            t = s.tree
            alive = keepref.alive(self.og, t.pts, t.parent, t.j)
            s.view, s.ran = alive, self.gen
            B.route_rows = -1
            self._touch(s)
            note.update(cut=float((~alive).mean()), alive=int(alive.sum()))
            return alive
        if kind in ARMS:
            return self._arm(B, op[2], op[-1], note, ARMS[kind], *op[3:-1])
        if kind in ("grow", "reroot", "relax"):
            a = self._arm(B, op[2], op[-1], note, kind, *op[3:-1])
            if isinstance(a, Refusal):
                return a
            ran = self._launch(B, note)
            assert not isinstance(ran, Refusal)  # (armed a moment ago on the active generation)
            a["tree"] = s.tree
            return a
        if kind == "goals":
            r = self._goals_refusal(s)
            if r:
                return r
            v, c = self._connect(s, op[3])
            note.update(live=s.view is None or bool(s.view.any()), connected=int((v >= 0).sum()), unconnected=int((v < 0).sum()))
            return v, c
        if kind == "routes":
            B.route_rows = -1  # (the engine clears the rows of the earlier call before it refuses)
            r = self._goals_refusal(s)
            if r:
                return r
            out = self._routes(s, op[3], op[4])
            B.route_rows, B.route_xy, B.route_ids = int(out[3][-1]), out[4], out[5]
            return out
        raise ValueError(kind)

    # ---- what every query answers after any operation ----
    def after(self):
        """per batch, per query: (get_result: Tree or Refusal, the probe goals call: (vertex, cost) or Refusal)"""
        out = []
        for B in self.b:
            row = []
            for s in B.q:
                if s._probe is None:
                    r = self._goals_refusal(s)
                    s._probe = r if r else self._connect(s, PROBE)
                row.append((s.tree if s.kind == "done" else Refusal(E_ARG, "has not run"), s._probe))
            out.append(row)
        return out

    def timers(self):
        """per batch, which of grow_ms / reroot_ms / relax_ms (and relax_stats) answers: only the one of the last seed call that ran.
        ("grow" | "reroot" | "relax", the relax's fell, its j0), or None while no seed call of the batch has run"""
        return [B.timed for B in self.b]


# ------------------------------------------------------------------------------------------------ the generator
class Step:
    def __init__(self, op, expect, after, timed=None):
        self.op, self.expect, self.after = op, expect, after
        self.timed = timed  # per batch: Model.timers() after the operation


class _Gen:
    """Draws one sequence operation by operation against the model, which tells it what is there to keep, cut and grow.  The order
    of the scenario blocks, the queries, the maps, the sample counts, the samples and the goals all come from the one seeded stream."""

    def __init__(self, seed, b=0, model=None):
        self.rng = np.random.default_rng(seed)
        self.m = model or Model()
        self.b = b
        self.steps = []
        self.free = [np.argwhere(g == 0) for g in self.m.maps]
        self.wall = [np.argwhere(g != 0) for g in self.m.maps]

    # draws
    def samples(self, m, k=None, special=True):
        k = self.m.map if k is None else k
        s = hostprep.draw_free_samples(self.rng, self.free[k], m)
        if special and m >= 8:  # the root's cell (accepted once: it is never in `sampled`) and an obstacle cell (never accepted)
            at = self.rng.choice(m, size=3, replace=False)
            s[at[0]] = s[at[1]] = self.m.xs
            s[at[2]] = self.wall[k][self.rng.integers(0, len(self.wall[k]))]
        return s

    def goals(self):
        k = self.m.map
        g = self.free[k][self.rng.integers(0, len(self.free[k]), size=N_GOALS - 4)]
        o = self.wall[k][self.rng.integers(0, len(self.wall[k]), size=4)]
        return np.concatenate([g, o]).astype(np.int32)[self.rng.permutation(N_GOALS)]

    def emit(self, *op):
        expect = self.m.apply(op)
        self.steps.append(Step(op, expect, self.m.after(), self.m.timers()))
        return expect

    # state
    def Q(self):
        return self.m.b[self.b].q

    def pick(self):
        return int(self.rng.integers(0, len(self.Q())))

    def other_map(self, choices=(MAP_A, MAP_B, MAP_WALL)):
        c = [k for k in choices if k != self.m.map]
        return int(c[self.rng.integers(0, len(c))])

    def ask(self, q):
        self.emit("goals", self.b, q, self.goals())

    def ask_routes(self, q):
        self.emit("routes", self.b, q, self.goals(), bool(self.rng.integers(0, 2)))

    # ---- the blocks; each leaves every query of the batch finished ----
    def prologue(self):
        self.emit("set_grid", MAP_A)
        for q, (n, alg) in enumerate(zip(NS, ALGS)):
            self.emit("set_query", self.b, q, dict(alg=alg, n=n, xg=self.m.xgs[q], samples=self.samples(n, special=False)))
        self.emit("launch", self.b)

    def keep_cut_grow(self):
        """a new map, keep, goals, a grow from the view, routes and their rows"""
        q = self.pick()
        self.emit("set_grid", self.other_map())
        alive = self.emit("keep", self.b, q)
        self.ask(q)
        room = self.Q()[q].n - int(alive.sum())
        self.emit("grow", self.b, q, self.samples(min(room, int(self.rng.integers(20, 120)))))
        self.ask_routes(q)
        self.emit("rows", self.b)

    def rearm_then_grow_without_a_view(self):
        q = self.pick()
        self.emit("rearm", self.b)
        self.emit("result", self.b, q)  # refused: rearmed and not launched
        self.emit("launch", self.b)
        t = self.Q()[q].tree
        self.emit("grow", self.b, q, self.samples(min(t.n - t.j, int(self.rng.integers(10, 60)))))
        self.emit("keep", self.b, q)  # directly after a grow on the same map: everything stays
        self.ask(q)

    def grow_nothing(self):
        q = self.pick()
        self.emit("keep", self.b, q)
        self.emit("grow", self.b, q, np.zeros((0, 2), dtype=np.int64))
        self.emit("result", self.b, q)

    def fill_exactly(self):
        q = self.pick()
        self.emit("set_grid", MAP_WALL if self.m.map != MAP_WALL else MAP_A)
        alive = self.emit("keep", self.b, q)
        self.emit("grow", self.b, q, self.samples(self.Q()[q].n - int(alive.sum())))
        self.ask_routes(q)

    def no_room(self):
        q = self.pick()
        alive = self.emit("keep", self.b, q)
        self.emit("grow", self.b, q, self.samples(self.Q()[q].n - int(alive.sum()) + 1))
        self.ask(q)  # the refusal left the view

    def root_blocked(self):
        q = self.pick()
        back = self.other_map()
        self.emit("set_grid", MAP_ROOT)
        self.emit("keep", self.b, q)
        self.ask(q)
        self.emit("grow", self.b, q, self.samples(10))
        self.emit("set_grid", back)
        self.emit("keep", self.b, q)

    def new_query_on_a_kept_one(self):
        q = self.pick()
        self.emit("keep", self.b, q)
        s = self.Q()[q]
        self.emit("set_query", self.b, q, dict(alg=int(self.rng.integers(0, 2)), n=s.n, xg=self.m.xgs[self.pick()], samples=self.samples(s.n, special=False)))
        self.emit("goals", self.b, q, self.goals())  # refused: not launched
        self.emit("launch", self.b)
        self.ask(q)

    def stale(self):
        """the map replaced under finished queries: the goals calls refuse, a launch with nothing to run changes no tree"""
        q = self.pick()
        self.emit("keep", self.b, (q + 1) % len(self.Q()))
        self.emit("launch", self.b)  # nothing runs; the view is gone
        self.emit("goals", self.b, (q + 1) % len(self.Q()), self.goals())  # refused: no grid it is known valid on
        self.emit("keep", self.b, (q + 1) % len(self.Q()))
        self.emit("keep", self.b, q)
        self.ask_routes(q)

    def armed_on_another_map(self):
        """grow seeded on one map, the map replaced, launch: refused until rearm"""
        q = self.pick()
        self.emit("keep", self.b, q)
        alive = self.Q()[q].view
        self.emit("arm", self.b, q, self.samples(min(self.Q()[q].n - int(alive.sum()), 30)))
        self.emit("set_grid", self.other_map())
        self.emit("launch", self.b)
        self.emit("rearm", self.b)
        self.emit("launch", self.b)
        self.ask(q)

    def run(self):
        self.prologue()
        blocks = [self.keep_cut_grow, self.keep_cut_grow, self.rearm_then_grow_without_a_view, self.grow_nothing, self.fill_exactly, self.no_room,
                  self.root_blocked, self.new_query_on_a_kept_one, self.stale, self.armed_on_another_map]
        for k in self.rng.permutation(len(blocks)):
            blocks[int(k)]()
        return self.steps


class _GenOne(_Gen):
    """One query at a time, in the calls a context's own batch and the planner classes have: ("plan", k, spec) sets map k, a query
    and runs it; ("keep1", k) sets map k and keeps the tree on it; ("grow1", samples), ("goals1", goals), ("routes1", goals, shortcut);
    ("set_grid", k) alone, after which everything is refused until the next plan.  The samples of plans and of grows that run come
    from a stream of their own, `self.draws`, drawn as a planner of that seed draws them (n of the free cells of its map a plan, m a
    grow; a refused grow draws nothing); everything else comes from the sequence's stream."""
    N1 = 900

    def __init__(self, seed):
        super().__init__(seed, model=Model(Q=1))
        self.draws = np.random.default_rng(seed)

    def emit1(self, *op):
        """one operation of the single-query vocabulary, as the operations of the model it stands for"""
        m = self.m
        if op[0] == "plan":
            m.apply(("set_grid", op[1]))
            m.apply(("set_query", 0, 0, op[2]))
            m.apply(("launch", 0))
            expect = m.b[0].q[0].tree
        elif op[0] == "keep1":
            m.apply(("set_grid", op[1]))
            expect = m.apply(("keep", 0, 0))
        elif op[0] == "set_grid":
            expect = m.apply(op)
        else:
            expect = m.apply((op[0][:-1], 0, 0) + tuple(op[1:]))
        m.notes[-1]["kind1"] = op[0]
        self.steps.append(Step(op, expect, m.after(), m.timers()))
        self.steps[-1].draws_state = self.draws.bit_generator.state  # where a planner's stream stands after the operation
        return expect

    def plan(self, k, alg):
        state = self.draws.bit_generator.state  # (a planner created for this plan starts its stream here)
        spec = dict(alg=alg, n=self.N1, xg=self.m.xgs[self.pick3()], samples=hostprep.draw_free_samples(self.draws, self.free[k], self.N1), draws_state=state)
        return self.emit1("plan", k, spec)

    def pick3(self):
        return int(self.rng.integers(0, len(self.m.xgs)))

    def grow1(self, m):
        refused = self.m.grow_refused(0, 0, m)
        samples = np.zeros((m, 2), dtype=np.int64) if refused else hostprep.draw_free_samples(self.draws, self.free[self.m.map], m)
        return self.emit1("grow1", samples)

    def ask1(self):
        self.emit1("goals1", self.goals())
        self.emit1("routes1", self.goals(), bool(self.rng.integers(0, 2)))

    def tree(self):
        return self.m.b[0].q[0].tree

    def run(self):
        self.plan(MAP_A, 1)
        self.ask1()
        self.grow1(min(self.N1 - self.tree().j, int(self.rng.integers(10, 60))))  # without a view
        for alg in (0, 1):
            for k in self.rng.permutation([MAP_B, MAP_WALL, MAP_A, MAP_WALL]):
                alive = self.emit1("keep1", int(k))
                self.ask1()
                room = self.N1 - int(alive.sum())
                self.grow1(int(self.rng.choice([0, min(room, 80), room + 1, room])))  # nothing, some, one too many, exactly the room
                self.emit1("goals1", self.goals())
            self.emit1("keep1", MAP_ROOT)
            self.emit1("goals1", self.goals())
            self.grow1(10)  # nothing to grow from
            back = self.other_map()
            self.emit1("set_grid", back)  # the map replaced and the tree not kept: refused until the next plan
            self.emit1("goals1", self.goals())
            self.grow1(10)
            if alg == 0:
                self.plan(back, 0)  # a new query in a kept one's place, RRTStandard
                self.ask1()
        return self.steps


NO_SAMPLES = np.zeros((0, 2), dtype=np.int64)


def _depths(t, alive=None):
    """edges between each vertex of the tree and its root; -1 for a vertex that is not alive"""
    d = np.asarray(keepref.depth(t.parent, t.j), dtype=np.int64)
    return d if alive is None else np.where(alive, d, -1)


def _deepest(t, alive=None):
    return int(np.argmax(_depths(t, alive)))


def _mid(t, alive=None):
    way = rerootref.path_to_root(t.parent, t.j, _deepest(t, alive))
    return int(way[len(way) // 2])


class _GenRoot(_Gen):
    """The sequences with reroot and relax: _Gen's draws and plumbing, blocks of their own.  The vertices to re-root at are read from
    the model's trees, so an operation list replayed on other state (interleaved) meets them as plain numbers."""

    def room(self, q):
        s = self.Q()[q]
        return s.n - (s.tree.j if s.view is None else int(s.view.sum()))

    def launch(self):
        """a launch; a query that would plan from a start the active map blocks (a reroot moved it) gets a new query first"""
        for q, s in enumerate(self.Q()):
            if s.kind == "set" and self.m.og[s.xs[0], s.xs[1]] != 0:
                self.emit("set_query", self.b, q, dict(alg=s.alg, n=s.n, xg=s.xg, samples=self.samples(s.n, special=False)))
        return self.emit("launch", self.b)

    def ready(self, q, view=False):
        """query q answers on the active map: with a view, or (view=False) as a whole tree in its own numbers"""
        s = self.Q()[q]
        if s.ran == self.m.gen and s.view is None and s.kind == "done" and not view:
            return
        alive = self.emit("keep", self.b, q)
        if not alive.any():  # the tree's root is blocked here: a new query from the start
            self.emit("set_query", self.b, q, dict(alg=s.alg, n=s.n, xg=s.xg, samples=self.samples(s.n, special=False)))
            self.launch()
            if view:
                self.emit("keep", self.b, q)
        elif not view:
            self.emit("grow", self.b, q, NO_SAMPLES)  # (uses up the view: the alive vertices are the tree)

    def some(self, q, lo, hi):
        return self.samples(min(self.room(q), int(self.rng.integers(lo, hi))))

    def r2(self):
        return hostprep.radius_threshold(RELAX_R[int(self.rng.integers(0, len(RELAX_R)))])

    def cutting_map(self, q):
        """another map than the active one: the one that cuts the tree of query q nearest to half"""
        t = self.Q()[q].tree
        cut = {k: float((~keepref.alive(self.m.maps[k], t.pts, t.parent, t.j)).mean()) for k in (MAP_A, MAP_B, MAP_WALL) if k != self.m.map}
        return min(cut, key=lambda k: (abs(cut[k] - 0.5), k))

    # ---- the blocks; each leaves every query of the batch finished ----
    def reroot_mid_then_deepest(self):
        q = self.pick()
        self.ready(q)
        self.emit("reroot", self.b, q, _mid(self.Q()[q].tree), self.some(q, 10, 50))
        self.ask(q)
        self.emit("reroot", self.b, q, _deepest(self.Q()[q].tree), NO_SAMPLES)
        self.ask_routes(q)
        self.emit("rows", self.b)

    def prologue(self):
        self.emit("set_grid", MAP_A)
        self.emit("reroot", self.b, 0, 0, NO_SAMPLES)  # refused: no query set
        self.emit("relax", self.b, 1, R2, NO_SAMPLES)
        for q, (n, alg) in enumerate(zip(NS, ALGS)):
            self.emit("set_query", self.b, q, dict(alg=alg, n=n, xg=self.m.xgs[q], samples=self.samples(n, special=False)))
        self.emit("launch", self.b)

    def the_gate(self):
        """reroot and relax on a query that is armed and on one that is set: refused, and nothing changes, the start least of all:
        the launch behind them plans from where the queries started before"""
        q = self.pick()
        p = (q + 1) % len(self.Q())
        self.ready(q)
        self.emit("arm", self.b, q, self.some(q, 5, 20))
        self.emit("reroot", self.b, q, 0, NO_SAMPLES)  # refused: armed and not launched
        self.emit("relax", self.b, q, self.r2(), NO_SAMPLES)
        self.emit("rearm", self.b)
        self.emit("reroot", self.b, p, 1, self.samples(3))  # refused: set and not launched
        self.emit("relax_arm", self.b, p, self.r2(), NO_SAMPLES)
        self.launch()
        self.ask(p)

    def reroot_room_before_the_cut(self):
        """the room is checked with the vertices before the call: at a vertex behind an edge that is blocked walked backwards, a reroot
        drops vertices, and one sample more than the room is refused all the same, though what the reroot leaves would have fitted"""
        q = self.pick()
        self.ready(q)
        t = self.Q()[q].tree
        behind = [k for k in range(1, t.j) if not oracle.collisionfree(self.m.og, t.pts[k], t.pts[int(t.parent[k])])[0]]
        r = behind[int(self.rng.integers(0, len(behind)))] if behind else _deepest(t)
        self.emit("reroot", self.b, q, r, self.samples(self.room(q) + 1))  # refused: room for
        self.m.notes[-1]["behind"] = len(behind)
        self.emit("reroot", self.b, q, r, self.some(q, 10, 40))
        self.ask(q)

    def reroot_from_a_view(self):
        """new map, keep, reroot at the deepest alive vertex in the caller's numbers with m > 0"""
        q = self.pick()
        self.emit("set_grid", self.cutting_map(q))
        self.ready(q, view=True)
        s = self.Q()[q]
        self.emit("reroot", self.b, q, _deepest(s.tree, s.view), self.some(q, 20, 80))
        self.ask_routes(q)

    def reroot_dead_then_live(self):
        """the refusals of a reroot in their order: the map replaced, a vertex outside the tree, one the view has not; then one it has"""
        q = self.pick()
        self.emit("set_grid", self.cutting_map(q))
        self.emit("reroot", self.b, q, 0, NO_SAMPLES)  # refused: replaced
        self.ready(q, view=True)
        s = self.Q()[q]
        dead = np.flatnonzero(~s.view)
        self.emit("reroot", self.b, q, s.tree.j, NO_SAMPLES)  # refused: outside [0, j)
        self.emit("reroot", self.b, q, int(dead[self.rng.integers(0, len(dead))]) if len(dead) else s.tree.j + 3, self.some(q, 5, 20))  # refused: not alive
        self.ask(q)  # the view stands
        self.emit("reroot", self.b, q, _mid(s.tree, s.view), NO_SAMPLES)
        self.ask(q)

    def reroot_then_relax_and_relax_then_reroot(self):
        q = self.pick()
        p = (q + 1 + int(self.rng.integers(0, len(self.Q()) - 1))) % len(self.Q())
        self.ready(q)
        self.emit("reroot", self.b, q, _mid(self.Q()[q].tree), NO_SAMPLES)
        self.emit("relax", self.b, q, self.r2(), self.some(q, 0, 30))
        self.ask(q)
        self.ready(p)
        self.emit("relax", self.b, p, self.r2(), NO_SAMPLES)
        self.emit("reroot", self.b, p, _deepest(self.Q()[p].tree), self.some(p, 0, 30))
        self.ask_routes(p)

    def relax_twice(self):
        """the largest query: the second relax lowers nothing"""
        q = len(self.Q()) - 1
        self.ready(q)
        if self.Q()[q].tree.j <= 1024:  # cut down by what came before: planned anew, it has more than a workgroup's width of vertices
            t = self.Q()[q]
            self.emit("set_query", self.b, q, dict(alg=t.alg, n=t.n, xg=t.xg, samples=self.samples(t.n, special=False)))
            self.launch()
        r2 = self.r2()
        self.emit("relax", self.b, q, r2, NO_SAMPLES)
        self.emit("relax", self.b, q, r2, NO_SAMPLES)
        self.ask(q)

    def relax_room(self):
        """one sample too many, a bad radius together with too many samples (the room wins), the bad radius alone, exactly the room"""
        q = self.pick()
        self.ready(q, view=True)
        room = self.room(q)
        self.emit("relax", self.b, q, self.r2(), self.samples(room + 1))
        self.emit("relax", self.b, q, 0, self.samples(room + 1))
        self.emit("relax", self.b, q, int(-self.rng.integers(0, 5)), self.samples(min(room, 8)))
        self.emit("relax", self.b, q, self.r2(), self.samples(room))
        self.ask(q)

    def reroot_rearm_launch(self):
        """rearm + launch plans from the new root"""
        q = self.pick()
        self.ready(q)
        self.emit("reroot", self.b, q, _mid(self.Q()[q].tree), NO_SAMPLES)
        self.emit("rearm", self.b)
        self.launch()
        self.ask(q)

    def reroot_then_the_old_start_blocked(self):
        """the map that blocks the old start: the re-rooted tree keeps what does not hang on it, a tree rooted there keeps nothing"""
        q = self.pick()
        p = (q + 1) % len(self.Q())
        back = self.other_map()
        self.ready(q)
        self.emit("reroot", self.b, q, _mid(self.Q()[q].tree), NO_SAMPLES)
        s = self.Q()[p]
        self.emit("set_query", self.b, p, dict(alg=s.alg, n=s.n, xg=s.xg, samples=self.samples(s.n, special=False)))  # p starts at the old start again
        self.launch()
        self.emit("set_grid", MAP_ROOT)
        self.emit("keep", self.b, q)
        self.ask(q)
        self.emit("keep", self.b, p)
        self.emit("relax", self.b, p, self.r2(), NO_SAMPLES)  # refused: p's root is blocked, nothing to grow from
        self.emit("grow", self.b, q, self.some(q, 5, 15))
        self.emit("set_grid", back)
        self.emit("keep", self.b, q)

    def armed_on_another_map(self):
        """a reroot and a relax seeded on one map, the map replaced, launch: refused until rearm"""
        q = self.pick()
        p = (q + 1) % len(self.Q())
        self.emit("set_grid", self.cutting_map(q))
        self.ready(q, view=True)
        s = self.Q()[q]
        self.emit("reroot_arm", self.b, q, _deepest(s.tree, s.view), self.some(q, 5, 30))
        self.ready(p)
        self.emit("relax_arm", self.b, p, self.r2(), self.some(p, 5, 30))
        self.emit("set_grid", self.other_map())
        self.emit("launch", self.b)  # refused: seeded
        self.emit("rearm", self.b)
        self.launch()
        self.ask(q)

    def run(self):
        self.prologue()
        blocks = [self.the_gate, self.reroot_mid_then_deepest, self.reroot_room_before_the_cut, self.reroot_from_a_view, self.reroot_dead_then_live, self.reroot_then_relax_and_relax_then_reroot,
                  self.relax_twice, self.relax_room, self.reroot_rearm_launch, self.reroot_then_the_old_start_blocked, self.armed_on_another_map]
        for k in self.rng.permutation(len(blocks)):
            blocks[int(k)]()
        q = self.pick()  # the Dubins calls on this batch: refused, and the view and the route rows stand
        self.emit("keep", self.b, q)
        self.ask_routes(q)
        self.emit("pose_calls", self.b, q)
        self.emit("rows", self.b)
        return self.steps


class _GenOneRoot(_GenOne):
    """_GenOne's vocabulary with ("reroot1", root, samples) and ("relax1", r2, samples): Context.reroot / relax with the launch and the
    result, RRT.reroot(vertex, m) / RRT.relax(r, m).  Their samples come from the planner's stream, and only when they run."""

    def seed1(self, how, arg, m):
        refused = self.m.grow_refused(0, 0, m, how, arg)
        samples = np.zeros((m, 2), dtype=np.int64) if refused else hostprep.draw_free_samples(self.draws, self.free[self.m.map], m)
        return self.emit1(how + "1", arg, samples)

    def r2(self):
        return hostprep.radius_threshold(RELAX_R[int(self.rng.integers(0, len(RELAX_R)))])

    def room1(self):
        s = self.m.b[0].q[0]
        return self.N1 - (s.tree.j if s.view is None else int(s.view.sum()))

    def some1(self, lo, hi):
        return min(self.room1(), int(self.rng.integers(lo, hi)))

    def run(self):
        s = self.m.b[0].q[0]
        self.plan(MAP_A, 1)
        self.ask1()
        self.seed1("reroot", _mid(self.tree()), self.some1(10, 60))
        self.ask1()
        self.seed1("relax", self.r2(), 0)
        self.emit1("goals1", self.goals())
        for alg in (1, 0):
            for k in self.rng.permutation([MAP_B, MAP_WALL, MAP_A]):
                alive = self.emit1("keep1", int(k))
                if not alive.any():  # (the moved root is blocked there)
                    self.seed1("relax", self.r2(), 5)
                    continue
                dead = np.flatnonzero(~alive)
                self.seed1("reroot", int(dead[0]) if len(dead) else self.tree().j, 3)  # refused: not alive, or outside the tree
                self.seed1("reroot", _deepest(self.tree(), s.view), self.some1(20, 80))  # from the view, in the caller's numbers
                self.ask1()
                self.seed1("relax", self.r2(), int(self.rng.choice([0, self.some1(10, 40), self.room1() + 1])))  # nothing, some, one too many
                self.grow1(self.some1(0, 30))
                self.emit1("goals1", self.goals())
            self.emit1("keep1", MAP_ROOT)  # the old start blocked: the re-rooted tree keeps what does not hang on it
            self.emit1("goals1", self.goals())
            self.seed1("relax", self.r2(), self.some1(0, 10))
            back = self.other_map()
            self.emit1("set_grid", back)  # the map replaced and the tree not kept: refused until the next plan
            self.seed1("reroot", 0, 0)
            self.seed1("relax", self.r2(), 0)
            if alg == 1:
                self.plan(back, 0)  # a new query from the old start, RRTStandard
                self.ask1()
                self.emit1("keep1", MAP_ROOT)  # this tree starts at the old start: nothing is alive
                self.seed1("reroot", 0, 0)  # refused: nothing to grow from
                self.emit1("keep1", back)
                self.seed1("relax", self.r2(), self.some1(10, 40))
                self.seed1("reroot", _deepest(self.tree()), 0)
                self.emit1("pose_calls1")  # the Dubins calls: refused, nothing changes
        return self.steps


def _gen_of(seed):
    return _GenRoot if seed in ROOT_SEEDS else _Gen


def trace_one(seed):
    if ("one", seed) not in _cache:
        g = (_GenOneRoot if seed in ROOT_ONE_SEEDS else _GenOne)(seed)
        _cache[("one", seed)] = (g.run(), g.m.notes)
    return _cache[("one", seed)]


def trace(seed):
    """the steps of sequence `seed` (operation, expected answer, what every query answers afterwards) and the model's notes; cached"""
    if ("trace", seed) not in _cache:
        g = _gen_of(seed)(seed)
        _cache[("trace", seed)] = (g.run(), g.m.notes)
    return _cache[("trace", seed)]


def operations(seed):
    return [s.op for s in trace(seed)[0]]


def replay(seed, upto=None, ops=None, nbatches=1):
    """the model after the first `upto` operations of sequence `seed` (or of the list `ops`), and the steps up to there: a failing
    GPU case read on the CPU"""
    ops = operations(seed) if ops is None else ops
    m = Model(nbatches=nbatches)
    steps = []
    for op in ops[:upto]:
        e = m.apply(op)
        steps.append(Step(op, e, m.after(), m.timers()))
    return m, steps


def interleaved(seed_a, seed_b, upto=None):
    """two batches on one context: alternate operations of two sequences, the second one's on batch 1.  The grid is shared, so one
    sequence's set_grid lands between the other's keep and grow, and the model decides who is "replaced".  A launch that would run a
    query while the root-blocking map is active gets a set_grid(first map) in front: a plan from a blocked root is no case of these
    tests."""
    key = ("interleaved", seed_a, seed_b, upto)
    if key not in _cache:
        a = operations(seed_a)[:upto]  # (upto: the first operations of each alone)
        b = [(op[0], 1) + tuple(op[2:]) if op[0] != "set_grid" else op for op in operations(seed_b)[:upto]]
        m = Model(nbatches=2)
        steps = []

        def emit(op):
            steps.append(Step(op, m.apply(op), m.after(), m.timers()))

        for k in range(max(len(a), len(b))):
            for ops in (a, b):
                if k >= len(ops):
                    continue
                op = ops[k]
                if m.map == MAP_ROOT and op[0] in ("launch", "grow", "arm") and (op[0] != "launch" or any(s.kind in ("set", "armed") for s in m.b[op[1]].q)):
                    emit(("set_grid", MAP_A))
                elif op[0] == "launch":  # ... nor is one from a start that a reroot moved onto a cell the active map blocks
                    starts = [s.xs for s in m.b[op[1]].q if s.kind == "set"]
                    if any(m.og[x[0], x[1]] != 0 for x in starts):
                        emit(("set_grid", next(k for k in (MAP_A, MAP_B, MAP_WALL) if all(m.maps[k][x[0], x[1]] == 0 for x in starts))))
                emit(op)
        _cache[key] = (steps, m.notes)
    return _cache[key]
