"""No GPU: the host model of tests/treemodel.py alone, for exactly the sequences tests/test_tree_sequences_gpu.py replays.

(a) every sequence exercises what it is for -- conditions on the model's own notes, met by the choice of the seeds and of the
    generator's blocks, so that a GPU run of the same seeds cannot pass on sequences that cut, grow or refuse nothing;
(b) the model agrees with itself: every edge of a tree that answers is free on the active map, a keep directly after a grow keeps
    everything, keeping for the first map again restores the first answers, and grows with nothing cut are the longer plan;
(c) the same for the sequences with reroot and relax (treemodel.ROOT_SEEDS)."""
import numpy as np
import pytest

import oracle
import treemodel as tm


# ------------------------------------------------------------------------------------------------ (a) coverage
@pytest.mark.parametrize("seed", tm.SEEDS)
def test_the_sequence_exercises_what_it_is_for(seed):
    steps, notes = tm.trace(seed)
    assert len(steps) == len(notes) >= 40
    assert sum(n["refused"] for n in notes) <= 0.30 * len(notes)
    done = [n for n in notes if not n["refused"]]
    keeps = [n for n in done if n["kind"] == "keep"]
    grows = [n for n in done if n["kind"] in ("grow", "arm")]
    assert sum(0.05 <= n["cut"] <= 0.95 for n in keeps) >= 3
    assert sum(n["view"] and n["m"] > 0 for n in grows) >= 3
    assert sum(not n["view"] for n in grows) >= 1
    assert sum(n["m"] == 0 for n in grows) >= 1
    assert sum(n["j0"] + n["m"] == n["n"] and n["m"] > 0 for n in grows) >= 1
    assert sum(n["kind"] == "grow" and n["refused"] and n.get("room", False) for n in notes) >= 1
    # a keep on the root-blocking map, and the next grow of the sequence refused
    at = [k for k, n in enumerate(notes) if n["kind"] == "keep" and not n["refused"] and n["map"] == tm.MAP_ROOT and n["alive"] == 0]
    assert at and any(next(n for n in notes[k:] if n["kind"] in ("grow", "arm"))["refused"] for k in at)
    assert any(a["kind"] == "rearm" and b["kind"] == "launch" and not b["refused"] for a, b in zip(notes, notes[1:]))
    assert any(n["kind"] == "set_query" and n["on_kept"] for n in notes)
    assert any(n["kind"] == "launch" and n["refused"] for n in notes)  # armed on one map, launched on another
    asked = [n for n in done if n["kind"] == "goals" and n["live"]]
    assert len(asked) >= 4 and all(n["connected"] >= 8 and n["unconnected"] >= 1 for n in asked)


def test_the_two_sequences_in_turns_make_each_others_queries_replaced():
    """two batches, one grid: the model says "replaced" often enough to matter, and trees are still cut and grown"""
    steps, notes = tm.interleaved(*tm.PAIR)
    assert sum(isinstance(s.expect, tm.Refusal) and s.expect.word == "replaced" for s in steps) >= 4
    assert sum(isinstance(s.expect, tm.Refusal) for s in steps) <= 0.30 * len(steps)
    assert sum(n["kind"] == "grow" and not n["refused"] for n in notes) >= 4
    assert sum(n["kind"] == "keep" and 0.05 <= n.get("cut", 0) <= 0.95 for n in notes) >= 4
    assert any(s.expect.word == "seeded" for s in steps if isinstance(s.expect, tm.Refusal))
    assert {op[1] for op in (s.op for s in steps) if op[0] != "set_grid"} == {0, 1}


@pytest.mark.parametrize("seed", tm.ONE_SEEDS)
def test_the_single_query_sequence_exercises_what_it_is_for(seed):
    steps, notes = tm.trace_one(seed)
    assert sum(n["refused"] for n in notes) <= 0.30 * len(notes)
    grows = [n for n in notes if n["kind"] == "grow" and not n["refused"]]
    assert sum(n["view"] and n["m"] > 0 for n in grows) >= 3 and sum(not n["view"] for n in grows) >= 1
    refused = [s.expect.word for s in steps if s.op[0] == "grow1" and isinstance(s.expect, tm.Refusal)]
    assert "nothing to grow from" in refused and "replaced" in refused
    assert sum(0.05 <= n["cut"] <= 0.95 for n in notes if n["kind"] == "keep") >= 3
    assert sum(s.op[0] == "plan" for s in steps) == 2 and {s.op[2]["alg"] for s in steps if s.op[0] == "plan"} == {0, 1}


def test_the_same_seed_gives_the_same_list():
    a = tm.operations(tm.SEEDS[0])
    b = [s.op for s in tm._Gen(tm.SEEDS[0]).run()]
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and len(x) == len(y)
        for u, v in zip(x[1:], y[1:]):
            if isinstance(u, dict):
                assert u.keys() == v.keys() and all(np.array_equal(u[k], v[k]) for k in u)
            else:
                assert np.array_equal(u, v)


def test_replay_rebuilds_a_prefix():
    seed = tm.SEEDS[1]
    steps, _ = tm.trace(seed)
    m, part = tm.replay(seed, 12)
    assert len(part) == 12 and len(m.notes) == 12
    for a, b in zip(part, steps):
        assert a.op is b.op and type(a.expect) is type(b.expect)


# ------------------------------------------------------------------------------------------------ (b) the model against itself
def _edges_free(og, t, alive):
    """every edge among the answering vertices, walked from the parent to the child"""
    for k in range(1, t.j):
        if alive is None or alive[k]:
            assert alive is None or alive[int(t.parent[k])]
            assert oracle.collisionfree(og, t.pts[int(t.parent[k])], t.pts[k])[0], k
    return True


@pytest.mark.parametrize("seed", tm.SEEDS[:2])
def test_every_edge_of_a_tree_that_answers_is_free_on_the_active_map(seed):
    """replayed operation by operation; `ran == gen` is the model's word for "answers".  This is the property the launch of a grow
    armed on another map would break: its seed edges were tested on the map of the grow call."""
    m = tm.Model()
    seen = set()
    for op in tm.operations(seed):
        m.apply(op)
        for s in m.b[0].q:
            if s.kind == "done" and s.ran == m.gen and (s.version, m.gen) not in seen:
                seen.add((s.version, m.gen))
                assert _edges_free(m.og, s.tree, s.view)
    assert len(seen) >= 15


@pytest.mark.parametrize("seed", tm.SEEDS)
def test_a_keep_directly_after_a_grow_on_the_same_map_keeps_everything(seed):
    ops, (_, notes) = tm.operations(seed), tm.trace(seed)
    hits = 0
    for k in range(1, len(ops)):
        if ops[k][0] == "keep" and ops[k - 1][0] == "grow" and ops[k][1:3] == ops[k - 1][1:3] and not notes[k - 1]["refused"]:
            assert notes[k]["cut"] == 0.0
            hits += 1
    assert hits >= 1


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) and np.asarray(x).dtype == np.asarray(y).dtype for x, y in zip(a, b))


def test_keeping_for_the_first_map_again_restores_the_first_answers():
    g = tm._Gen(5)
    g.prologue()
    goals = g.goals()
    first = [(g.m.apply(("goals", 0, q, goals)), g.m.apply(("routes", 0, q, goals, True))) for q in range(3)]
    g.m.apply(("set_grid", tm.MAP_B))
    cut = [g.m.apply(("keep", 0, q)) for q in range(3)]
    assert all(0.05 <= (~a).mean() <= 0.95 for a in cut)
    for q in range(3):
        assert not _same(g.m.apply(("goals", 0, q, goals)), first[q][0])
    g.m.apply(("set_grid", tm.MAP_A))
    for q in range(3):
        assert isinstance(g.m.apply(("goals", 0, q, goals)), tm.Refusal)  # a new generation, whatever the map holds
        assert g.m.apply(("keep", 0, q)).all()
        assert _same(g.m.apply(("goals", 0, q, goals)), first[q][0]) and _same(g.m.apply(("routes", 0, q, goals, True)), first[q][1])


@pytest.mark.parametrize("q", [0, 1, 2])
def test_a_chain_of_grows_with_nothing_cut_is_the_plan_over_all_samples(q):
    g = tm._Gen(6)
    g.prologue()
    s = g.m.b[0].q[q]
    first = s.buf.copy()
    room = s.n - s.tree.j
    parts = [g.samples(room // 3), g.samples(0), g.samples(room // 2)]
    assert room // 3 >= 8
    for k, p in enumerate(parts):
        if k == 1:
            assert g.m.apply(("keep", 0, q)).all()  # a view that cuts nothing is no cut
        out = g.m.apply(("grow", 0, q, p))
        assert not isinstance(out, tm.Refusal) and out["j0"] == out["log0"]
    more = np.concatenate(parts)
    n = s.n + len(more)
    st, ro = oracle.plan(g.m.og, n, s.alg, g.m.xs, s.xg, np.concatenate([first, more]), r2_rewire=tm.R2 if s.alg else 0)
    t = s.tree
    live = ro.j + ro.found
    assert (t.j, t.found) == (ro.j, ro.found) and t.j > out["j0"] >= s.n - room
    assert np.array_equal(t.pts[:live], ro.pts[:live]) and np.array_equal(t.parent[:live], ro.parent[:live])
    assert np.array_equal(np.ascontiguousarray(t.vcost[:live]).view(np.int64), np.ascontiguousarray(ro.vcost[:live]).view(np.int64))


# ------------------------------------------------------------------------------------------------ (c) the sequences with reroot and relax
WORDS = ("no query set", "not launched", "replaced", "nothing to grow from", "room for", "has the vertices [0,", "is not alive", "r2=")  # the refusals of reroot and relax, in the engine's order


def _seed_calls(notes, how):
    return [n for n in notes if n["kind"] in tm.SEED_OPS and not n["refused"] and n["how"] == how]


@pytest.mark.parametrize("seed", tm.ROOT_SEEDS)
def test_the_reroot_and_relax_sequence_exercises_what_it_is_for(seed):
    steps, notes = tm.trace(seed)
    assert len(steps) == len(notes) >= 40
    assert sum(n["refused"] for n in notes) <= 0.30 * len(notes)
    assert sum(0.05 <= n["cut"] <= 0.95 for n in notes if n["kind"] == "keep" and not n["refused"]) >= 3
    reroots, relaxes = _seed_calls(notes, "reroot"), _seed_calls(notes, "relax")
    assert sum(n["root"] != 0 for n in reroots) >= 2 and sum(n["root"] != 0 and n["view"] and n["m"] > 0 for n in reroots) >= 1
    assert sum(n["fell"] > 0 for n in relaxes) >= 2 and sum(n["fell"] > 0 and n["j0"] > 1024 for n in relaxes) >= 1
    assert any("reroot" in n["on"] for n in relaxes) and any("relax" in n["on"] for n in reroots)
    assert any(n["fell"] == 0 for n in relaxes)  # the second of two relaxes with one radius
    assert any(n["m"] > 0 and n["j0"] + n["m"] == n["n"] for n in relaxes)  # exactly the room
    refused = {(s.op[0], s.expect.word) for s in steps if isinstance(s.expect, tm.Refusal)}
    assert {w for _, w in refused} >= set(WORDS) | {"seeded"}
    assert ("reroot", "replaced") in refused and ("relax", "room for") in refused and ("relax", "nothing to grow from") in refused
    # the finished-tree gate: no query set, a query that is set, one that is armed -- each for both calls
    assert {("reroot", "no query set"), ("relax", "no query set"), ("reroot", "not launched"), ("relax", "not launched"), ("relax_arm", "not launched")} <= refused
    armed = [k for k, s in enumerate(steps) if s.op[0] == "arm" and not isinstance(s.expect, tm.Refusal)]
    assert any(steps[k + 1].op[0] == "reroot" and steps[k + 1].op[2] == steps[k].op[2] and isinstance(steps[k + 1].expect, tm.Refusal) for k in armed)
    # r2 <= 0 together with too many samples: the room wins
    assert any(s.op[0] == "relax" and s.op[3] <= 0 and isinstance(s.expect, tm.Refusal) and s.expect.word == "room for" for s in steps)
    # the room is checked with the vertices before the call: refused for one sample more, though the reroot that follows cuts vertices
    at = [k for k, n in enumerate(notes) if n.get("behind", 0) > 0 and n["refused"]]
    assert at and all(steps[k].expect.word == "room for" and not notes[k + 1]["refused"] and notes[k + 1]["j0"] < notes[k + 1]["count"] and
                      notes[k + 1]["j0"] + len(steps[k].op[4]) <= notes[k + 1]["n"] for k in at)
    # rearm + launch from a moved root
    assert any(a["kind"] == "rearm" and any(n.get("moved") for n in notes[k + 1:k + 4] if n["kind"] == "launch") for k, a in enumerate(notes))
    # armed on one map, launched on another: both calls armed, the launch refused
    at = [k for k, s in enumerate(steps) if s.op[0] == "launch" and isinstance(s.expect, tm.Refusal)]
    assert at and {s.op[0] for s in steps[:at[0]]} >= {"reroot_arm", "relax_arm"}
    # the old start's cell blocked: the re-rooted tree keeps vertices, a tree that starts there keeps none
    root_map = [n for n in notes if n["kind"] == "keep" and not n["refused"] and n["map"] == tm.MAP_ROOT]
    assert any(n["alive"] > 0 for n in root_map) and any(n["alive"] == 0 for n in root_map)
    # which timer answers changes hands
    assert {s.timed[0][0] for s in steps if s.timed[0]} == {"grow", "reroot", "relax"}


def test_some_reroot_drops_vertices_behind_a_blocked_reversed_edge():
    """j0 smaller than the count the room was checked with"""
    cut = [(seed, n["count"], n["j0"]) for seed in tm.ROOT_SEEDS for n in _seed_calls(tm.trace(seed)[1], "reroot") if n["j0"] < n["count"]]
    assert len(cut) >= 1, cut


def test_the_reroot_and_relax_sequences_in_turns():
    steps, notes = tm.interleaved(*tm.ROOT_PAIR, tm.ROOT_PAIR_OPS)
    words = [s.expect.word for s in steps if isinstance(s.expect, tm.Refusal)]
    assert words.count("replaced") >= 4 and len(words) <= 0.30 * len(steps)
    assert len([n for n in _seed_calls(notes, "reroot") if n["root"] != 0]) >= 4 and len([n for n in _seed_calls(notes, "relax") if n["fell"] > 0]) >= 4
    assert {op[1] for op in (s.op for s in steps) if op[0] != "set_grid"} == {0, 1}
    assert {t[0] for s in steps for t in s.timed if t} == {"grow", "reroot", "relax"}


@pytest.mark.parametrize("seed", tm.ROOT_ONE_SEEDS)
def test_the_single_query_reroot_and_relax_sequence_exercises_what_it_is_for(seed):
    steps, notes = tm.trace_one(seed)
    assert sum(n["refused"] for n in notes) <= 0.30 * len(notes)
    reroots, relaxes = _seed_calls(notes, "reroot"), _seed_calls(notes, "relax")
    assert sum(n["root"] != 0 and n["view"] for n in reroots) >= 2 and sum(n["root"] != 0 and not n["view"] for n in reroots) >= 2
    assert sum(n["fell"] > 0 for n in relaxes) >= 3 and any("reroot" in n["on"] for n in relaxes) and any("relax" in n["on"] for n in reroots)
    assert any(n["m"] > 0 for n in reroots) and any(n["m"] > 0 for n in relaxes)
    words = {s.expect.word for s in steps if s.op[0] in ("reroot1", "relax1") and isinstance(s.expect, tm.Refusal)}
    assert words >= {"replaced", "nothing to grow from", "is not alive"}
    assert sum(0.05 <= n["cut"] <= 0.95 for n in notes if n["kind"] == "keep") >= 3
    assert {s.op[2]["alg"] for s in steps if s.op[0] == "plan"} == {0, 1}
    # a refused call draws nothing from the planner's stream
    for a, b in zip(steps, steps[1:]):
        if b.op[0] in ("reroot1", "relax1", "grow1") and isinstance(b.expect, tm.Refusal):
            assert a.draws_state == b.draws_state


def test_replay_rebuilds_a_prefix_of_a_reroot_and_relax_sequence():
    seed = tm.ROOT_SEEDS[1]
    steps, _ = tm.trace(seed)
    m, part = tm.replay(seed, 10)
    assert len(part) == 10 and all(a.op is b.op and type(a.expect) is type(b.expect) and a.timed == b.timed for a, b in zip(part, steps))


@pytest.mark.parametrize("seed", tm.ROOT_SEEDS)
def test_every_edge_of_a_rerooted_or_relaxed_tree_that_answers_is_free_on_the_active_map(seed):
    """over the states the model recorded while the sequence was drawn (notes[k]["answers"]): no second replay"""
    _, notes = tm.trace(seed)
    maps = tm.workload()[0]
    seen = 0
    for n in notes:
        for t, view, k in n["answers"]:
            assert _edges_free(maps[k], t, view)
            seen += 1
    assert seen >= 15


@pytest.mark.parametrize("seed", tm.ROOT_SEEDS)
def test_a_reroot_puts_the_vertex_first_and_prices_it_zero(seed):
    """after a reroot at r, pts[0] is the old pts[r] and vcost[0] == 0.0; a relax leaves the root where it is"""
    steps, _ = tm.trace(seed)
    hits = 0
    for before, st in zip(steps, steps[1:]):
        if st.op[0] in ("reroot", "relax") and not isinstance(st.expect, tm.Refusal):
            old, new = before.after[st.op[1]][st.op[2]][0], st.expect["tree"]
            r = st.op[3] if st.op[0] == "reroot" else 0
            assert np.array_equal(new.pts[0], old.pts[r]) and new.vcost[0] == 0.0 and new.parent[0] == -1 and st.expect["old_id"][0] == r
            assert st.expect["j0"] == len(st.expect["old_id"]) <= new.j
            hits += 1
    assert hits >= 10
