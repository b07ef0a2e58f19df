"""No GPU: the host model of tests/posetreemodel.py alone, for exactly the sequences tests/test_pose_sequences_gpu.py replays: every
sequence exercises what it is for (conditions on the model's own notes, met by the choice of the seeds), and every parent edge of a
tree that answers is a swept-free word on the active map."""
import numpy as np
import pytest

import posekeepref
import posetreemodel as pm
import treemodel as tm


def _seed_calls(notes, how):
    return [n for n in notes if n["kind"] in ("grow", "arm", "relax", "relax_arm") and not n["refused"] and n["how"] == how]


def _after_refused(steps, kinds_asked):
    """the operations directly in front of a refused `rows` / `points`"""
    kinds = [s.op[0] for s in steps]
    return {kinds[k - 1] for k in range(1, len(steps)) if kinds[k] in kinds_asked and isinstance(steps[k].expect, tm.Refusal)}


@pytest.mark.parametrize("seed", pm.POSE_SEEDS)
def test_the_pose_sequence_exercises_what_it_is_for(seed):
    """the blocks are shared out between the sequence of even and the one of odd seed (_GenPose.run); each is held to what its blocks are for"""
    steps, notes = pm.trace(seed)
    assert len(steps) == len(notes) >= 40 and sum(n["refused"] for n in notes) <= 0.30 * len(notes)
    assert sum(0.05 <= n["cut"] <= 0.95 for n in notes if n["kind"] == "keep" and not n["refused"]) >= 2
    grows, relaxes = _seed_calls(notes, "grow"), _seed_calls(notes, "relax")
    words = {s.expect.word for s in steps if isinstance(s.expect, tm.Refusal)}
    kinds = [s.op[0] for s in steps]
    routes = [n for n in notes if n["kind"] == "routes" and not n["refused"]]
    assert words >= {"replaced", "nothing to grow from", "a Dubins batch", "not a Dubins batch"} and {"line_calls", "pose_calls"} <= set(kinds)
    assert sum(n["view"] and n["m"] > 0 for n in grows) >= 1 and all(n["rows"] >= 8 for n in routes) and any(n["points"] for n in routes)
    if seed % 2 == 0:  # keep_cut_grow, rows_do_not_outlive, root_blocked
        assert sum(n["view"] and n["m"] > 0 for n in grows) >= 2 and {s.timed[0][0] for s in steps if s.timed[0]} == {"grow"}
        assert len(routes) >= 4 and any(not n["points"] for n in routes) and any(n["shortcut"] for n in routes) and any(n["view"] for n in routes)
        assert words >= {"no routes", "no points"}
        # the rows and the points of a routes call answer once, and are refused after a keep, a rearm, a launch, a grow and a refused routes call
        assert any(kinds[k:k + 3] == ["routes", "rows", "points"] and not isinstance(steps[k + 1].expect, tm.Refusal) and
                   not isinstance(steps[k + 2].expect, tm.Refusal) for k in range(len(steps) - 2))
        assert _after_refused(steps, ("rows", "points")) >= {"keep", "rearm", "launch", "grow", "routes"}
        assert any(s.op[0] == "routes" and isinstance(s.expect, tm.Refusal) and s.expect.word == "replaced" for s in steps)
        assert any(kinds[k:k + 3] == ["routes", "rows", "points"] and not steps[k].op[4] and not isinstance(steps[k + 1].expect, tm.Refusal) and
                   isinstance(steps[k + 2].expect, tm.Refusal) for k in range(len(steps) - 2))  # rows without points
    else:  # relax_with_samples, relax_room, rearm_then_grow_without_a_view, armed_on_another_map, root_blocked
        assert sum(not n["view"] for n in grows) >= 1 and {s.timed[0][0] for s in steps if s.timed[0]} == {"grow", "relax"}
        assert sum(n["fell"] > 0 and n["m"] > 0 and n["view"] for n in relaxes) >= 2  # the heading rows [j0, j0 + m) behind a relax that renumbers
        assert max(n["j0"] for n in grows + relaxes) > 1024  # more than 1024 live vertices at a grow-like call
        assert words >= {"room for", "r2=", "seeded"}
        assert any(s.op[0] == "relax" and s.op[3] <= 0 and isinstance(s.expect, tm.Refusal) and s.expect.word == "room for" for s in steps)
        # a refused launch drops nothing: the rows and the points of the routes call before it still answer
        at = [k for k, s in enumerate(steps) if s.op[0] == "launch" and isinstance(s.expect, tm.Refusal)]
        assert at and all(kinds[k + 1:k + 3] == ["rows", "points"] and not isinstance(steps[k + 1].expect, tm.Refusal) and
                          not isinstance(steps[k + 2].expect, tm.Refusal) and len(steps[k + 1].expect[1]) >= 8 for k in at)


def test_the_two_pose_sequences_have_every_block_between_them():
    assert {seed % 2 for seed in pm.POSE_SEEDS} == {0, 1}


def test_three_queries_with_three_rho_and_nh():
    assert len({q[3:] for q in pm.QUERIES}) == len(pm.QUERIES) == 3 and pm.ONE[3:] not in {q[3:] for q in pm.QUERIES}


def test_the_two_pose_sequences_in_turns():
    steps, notes = pm.interleaved(*pm.POSE_PAIR, pm.POSE_PAIR_OPS)
    words = [s.expect.word for s in steps if isinstance(s.expect, tm.Refusal)]
    assert words.count("replaced") >= 4 and len(words) <= 0.30 * len(steps)
    assert len(_seed_calls(notes, "grow")) >= 2 and len(_seed_calls(notes, "relax")) >= 2  # each seed call more than once while the other batch moves the grid
    assert {op[1] for op in (s.op for s in steps) if op[0] != "set_grid"} == {0, 1}


def test_replay_rebuilds_a_prefix_of_a_pose_sequence():
    seed = pm.POSE_SEEDS[0]
    steps, _ = pm.trace(seed)
    m, part = pm.replay(seed, 8)
    assert len(part) == 8 and all(a.op is b.op and type(a.expect) is type(b.expect) for a, b in zip(part, steps))


def _edges_swept_free(notes):
    maps, _, _ = pm.workload()
    seen = 0
    for n in notes:
        for t, view, k in n["answers"]:
            ok = posekeepref.edge_ok(maps[k], t.pts, t.head, t.parent, t.j, t.rho, t.nh)
            alive = np.ones(t.j, dtype=bool) if view is None else view
            below = alive & (np.arange(t.j) > 0)
            assert ok[alive].all() and (t.parent[:t.j][below] >= 0).all() and alive[t.parent[:t.j][below]].all()
            seen += 1
    return seen


@pytest.mark.parametrize("seed", pm.POSE_SEEDS)
def test_every_parent_edge_of_a_pose_tree_that_answers_is_a_swept_free_word_on_the_active_map(seed):
    """over the states the model recorded while the sequence was drawn (notes[k]["answers"]): no second replay"""
    assert _edges_swept_free(pm.trace(seed)[1]) >= 10


def test_the_single_query_pose_sequence_exercises_what_it_is_for():
    steps, notes = pm.trace_one(pm.POSE_ONE_SEED)
    assert sum(n["refused"] for n in notes) <= 0.30 * len(notes)
    grows, relaxes = _seed_calls(notes, "grow"), _seed_calls(notes, "relax")
    assert sum(n["view"] for n in grows) >= 1 and sum(not n["view"] for n in grows) >= 1
    assert sum(n["view"] and n["m"] > 0 for n in relaxes) >= 1 and sum(n["fell"] > 0 for n in relaxes) >= 2
    words = {s.expect.word for s in steps if isinstance(s.expect, tm.Refusal)}
    assert words >= {"replaced", "nothing to grow from"}
    assert sum(0.05 <= n["cut"] <= 0.95 for n in notes if n["kind"] == "keep") >= 2
    assert {s.op[0] for s in steps} >= {"plan", "keep1", "grow1", "relax1", "poses1", "routes1"} and sum(s.op[0] == "plan" for s in steps) == 2
    assert _edges_swept_free(notes) >= 8
