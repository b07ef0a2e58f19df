"""CPU: the cases of tests/test_shift_pair_gpu.py are what that file says they are, so that none of its tests passes vacuously; and
the two tables of launch shapes both name the pair of 64 in one shift and in two."""
import numpy as np
import pytest

import devcheck
import farnn
import growref
import oracle
import shiftcases as sc
import treecalls as tc


# ------------------------------------------------------------------------------------------------ the tables of launch shapes
def test_both_tables_hold_the_capped_and_the_uncapped_pair_and_nothing_else_that_large():
    for table in (devcheck.KERNEL_ARGS, {k: kw for k, (kw, _) in tc.SHAPES.items()}):
        assert table["team"] == {} and table["team64"] == {"team": 64}
        assert [k for k, kw in table.items() if kw.get("team", 0) >= 64] == ["team64"]
    assert "team64" in devcheck.KERNELS_NOFAULT and list(tc.SHAPES)[-1] == "team64"
    assert tc.TWO_SHIFTS == tc.ONE_SHIFT + " in 2 shifts" and set(sc.PAIR) == {"team", "team64"}


def test_the_name_of_each_shape_by_batch_size():
    """One query: two shifts without a cap, one with the cap of 64.  Two queries: the pair of 64 in one shift.  Three and more: the
    launch plan restated -- on 256 compute units three queries get the pair of 32 (a team of 64 takes 6 slots of 65 for them), and
    so on down to the kernels test_variant_matrix.py names."""
    pair32 = "rrt_expand_block_kernel<32, 2, true, false> as rrt_block_commit_kernel + rrt_block_work_kernel<32, 2, false>"
    assert tc.team_name_ok(tc.TWO_SHIFTS, 1) and not tc.team_name_ok(tc.ONE_SHIFT, 1)
    assert tc.team64_name_ok(tc.ONE_SHIFT, 1) and not tc.team64_name_ok(tc.TWO_SHIFTS, 1)
    for ok in (tc.team_name_ok, tc.team64_name_ok):
        assert ok(tc.ONE_SHIFT, 2) and not ok(tc.TWO_SHIFTS, 2)
    assert tc.planned_name(2, cus=256) == tc.ONE_SHIFT and tc.planned_name(3, cus=256) == tc.planned_name(4, cus=256) == pair32
    assert tc.planned_name(8, cus=256) == "rrt_expand_block_kernel<16, 4, true, false> as rrt_block_commit_kernel + rrt_block_work_kernel<16, 4, false>"
    assert tc.planned_name(16, cus=256) == "rrt_expand_block_kernel<8, 8, true, false> as rrt_block_commit_kernel + rrt_block_work_kernel<8, 8, false>"
    assert tc.planned_name(3, want=8, cus=256) == tc.planned_name(16, cus=256)
    assert tc.planned_name(512, cus=256) == "rrt_pipe_kernel"
    for shape in tc.SHAPES:  # every check takes (name, Q)
        assert tc.SHAPES[shape][1]("no such kernel", 1) is False


# ------------------------------------------------------------------------------------------------ a. mid-stream starts
def test_the_m_values_make_the_block_counts_they_are_for():
    assert tuple(sc.GROW_BLOCKS) == sc.GROW_M and all(sc.blocks(m) == b for m, b in sc.GROW_BLOCKS.items())
    assert [m % sc.SB for m in sc.GROW_M] == [1, 63, 0, 1, 63, 0, 1, 0, 1]  # short last blocks, full ones, blocks of one sample
    # the short last block on either shift: block 3 is the first shift's, blocks 2 and 4 the second's
    assert sc.blocks(65) == 2 and sc.blocks(129) == 3 and sc.blocks(193) == 4 and set(sc.SEED_M) == {65, 129}


def test_one_seed_is_a_multiple_of_64_and_the_other_is_not():
    a, w = sc.seed_case("aligned"), sc.seed_case("wall")
    assert len(a["ids"]) % 64 == 0 and len(w["ids"]) % 64 != 0, (len(a["ids"]), len(w["ids"]))
    assert len(a["ids"]) > 64 and len(w["ids"]) > 64  # above the tiny-tree path of the seed
    c = tc.base()
    for d in (a, w):
        assert len(d["ids"]) + sc.STREAM <= c["n"] and d["og2"][c["xs"][0], c["xs"][1]] == 0
        assert int(d["alive"].sum()) == len(d["ids"]) and len(d["samples"]) == sc.STREAM


@pytest.mark.parametrize("which", ["aligned", "wall"])
def test_the_rejected_run_covers_a_whole_block_and_what_else_is_planted(which):
    d = sc.seed_case(which)
    lo, hi = d["run"]
    g = sc.grown(which, sc.STREAM)
    assert hi - lo >= 64 and any(lo <= 64 * k and 64 * (k + 1) <= hi for k in range(4))  # a block of the launch commits nothing
    assert not g.accept_log[lo:hi].any()
    s, og2 = d["samples"], d["og2"]
    blocked = og2[s[:, 0], s[:, 1]] != 0
    assert blocked[3] and blocked[41] and blocked[lo:hi].sum() >= 30 and not g.accept_log[blocked].any()
    seeded = {(int(x), int(y)) for x, y in d["seed"][0][1:]}
    dup = np.array([(int(x), int(y)) in seeded for x, y in s])
    assert dup[2] and dup[40] and dup[lo:hi].sum() >= 30 and not g.accept_log[dup].any()
    a = d["twin"]
    assert a < 7 and (s[7] == s[a]).all() and g.accept_log[a] == 1 and g.accept_log[7] == 0  # the second of two equal samples of one block
    assert (s[9] == tc.base()["xs"]).all() and g.accept_log[9] == 1  # the root's cell becomes a vertex once
    outside = np.ones(sc.STREAM, dtype=bool)
    outside[lo:hi] = False
    for k in range(sc.blocks(sc.STREAM)):  # every other block grows the tree (a block with 32 free draws and more: 8 vertices at the least)
        out = outside[64 * k:64 * (k + 1)]
        if out.sum() >= 32:
            assert g.accept_log[64 * k:64 * (k + 1)][out].sum() >= 8, k


@pytest.mark.parametrize("which", ["aligned", "wall"])
def test_every_grow_is_a_prefix_of_the_longest(which):
    """growref.grow per m: the loop of the first m iterations of the longest run, then its own goal connection"""
    full = sc.grown(which, sc.STREAM)
    for m in sc.GROW_M:
        g = sc.grown(which, m)
        assert g.j0 == len(sc.seed_case(which)["ids"]) and np.array_equal(g.accept_log, full.accept_log[:m]) and np.array_equal(g.jlog, full.jlog[:m])
        assert g.j == g.j0 + int(full.accept_log[:m].sum()) and np.array_equal(g.pts[:g.j], full.pts[:g.j])
        assert g.found == 1 and g.status == growref.ST_OK  # (the kept seed sees the goal or the grown tree does)


def test_the_rerooted_and_the_relaxed_seed_grow():
    r = sc.reroot_vertex()
    d = sc.seed_case("wall")
    assert d["alive"][r] and r > 0
    for m in sc.SEED_M:
        R, g = sc.rerooted(m)
        assert len(R.ids) > 64 and g.j0 == len(R.ids) and g.j > g.j0 and (g.pts[0] == tc.base()["ro"].pts[r]).all()
        X, g = sc.relaxed(m)
        assert len(X.ids) == len(d["ids"]) and X.fell > 0 and g.j0 == len(X.ids) and g.j > g.j0


def test_the_late_second_block_is_the_heavy_one():
    d = sc.late_case()
    ro, g, more = d["ro"], d["grown"], d["more"]
    assert ro.j > 4096 + 64 and d["n"] - ro.j >= len(more) == sc.LATE["m"] == 2 * sc.SB and g.j0 == ro.j
    vertices = {(int(x), int(y)) for x, y in ro.pts[1:ro.j]}
    assert all((int(x), int(y)) in vertices for x, y in more[:64]) and not g.accept_log[:64].any()  # block 1: nothing to resolve
    assert (ro.pts[g.nearest_log[:64]] == more[:64]).all()  # (each one's nearest vertex is the vertex on its cell)
    acc = g.accept_log[64:]
    assert acc.sum() >= 32 and g.sum_near >= 1000 * int(acc.sum())  # block 2: near sets of a thousand vertices and more on average


# ------------------------------------------------------------------------------------------------ b. the same batch again
def test_the_relaunches_change_their_block_count_every_time():
    ns = sc.RELAUNCH_NS
    assert ns == (257, 65, 1, 129, 64, 193, 2) and max(ns) <= sc.RELAUNCH_CAP
    nb = [sc.blocks(n) for n in ns]
    assert nb == [5, 2, 1, 3, 1, 4, 1] and all(a != b for a, b in zip(nb, nb[1:]))
    for n in ns:
        st, ro = sc.relaunch(n)["plan"]
        assert ro.j >= min(n, 2) and len(ro.accept_log) == n
    assert sc.relaunch(257)["plan"][1].j > 129  # the second shift's blocks commit vertices too


def test_the_informed_query_goes_through_the_unit_ball_hand_over():
    d = sc.informed()
    st0, ro0 = d["first"]
    assert st0 == oracle.ORC_NEED_UNITBALL and 0 < ro0.i_switch < d["n"]
    st, ro = d["plan"]
    assert st == 0 and ro.found and ro.i_switch == ro0.i_switch and np.isfinite(ro.cbest_log[ro.i_switch:]).all()
    st1, ro1 = sc.relaunch(sc.INFORMED_N)["plan"]
    assert st1 == 0 and ro1.found


# ------------------------------------------------------------------------------------------------ c. go2goal across the shifts
@pytest.mark.parametrize("k", sc.SIZED_K)
def test_sized_trees_and_their_two_goals(k):
    assert sc.SIZED_K == (1, 2, 63, 64, 65, 127, 128, 129)
    seen, unseen = sc.sized_case(k, True), sc.sized_case(k, False)
    for c in (seen, unseen):
        assert c["ro"].j == k and c["alg"] == 0
    assert seen["st"] == 0 and seen["ro"].found == 1 and seen["ro"].vgoal == k
    ro = unseen["ro"]
    assert unseen["st"] == growref.ST_UNREACHABLE and ro.found == 0 and ro.vgoal == 0
    for v in range(k):  # no vertex sees the goal, in either direction
        assert not oracle.collisionfree(unseen["og8"], ro.pts[v], unseen["xg"])[0]
        assert not oracle.collisionfree(unseen["og8"], unseen["xg"], ro.pts[v])[0]
    # fewer vertices than members: with 129 workgroups every tree below 129 leaves members without a candidate, with 65 those below 65
    assert sum(k < 129 for k in sc.SIZED_K) == 7 and sum(k < 65 for k in sc.SIZED_K) == 4


@pytest.mark.parametrize("which", list(sc.TIES))
def test_the_ties_are_ties_and_fall_where_the_fold_says(which):
    c = sc.tie_case(which)
    ro = c["ro"]
    u, v = sc.TIES[which]
    assert c["st"] == 0 and ro.found and ro.j > 129 and ro.accept_log[:v].all()
    assert tuple(ro.pts[u]) == sc.TIE_P and tuple(ro.pts[v]) == sc.TIE_Q and ro.parent[u] == ro.parent[v] == 0
    ku, kv = sc.goal_key(c, u), sc.goal_key(c, v)
    assert ku.view(np.int64) == kv.view(np.int64) and ku == 100.0
    assert ro.parent[ro.vgoal] == u < v and ro.vcost[ro.vgoal] == ku  # the oracle took the lower index
    for k in range(ro.j):  # every other vertex costs more or does not see the goal
        if k not in (u, v):
            assert sc.goal_key(c, k) > ku or not oracle.collisionfree(c["og8"], ro.pts[k], c["xg"])[0], k
    assert not oracle.collisionfree(c["og8"], ro.pts[0], c["xg"])[0] and sc.goal_key(c, 0) < ku  # (the root: cheaper, behind the wall)
    mu, mv = sc.member_of(u, 2), sc.member_of(v, 2)
    assert 1 <= mu <= 64 < mv <= 128  # the lower index on the first shift, the higher on the second
    if which == "same_lane":
        assert sc.lane_of(mu) == sc.lane_of(mv) and mv == mu + 64  # members l + 1 and l + 65 of one lane
    else:
        assert sc.lane_of(mu) != sc.lane_of(mv)
    assert sc.member_of(u, 1) != sc.member_of(v, 1) and 0 not in (sc.member_of(u, 1), sc.member_of(v, 1))  # one shift: two workers' answers
    assert sc.member_of(129, 2) == 0 and sc.member_of(65, 1) == 0 and sc.lane_of(65) == 0 and sc.lane_of(128) == 63


# ------------------------------------------------------------------------------------------------ d. maps that break kernels
def test_the_strip_map_and_the_pocket_cases():
    og8 = sc.strip_grid()
    S = sc.STRIP
    assert og8.shape == (300, 260) and og8[S["xs"]] == 0 and og8[S["xg"]] == 0
    st, ro, samples = _strip_plan()
    assert st == 0 and ro.found and ro.j > 2000
    assert len({int(p[0]) // 60 for p in ro.pts[:ro.j]}) == 5  # the tree reaches every strip
    assert [c["alg"] for c in farnn.PIPE_CASES] == [0, 1, 0, 0] and all(c["n"] == 3000 for c in farnn.PIPE_CASES)


def _strip_plan():
    from rrtplanner_amd import hostprep
    S, og8 = sc.STRIP, sc.strip_grid()
    samples = hostprep.draw_free_samples(np.random.default_rng(S["seed"]), np.argwhere(og8 == 0), S["n"])
    st, ro = oracle.plan(og8, S["n"], 1, S["xs"], S["xg"], samples, r2_rewire=hostprep.radius_threshold(S["rr"]))
    return st, ro, samples


# ------------------------------------------------------------------------------------------------ e. a team that loses member 1
def test_the_query_of_the_team_that_loses_a_member():
    d = sc.fault_case()
    st, ro = d["plan"]
    assert d["n"] == 600 and sc.blocks(d["n"]) == 10 and st == 0 and ro.found and ro.j > 300
