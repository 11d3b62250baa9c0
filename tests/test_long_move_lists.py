"""Positions with more than TG_MAX_MOVES (512) legal moves, on the CPU: the generators of posgen.long_list_states, the oracle's
uncut move list, and the teeth of the solver reference's give-up rule (include/takgpu.h, "Move-list capacity inside the tree").
Everything the GPU tests of tests/test_gpu_long_move_lists.py rely on is asserted here by the oracle / the reference alone."""
import functools

import numpy as np

import posgen
import tactics_ref as T
from oracle import oracle as orc

N = 6
COUNTS = {"max": 1076, "S": 763, "S_swapped": 763, "S_mirror": 763, "e512": 512, "e513": 513, "e512_bare": 512}
FIVE_531 = "11111,x,x,x,11111/x,x,x,11111,x/x,x,22221,22221,x/x,x,22221,x,22221/x,x,x,22221,x 1 41"


@functools.lru_cache(maxsize=None)
def family():
    return posgen.long_list_states(orc, N)


def _all_states():
    fam = family()
    return np.stack(list(fam["states"].values()) + [r for r, _, _ in fam["roots"].values()])


def test_every_state_is_a_consistent_ongoing_position():
    sts = _all_states()
    assert posgen.is_position(sts, N).all() and posgen.reserves_consistent(sts, N).all()
    assert (orc.result(N, sts) == 0).all()
    for name, st in family()["states"].items():
        assert orc.to_tps(N, st) == orc.to_tps(N, posgen.from_tps(N, orc.to_tps(N, st))), name
    for name, tps in posgen.LONG_LIST_TPS.items():
        assert orc.to_tps(N, family()["states"][name]) == tps, name


def test_counts_and_the_edge_pair():
    fam = family()
    for name, want in COUNTS.items():
        assert int(orc.movegen_full(N, fam["states"][name])[1][0]) == want, name
    assert int(orc.movegen_full(N, fam["states"]["W"])[1][0]) > 512
    for name, (root, move, child) in fam["roots"].items():
        moves, counts = orc.movegen(N, root)
        assert counts[0] <= 128 and move in moves[0, : counts[0]], name  # the root's own list is short
        ch, status = orc.play(N, root, [move])
        assert status[0] == 0 and np.array_equal(ch[0], fam["states"][child]), name


def test_edge_roots_and_the_off_by_one_teeth():
    """E512 / E513: black to move with placements only; the longest child list is exactly 512 / 513.  A reference that gives up at
    512 moves already (capacity 511: `>=` for `>`) is told from the rule on E512 by the GPU tests' comparison."""
    fam = family()
    for name, longest, how_many in (("E512", 512, 39), ("E513", 513, 44)):
        root = fam["edge_roots"][name]
        assert posgen.is_position(root[None], N).all() and posgen.reserves_consistent(root[None], N).all() and orc.result(N, root)[0] == 0
        moves, counts = orc.movegen(N, root)
        ch, status = orc.play(N, np.repeat(root[None], counts[0], axis=0), moves[0, : counts[0]])
        assert not status.any() and (orc.result(N, ch) == 0).all()
        cc = orc.movegen_full(N, ch)[1]
        assert cc.max() == longest and (cc == longest).sum() == how_many, name
    roots = np.stack([fam["edge_roots"]["E512"], fam["edge_roots"]["E513"]])
    for depth in (2, 3):
        rule, off = T.Ref(N).solve(roots, depth, False), T.Ref(N, capacity=511).solve(roots, depth, False)
        assert list(rule["budget_hit"]) == [0, 1] and list(off["budget_hit"]) == [1, 1]
        assert T.compare_with_give_up(rule, off) != []


def test_the_committed_depth4_answers_belong_to_the_positions():
    import hashlib
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_list_depth4.json")) as f:
        doc = json.load(f)
    roots = np.stack([family()["roots"][k][0] for k in doc["names"]])
    assert hashlib.sha256(roots.tobytes()).hexdigest() == doc["sha256"] and doc["depth"] == 4
    for mode in ("default", "road_only"):
        for name, row in zip(doc["names"], doc[mode]):
            moves, counts = orc.movegen(N, family()["roots"][name][0])
            assert row["counts"] == counts[0] and row["moves"] == [int(x) for x in moves[0, : counts[0]]]
    i = doc["names"].index("R")
    j = doc["default"][i]["moves"].index(family()["roots"]["R"][1])
    assert doc["default"][i]["move_values"][j] == 0 and doc["default"][i]["budget_hit"] == 1


def test_the_defences_of_S_lie_behind_the_capacity():
    fam = family()
    for name in ["S", "S_swapped"] + [f"S_sym{s}" for s in fam["s_images"]]:
        moves, res, hit = posgen.reply_table(orc, N, fam["states"][name])
        assert len(moves) == 763 and (res == 0).all(), name
        assert hit[:512].all(), name                       # after each of the first 512 moves the other side wins at once
        defences = np.flatnonzero(~hit)
        assert len(defences) == 3 and defences.min() >= 512, (name, defences)  # flat, wall and capstone on the open square
    # the images that keep the defence behind index 511: recorded, so that a change of the move order shows
    assert fam["s_images"] == [1, 5, 6]
    # the control: mirrored, the open file is file a and the defences are the first three moves of the list
    moves, res, hit = posgen.reply_table(orc, N, fam["states"]["S_mirror"])
    assert list(np.flatnonzero(~hit)) == [0, 1, 2]
    # W: the mover has an instant road among the first 512 moves
    moves, res, hit = posgen.reply_table(orc, N, fam["states"]["W"])
    assert np.flatnonzero(res == 1).min() < 512


def test_the_uncut_list_agrees_with_movegen():
    sts = np.concatenate([_all_states(), orc.random_positions(N, 64, seed=5, max_plies=60)])
    full, fc = orc.movegen_full(N, sts)
    cut, cc = orc.movegen(N, sts)
    assert np.array_equal(fc, cc) and fc.max() == 1076 and fc.min() < 512
    for i in range(len(sts)):
        k = min(int(fc[i]), 512)
        assert np.array_equal(full[i, :k], cut[i, :k])
        assert len(set(full[i, : fc[i]].tolist())) == fc[i]  # every move once
    # every move of the uncut list is legal and the tail (behind 512) is played like the head
    big = family()["states"]["max"]
    _, status = orc.play(N, np.repeat(big[None], 1076, axis=0), full[0, :1076])
    assert not status.any()


def test_5x5_has_a_position_above_the_capacity():
    """eight mover-topped stacks of five (found by hill climbing over stack heights): 531 moves.  The GPU tests stay on 6×6."""
    st = posgen.from_tps(5, FIVE_531)
    assert posgen.is_position(st[None], 5).all() and posgen.reserves_consistent(st[None], 5).all() and orc.result(5, st)[0] == 0
    assert int(orc.movegen_full(5, st)[1][0]) == 531


@functools.lru_cache(maxsize=None)
def solved(variant, capacity, depth=3):
    fam = family()
    roots = np.stack([r for r, _, _ in fam["roots"].values()])
    return T.Ref(N, variant=variant, capacity=capacity).solve(roots, depth, False)


def _row(name):
    return list(family()["roots"]).index(name)


def _move_value(out, name):
    i = _row(name)
    return int(out["move_values"][i, list(out["moves"][i]).index(family()["roots"][name][1])])


def test_give_up_rule_of_the_reference():
    rule, exact = solved(None, 512), solved(None, None)
    assert T.sound(exact, rule, 3) == []
    assert not exact["budget_hit"].any()
    for name in ("R", "R_swapped"):  # the exact value of the move into S is "not proven"; the rule says so and reports it
        assert _move_value(exact, name) == 0 and _move_value(rule, name) == 0 and rule["budget_hit"][_row(name)] == 1
    # a win among the first 512 moves of a cut list is a win
    assert _move_value(exact, "R_W") == -2 and _move_value(rule, "R_W") == -2 and rule["value"][_row("R_W")] == -2
    assert np.array_equal(rule["value"], exact["value"])  # on this family nothing else is lost to the rule


def test_teeth_a_solver_that_cuts_x_test_is_rejected():
    """the parent's behaviour: the first 512 moves of S taken for all of them — +3 for the move into S"""
    planted, rule, exact = solved("cut_x_test", 512), solved(None, 512), solved(None, None)
    assert _move_value(planted, "R") == 3 and _move_value(planted, "R_swapped") == 3
    assert T.compare_with_give_up(rule, planted) != []
    assert T.sound(exact, planted, 3) != []
    assert _move_value(planted, "R_mirror") == 0  # the control: the defence is inside the first 512, the cut does no harm there


def test_teeth_a_give_up_that_is_not_reported_is_rejected():
    planted, rule = solved("silent_give_up", 512), solved(None, 512)
    assert T.compare(rule, planted, budget_free=False) == []  # same values: only the report is missing
    assert T.compare_with_give_up(rule, planted) != []
