"""The road-only reference (tests/tinue_ref.py) itself: hand-made positions with their values written out, the teeth of the
comparison the GPU tests use (each planted mistake of this mode, and the default mode's own answer, is rejected on one of their
sets), a recomputed sample of the committed cases, and the implication between the two modes.  No GPU."""
import numpy as np
import pytest

import tactics_ref as T
import tinue_ref as R
from oracle import oracle

# 5×5, e5 alone empty, row 3 all walls, the other rows a chequerboard (no two flats of a colour touch: no road is one move away).
# White has 10 flats and black 9; white to move.  Any stone on e5 fills the board.
_W = "d1 a2 c2 e2 a4 c4 e4 b5 d5 Sa3 Sb3".split()
_B = "c1 e1 b2 d2 b4 d4 a5 c5 Sc3 Sd3 Se3".split()
FULL_BUT_ONE = ["a1", "b1"] + [m for pair in zip(_W, _B) for m in pair]


def _solve(n, ptn, depth, road_only, half_komi=0, all_moves=True):
    """→ (value, best as PTN or None, {PTN move: value} of the non-zero entries, {PTN move: result code after it})"""
    s = oracle.from_ptn(n, ptn, half_komi)
    r = (R.TinueRef(n) if road_only else T.Ref(n)).solve(s[None], depth, all_moves)
    c = int(r["counts"][0])
    names = [oracle.format_move(n, m) for m in r["moves"][0, :c]]
    after, _ = oracle.play(n, np.repeat(s[None], c, axis=0), r["moves"][0, :c])
    value = int(r["value"][0])
    return (value, oracle.format_move(n, r["best"][0]) if value else None,
            {m: int(v) for m, v in zip(names, r["move_values"][0, :c]) if v}, dict(zip(names, (int(x) for x in oracle.result(n, after)))))


def test_a_road_in_one():
    # white a1 b1 c1, black a4 b4 c4, white to move: d1 completes the row — in both modes
    for road_only in (True, False):
        assert _solve(4, "a4 a1 b1 b4 c1 c4", 1, road_only)[:3] == (1, "d1", {"d1": 1})


def test_a_flat_win_in_one_is_no_road():
    value, best, vals, res = _solve(5, FULL_BUT_ONE, 1, False)
    assert {m: r for m, r in res.items() if r} == {"e5": 2, "Se5": 2, "Ce5": 2}  # WhiteFlat, and no other move ends the game
    assert (value, best, vals) == (1, "e5", {"e5": 1, "Se5": 1, "Ce5": 1})
    assert _solve(5, FULL_BUT_ONE, 1, True)[:3] == (0, None, {})
    assert _solve(5, FULL_BUT_ONE, 3, True, all_moves=False)[0] == 0  # … and it stays unproven: the flat win is not searched past either


def test_filling_the_board_for_the_opponent_is_no_loss():
    # the same board with komi 3: 11 white flats against 9 + 3, every stone on e5 ends the game in BlackFlat
    value, best, vals, res = _solve(5, FULL_BUT_ONE, 1, False, half_komi=6)
    assert {m: r for m, r in res.items() if r} == {"e5": 4, "Se5": 4, "Ce5": 4}
    assert (value, vals) == (0, {"e5": -1, "Se5": -1, "Ce5": -1})
    assert _solve(5, FULL_BUT_ONE, 1, True, half_komi=6)[:3] == (0, None, {})


def test_a_move_that_completes_both_roads_is_the_movers_road():
    # black a5 b5 c5 d5 and a black flat under the white stone on e5, white a4 b4 c4 d4: e5- lands on e4 and uncovers e5
    ptn = "a5 a4 b4 b5 c4 c5 e4 e5 e4+ d5 d4 a1"
    value, best, vals, res = _solve(5, ptn, 1, True)
    assert res["e5-"] == 1 and vals == {"e4": 1, "Ce4": 1, "e5-": 1, "2e5-": 1} and (value, best) == (1, "e4")
    # black's row is a road too once the stone has left
    s = oracle.from_ptn(5, ptn)
    lifted, _ = oracle.play(5, s[None], [oracle.parse_move(5, "e5-")])
    flats = oracle.to_tps(5, lifted[0]).split(" ")[0].split("/")
    assert flats[0] == "2,2,2,2,2" and flats[1] == "1,1,1,1,1"  # both rows stand complete


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_the_comparison_rejects_a_planted_mistake(variant):
    """flats counted as a win at the attacker's last ply only, flats counted as a loss in X, the opponent's flat win searched on: the
    tall-stack play-outs at depth 3 with the early stop, one of the GPU tests' own comparisons, reject each"""
    good = R.reference("s5_200", 3, False)
    bad = R.Planted(5, variant).solve(R.positions("s5_200"), 3, False)
    assert T.compare(good, bad) != []
    assert T.compare({f: good[f][:40] for f in T.FIELDS}, R.TinueRef(5).solve(R.positions("s5_200")[:40], 3, False)) == []


@pytest.mark.parametrize("name", ("p5_400", "p6_200", "s5_200"))
def test_the_modes_differ_and_a_road_proof_is_a_proof(name):
    """on the play-out sets the default mode's answer is rejected as a road-only answer (at least 100 `value` rows differ), and
    by the reference alone: road-only v > 0 ⇒ default 0 < v' <= v; road-only v < 0 ⇒ default v' < 0 and |v'| <= |v|"""
    road, plain = R.reference(name, 3, False), R.reference(name, 3, False, None, False)
    assert T.compare(road, plain, budget_free=False) != []
    v, w = road["value"].astype(int), plain["value"].astype(int)
    assert int((v != w).sum()) >= 100
    T.require_classes(v, (1,))
    assert ((w[v > 0] > 0) & (w[v > 0] <= v[v > 0])).all()
    assert ((w[v < 0] < 0) & (-w[v < 0] <= -v[v < 0])).all()


def test_the_mined_sets_hold_the_deep_classes_and_hardly_tell_the_modes_apart():
    """why both kinds of input are needed: the mined positions carry the road tactics (−2 and 3 by the dozen, which the play-outs
    lack) and give the same values in both modes"""
    for name, classes in (("m5_400", (1, -2, 3)), ("m6_200", (1, -2, 3))):
        road, plain = R.reference(name, 3, False), R.reference(name, 3, False, None, False)
        T.require_classes(road["value"], classes)
        assert (road["value"] == -2).sum() >= 30 and (road["value"] == 3).sum() >= 10
        assert np.array_equal(road["value"], plain["value"])


def test_the_committed_cases_are_the_reference():
    """a sample of tests/golden/tinue_cases.json recomputed (make_tinue_cases.py rebuilds all of it): on 5×5 one position of each
    of the values 5, −4, 3, −2, 1 and 0 at depth 4 and 5, on 6×6 one of −4, 3 and 0 at depth 4"""
    doc = R.cases()
    five, six = doc["five"], doc["six"]
    assert R.positions("m5_400").shape == (400, oracle.state_bytes(5)) and R.positions("m6_200").shape == (200, oracle.state_bytes(6))
    assert five["value_counts_depth4_mined"] == {"-4": 8, "-2": 44, "0": 667, "1": 402, "3": 24}
    assert five["value_counts_depth4_committed"] == {"-4": 8, "-2": 44, "0": 200, "1": 124, "3": 24}
    assert five["value_counts_depth5_committed"] == {"-4": 8, "-2": 44, "0": 195, "1": 124, "3": 24, "5": 5}
    assert six["value_counts_depth3_mined"] == {"-2": 33, "0": 380, "1": 302, "3": 10}
    assert six["value_counts_depth4_committed"] == {"-4": 3, "-2": 33, "0": 97, "1": 57, "3": 10}
    v5 = [c["depth5"]["value"] for c in five["cases"]]
    assert len(v5) == 8 + 24 + 5 + 16 + 16 and sorted(c["index"] for c in five["cases"]) == [c["index"] for c in five["cases"]]
    T.require_classes(v5, (1, -2, 3, -4, 5))
    T.require_classes([c["depth4"]["value"] for c in five["cases"]], (1, -2, 3, -4))
    v6 = [c["depth4"]["value"] for c in six["cases"]]
    assert len(v6) == 3 + 10 + 16 + 16 + 1  # (one more −2: the first 16 shallow ones hold a single one)
    T.require_classes(v6, (1, -2, 3, -4))
    for block, n, picks, depths in ((five, 5, [v5.index(x) for x in (5, -4, 3, -2, 1, 0)], (4, 5)),
                                    (six, 6, [v6.index(x) for x in (-4, 3, 0)], (4,))):
        states = R.positions(block["set"])
        for j in picks:
            c = block["cases"][j]
            for depth in depths:
                value, best, moves, vals = R.TinueRef(n).solve_one(states[c["index"]], depth, False)
                e = c[f"depth{depth}"]
                assert (value, best, [int(m) for m in moves], vals) == (e["value"], e["best"], c["moves"], e["move_values"]), (n, c["index"], depth)


def test_forced_line_on_the_reference():
    """analysis.forced_line needs no GPU: on the reference's solver it gives, for a committed position of value 3, three legal moves
    that end in the mover's road, and nothing where nothing is proven"""
    from tak_amd.analysis import forced_line

    states, ref = R.table("five", 4)
    j = int(np.nonzero(ref["value"] == 3)[0][0])
    line = forced_line(R.RefSolver(5), states[j], 4, road_only=True)
    assert len(line) == 3 and line[0] == int(ref["best"][j])
    cur = states[j : j + 1]
    for m in line:
        assert int(oracle.result(5, cur)[0]) == 0 and m in oracle.movegen(5, cur)[0][0, : oracle.movegen(5, cur)[1][0]]
        cur, status = oracle.play(5, cur, [m])
        assert not status.any()
    assert int(oracle.result(5, cur)[0]) == (1 if int(states[j, -16 + 1]) == 0 else 3)
    k = int(np.nonzero(ref["value"] == 0)[0][0])
    assert forced_line(R.RefSolver(5), states[k], 3, road_only=True) == []
