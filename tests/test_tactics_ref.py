"""The forced-win reference (tests/tactics_ref.py) itself: hand-made positions with their values written out, the teeth of the
comparison the GPU tests use (each planted mistake is rejected on one of their sets), and a recomputed sample of the committed
depth-4 / depth-5 cases.  No GPU."""
import json
import os

import numpy as np
import pytest

import tactics_ref as T
from oracle import oracle


def _solve(n, ptn, depth, all_moves=True, variant=None):
    """→ (value, best as PTN or None, {PTN move: value} of the non-zero entries, {PTN move: result code after it})"""
    s = oracle.from_ptn(n, ptn)
    r = T.Ref(n, variant).solve(s[None], depth, all_moves)
    c = int(r["counts"][0])
    names = [oracle.format_move(n, m) for m in r["moves"][0, :c]]
    after, _ = oracle.play(n, np.repeat(s[None], c, axis=0), r["moves"][0, :c])
    value = int(r["value"][0])
    return (value, oracle.format_move(n, r["best"][0]) if value else None,
            {m: int(v) for m, v in zip(names, r["move_values"][0, :c]) if v}, dict(zip(names, (int(x) for x in oracle.result(n, after)))))


def test_a_road_in_one():
    # white a1 b1 c1, black a4 b4 c4, white to move: d1 completes the row
    value, best, vals, _ = _solve(4, "a4 a1 b1 b4 c1 c4", 1)
    assert (value, best, vals) == (1, "d1", {"d1": 1})
    assert _solve(4, "a4 a1 b1 b4 c1 c4", 3, all_moves=False)[:2] == (1, "d1")


def test_a_two_way_threat():
    # white a2 c2 b1 b3, black a4 c4 d3 d1, white to move: b2 threatens d2 (row 2) and b4 (column b) at once, and no black stone
    # stands next to b2
    attacker = "a4 a2 c2 c4 b1 d3 b3 d1"
    assert _solve(4, attacker, 3) == (3, "b2", {"b2": 3}, _solve(4, attacker, 1)[3])
    assert _solve(4, attacker, 2)[0] == 0  # not within 2 plies
    value, best, vals, res = _solve(4, attacker + " b2", 3)
    assert value == -2 and best == "a1" and len(vals) == len(res) == 24 and set(vals.values()) == {-2}  # every defence loses; the first move is `best`
    assert _solve(4, attacker + " b2", 1)[0] == 0


def test_a_move_that_completes_only_the_opponents_road():
    # black a1 c1 d1 and a black flat under the white stone on b1: lifting that stone (b1+) leaves black's row and nothing for white
    value, best, vals, res = _solve(4, "a1 b2 a4 b1 b2- c1 a3 d1", 1)
    assert res["b1+"] == 3 and vals == {"b1+": -1} and (value, best) == (0, None)
    assert _solve(4, "a1 b2 a4 b1 b2- c1 a3 d1", 1, variant="no_suicide")[2] == {}


def test_a_move_that_completes_both_roads_wins_for_the_mover():
    # as above, but the lifted stone lands on b2 between white's a2, c2, d2: both rows are roads, the mover's counts (dragon clause)
    value, best, vals, res = _solve(4, "a1 b2 a2 b1 b2- c1 c2 d1 d2 a4", 1)
    assert res["b1+"] == 1 and vals["b1+"] == 1 and vals == {"b1+": 1, "2b1+": 1, "b2": 1} and (value, best) == (1, "b1+")


def test_a_flat_win_by_filling_the_board():
    # 3×3 with c3 alone empty, white flats a1 c1 b2 a3 against one black flat and three walls: a flat or a wall on c3 fills the board
    value, best, vals, res = _solve(3, "b1 a1 c1 Sa2 b2 Sc2 a3 Sb3", 1)
    assert res["c3"] == 2 and res["Sc3"] == 2  # WhiteFlat
    assert vals == {"b2-": 1, "c3": 1, "Sc3": 1} and res["b2-"] == 1 and (value, best) == (1, "b2-")  # (b2- is a road; it comes first)


def test_the_only_escape_is_a_draw():
    """a 3×3 position found by a random search over PTN games: black has four moves, three lose (a wall that ends the game on
    flats, two that allow a road) and one ends the game in a draw — value 0, not a loss"""
    ptn = "c3 a3 Sb3 a2 Sb1 c3- b2 Sc1 b1+ Sa1 b2< c2+ Sb1"
    value, best, vals, res = _solve(3, ptn, 2)
    assert len(res) == 4 and vals == {"c1+": -2, "Sc2": -1, "c3-": -2} and (value, best) == (0, None)
    (escape,) = [m for m in res if m not in vals]
    assert res[escape] in (5, 6)
    assert _solve(3, ptn, 2, variant="draw_is_loss")[0] == -2


@pytest.mark.parametrize("variant", T.VARIANTS)
def test_the_comparison_rejects_a_planted_mistake(variant):
    """on the 400 playout positions at depth 3 with the early stop, one of the GPU tests' own comparisons (the early-stop variant on
    a prefix: it is the ALL_MOVES table, the expensive one)"""
    rows = slice(0, 100) if variant == "no_early_stop" else slice(None)
    good = T.reference("p5_400", 3, False)
    T.require_classes(good["value"][rows], (1, -2, 3))
    bad = T.Ref(5, variant).solve(T.positions("p5_400")[rows], 3, False)
    assert T.compare({f: good[f][rows] for f in T.FIELDS}, bad) != []
    assert T.compare({f: good[f][rows] for f in T.FIELDS}, T.Ref(5).solve(T.positions("p5_400")[rows][:40], 3, False)) != []  # (a shorter batch is no match either)
    assert T.compare({f: good[f][:40] for f in T.FIELDS}, T.Ref(5).solve(T.positions("p5_400")[:40], 3, False)) == []


def test_the_committed_cases_are_the_reference():
    """a sample of tests/golden/solve_cases.json recomputed (make_solve_cases.py rebuilds all of it): one position of
    each of the values +5, -4, +3 and +1"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_cases.json")) as f:
        doc = json.load(f)
    cases = doc["cases"]
    assert doc["value_counts_depth5_all_160"] == {"-4": 2, "-2": 9, "0": 44, "1": 96, "3": 6, "5": 3}
    values = [c["depth5"]["value"] for c in cases]
    assert sorted(c["index"] for c in cases) == [c["index"] for c in cases] and len(cases) == 11 + 16 + 16
    T.require_classes(values, (1, -2, 3, -4, 5))
    pick = [values.index(5), values.index(-4), values.index(3), values.index(1)]
    states = T.positions(doc["set"])
    ref = T.Ref(5)
    for j in pick:
        c = cases[j]
        for depth in (4, 5):
            value, best, moves, vals = ref.solve_one(states[c["index"]], depth, False)
            e = c[f"depth{depth}"]
            assert (value, best, [int(m) for m in moves], vals) == (e["value"], e["best"], c["moves"], e["move_values"]), (c["index"], depth)
