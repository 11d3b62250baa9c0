"""The forced-win reference (tests/tactics_ref.py) itself: hand-made positions with their values written out, the teeth of the
comparison the GPU tests use (each planted mistake is rejected on one of their sets; the two about draws on every set that puts the
50-reversible-plies draw inside the tree), and a recomputed sample of the committed depth-4 / depth-5 / depth-6 cases.  No GPU."""
import json
import os

import numpy as np
import pytest

import posgen
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


@pytest.mark.parametrize("variant", ("no_suicide", "draw_is_loss", "min_at_lost", "last_best", "no_early_stop"))
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


def _reversible_depth(name):
    return 4 if name.endswith("_r47") else 3


@pytest.mark.parametrize("variant", ("reversible_is_ongoing", "draw_is_loss"))
@pytest.mark.parametrize("name", sorted(T.REVERSIBLE))
def test_the_reversible_sets_reject_a_mistake_about_the_draw(name, variant):
    """the sets whose header counter stands at 49, 48 and 47: a solver that searches on through the 50-reversible-plies draw, or
    takes it for a loss, is rejected by the GPU tests' comparison on every one of them (on the rows whose ALL_MOVES table the counter
    changes, the first 3 of them: the planted solver is slow where it plays on)"""
    base, k, _ = T.REVERSIBLE[name]
    depth = _reversible_depth(name)
    scan = k if base == "s5_200" else 24  # (the tall-stack sets move few rows and their references are cheap; the others move a third)
    good, plain = T.reference(name, depth, True), T.Ref(T.BOARD[base]).solve(T.positions(base)[:scan], depth, True)
    rows = np.nonzero((good["move_values"][:scan] != plain["move_values"]).any(axis=1))[0][:3]
    assert len(rows) >= 2
    bad = T.Ref(T.BOARD[name], variant).solve(T.positions(name)[rows], depth, True)
    assert T.compare({f: good[f][rows] for f in T.FIELDS}, bad) != []
    assert T.compare({f: good[f][rows] for f in T.FIELDS}, T.Ref(T.BOARD[name]).solve(T.positions(name)[rows], depth, True)) == []


def test_playouts_alone_hardly_see_the_reversible_draw():
    """the gap the sets above close.  On the 400 play-out positions at depth 3 with the early stop — the comparison the other planted mistakes are tried on — a
    solver that searches on through the 50-reversible-plies draw differs in three move values of ONE position (row 115, whose play-out
    happens to have brought the counter near 50): rejected, but by a single row, and on the tall-stack set not at all."""
    good = T.reference("p5_400", 3, False)
    bad = T.reference("p5_400", 3, False, "reversible_is_ongoing")
    assert np.array_equal(good["value"], bad["value"]) and np.array_equal(good["best"], bad["best"])
    rows, cols = np.nonzero(good["move_values"] != bad["move_values"])
    assert rows.tolist() == [115, 115, 115]
    assert int(posgen.header(T.positions("p5_400")[115:116], "reversible_plies")[0]) >= 47
    assert T.compare(T.reference("s5_200", 3, False), T.reference("s5_200", 3, False, "reversible_is_ongoing")) == []  # the tall stacks: no tooth at all


def test_the_committed_cases_are_the_reference():
    """a sample of tests/golden/solve_cases.json recomputed (make_solve_cases.py rebuilds all of it): one position of
    each of the values +5, -4, +3 and +1 at depth 4 and 5, one of -6 at depth 6 and one 6×6 position of +5 at depth 5"""
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
    # depth 6 and 6×6: one position of value -6 (a tall-stack one: the cheapest to recompute) and one 6×6 position of value +5
    tall, six = doc["tall_stacks"], doc["six"]
    assert tall["value_counts_depth5_first_100"] == {"-4": 1, "-2": 1, "0": 29, "1": 69} and len(tall["cases"]) == 29
    assert six["value_counts_depth5_all_80"] == {"-4": 3, "-2": 3, "0": 16, "1": 52, "3": 2, "5": 4}
    deep6 = [c["depth6"]["value"] for c in cases] + [c["depth6"]["value"] for c in tall["cases"]]
    assert deep6.count(-6) == 3 and [c["index"] for c in tall["cases"] if c["depth6"]["value"] == -6] == [43, 99]
    assert [c["index"] for c in cases if c["depth6"]["value"] == -6] == [44]
    assert all(c["depth5"]["value"] == 0 for c in tall["cases"])
    T.require_classes([c["depth5"]["value"] for c in six["cases"]], (1, -2, 3, -4, 5))
    assert sum("depth6" in c for c in six["cases"]) == 9 + len(six["depth6_unproven"]) and len(six["depth6_unproven"]) <= 6
    for block, depth, wanted in ((tall, 6, -6), (six, 5, 5)):
        c = next(c for c in block["cases"] if c[f"depth{depth}"]["value"] == wanted)
        n = T.BOARD[block["set"]]
        value, best, moves, vals = T.Ref(n).solve_one(T.positions(block["set"])[c["index"]], depth, False)
        e = c[f"depth{depth}"]
        assert (value, best, [int(m) for m in moves], vals) == (e["value"], e["best"], c["moves"], e["move_values"]), (block["set"], c["index"])
