"""GPU gate of the road-only forced-win solver (TG_SOLVE_ROAD_ONLY of tg_solve / tg_search_solve) against tests/tinue_ref.py, the
plain statement of the road-only definitions in include/takgpu.h.  Integer work: every comparison is exact (tactics_ref.compare:
all of FIELDS row for row, budget_hit == 0).  Two kinds of input: the play-out sets of test_gpu_solve.py, where the two modes
disagree on most rows, and the committed mined positions (tests/golden/make_tinue_cases.py), where road tactics run deep.  Live
references only at depth <= 3; everything deeper comes from the committed cases.  Each test first asserts, by the reference alone,
the condition that makes it meaningful."""
import numpy as np
import pytest

import tactics_ref as T
import tinue_ref as R

pytestmark = pytest.mark.gpu

BUDGET = 1 << 22


@pytest.fixture(scope="module")
def engines():
    import tak_amd

    es = {n: tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=64,
                            policy_head=tak_amd.HEAD_FC5 if n == 5 else tak_amd.HEAD_CONV) for n in (5, 6)}
    yield es
    for e in es.values():
        e.close()


def _rows(ref, rows):
    return {f: ref[f][rows] for f in T.FIELDS}


@pytest.mark.parametrize("all_moves", [True, False])
@pytest.mark.parametrize("name", ["m5_400", "m6_200"])
def test_depth3_on_the_mined_positions(engines, name, all_moves):
    ref = R.reference(name, 3, all_moves)
    T.require_classes(ref["value"], (1, -2, 3))
    got = engines[R.BOARD[name]].solve(R.positions(name), 3, all_moves=all_moves, road_only=True, node_budget=BUDGET)
    print(f"road-only {name} depth 3 all_moves {all_moves}: values {T.class_counts(got['value'])}, nodes {int(got['nodes'].sum())}")
    assert T.compare(ref, got) == []


@pytest.mark.parametrize("name", ["p5_400", "p6_200"])
def test_depth3_where_the_modes_disagree(engines, name):
    """positions one ply before a game's end, mostly flat endings: the default mode's answer is wrong on more than 100 rows"""
    ref, plain = R.reference(name, 3, False), R.reference(name, 3, False, None, False)
    assert int((ref["value"] != plain["value"]).sum()) >= 100
    T.require_classes(ref["value"], (1,))
    got = engines[R.BOARD[name]].solve(R.positions(name), 3, road_only=True, node_budget=BUDGET)
    assert T.compare(ref, got) == []
    assert T.compare(plain, got, budget_free=False) != []


@pytest.mark.parametrize("block,depth", [("five", 4), ("five", 5), ("six", 4)])
def test_depths_4_and_5_from_the_committed_cases(engines, block, depth):
    states, ref = R.table(block, depth)
    T.require_classes(ref["value"], (1, -2, 3, -4) + ((5,) if depth == 5 else ()))
    got = engines[R.BOARD[R.cases()[block]["set"]]].solve(states, depth, road_only=True, node_budget=BUDGET)
    print(f"road-only {block} depth {depth}: nodes {int(got['nodes'].sum())}, largest position {int(got['nodes'].max())}")
    assert T.compare(ref, got) == []


def test_depth1_is_a_road_in_one(engines, orc):
    """value 1 exactly where some child's result is the mover's road, a move value +1 exactly on those children and −1 exactly where
    the child is the opponent's road: against oracle.result directly, tinue_ref takes no part"""
    roads = flats = 0
    for name in ("p5_400", "p6_200", "s5_200", "m5_400"):
        n, states = R.BOARD[name], R.positions(name)
        got = engines[n].solve(states, 1, all_moves=True, road_only=True)
        moves, counts = orc.movegen(n, states)
        assert np.array_equal(got["counts"], counts) and np.array_equal(got["moves"], moves)
        for i in range(len(states)):
            c = int(counts[i])
            ch, _ = orc.play(n, np.repeat(states[i : i + 1], c, axis=0), moves[i, :c])
            res = orc.result(n, ch)
            mover = int(states[i, -16 + 1])
            mine, theirs = res == (1 if mover == 0 else 3), res == (3 if mover == 0 else 1)
            assert np.array_equal(got["move_values"][i, :c] == 1, mine), (name, i)
            assert np.array_equal(got["move_values"][i, :c] == -1, theirs), (name, i)
            assert (int(got["value"][i]) == 1) == bool(mine.any()), (name, i)
            roads += int(mine.any())
            flats += int(np.isin(res, (2, 4)).any() and not mine.any())
    assert roads >= 2 and flats >= 100  # positions a flat ending is one move away from, and no road: the default mode's +1 / −1


def test_budget_keeps_every_proof_sound(engines):
    states, ref = R.table("five", 4)
    T.require_classes(ref["value"], (3, -4))
    exact = engines[5].solve(states, 4, all_moves=True, road_only=True, node_budget=BUDGET)
    assert not exact["budget_hit"].any()
    assert np.array_equal(exact["value"], ref["value"])  # (the value does not depend on ALL_MOVES)
    tight = engines[5].solve(states, 4, all_moves=True, road_only=True, node_budget=64)
    assert tight["budget_hit"].sum() >= 1
    assert np.array_equal(tight["counts"], exact["counts"]) and np.array_equal(tight["moves"], exact["moves"])
    nz = tight["move_values"] != 0
    assert (np.sign(tight["move_values"][nz]) == np.sign(exact["move_values"][nz])).all()
    assert (np.abs(tight["move_values"][nz]) >= np.abs(exact["move_values"][nz])).all()
    vz = tight["value"] != 0
    assert (np.sign(tight["value"][vz]) == np.sign(exact["value"][vz])).all() and (np.abs(tight["value"][vz]) >= np.abs(exact["value"][vz])).all()
    clean = tight["budget_hit"] == 0
    assert np.array_equal(tight["move_values"][clean], exact["move_values"][clean])


def test_search_solve_with_the_flag_matches_solve_and_leaves_the_trees_alone(engines):
    import tak_amd

    ref = R.reference("m5_400", 3, True)
    rows = [int(np.nonzero(ref["value"] == v)[0][0]) for v in (3, -2, 1, 0)] + [int(np.nonzero(ref["value"] == 3)[0][1])]
    roots = R.positions("m5_400")[rows]
    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_FC5)
    try:
        e.search_create(5, arena_nodes=1 << 14, seed=5)
        e.search_reset(roots)
        e.search_run(30)
        before = [e.search_dump(g) for g in range(5)]
        active = np.array([1, 1, 0, 1, 1], np.uint8)
        got = e.search_solve(3, active=active, all_moves=True, road_only=True, node_budget=BUDGET)
        want = e.solve(e.search_states(), 3, all_moves=True, road_only=True, node_budget=BUDGET)
        for f in T.FIELDS + ("budget_hit", "nodes"):
            assert np.array_equal(got[f][active == 1], want[f][active == 1]), f
            assert not got[f][active == 0].any(), f
        assert T.compare(_rows(ref, rows), want) == []
        assert [int(v) for v in got["value"]] == [3, -2, 0, 0, 3]
        after = [e.search_dump(g) for g in range(5)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    finally:
        e.close()


@pytest.mark.parametrize("count", [1, 5, 257])
def test_results_do_not_depend_on_the_batch(engines, count):
    ref = R.reference("m5_400", 3, True)
    T.require_classes(ref["value"][:257], (1, -2, 3))
    first = {1: int(np.nonzero(ref["value"] == 3)[0][0]), 5: int(np.nonzero(ref["value"] == -2)[0][0]), 257: 0}[count]
    rows = slice(first, first + count)
    got = engines[5].solve(R.positions("m5_400")[rows], 3, all_moves=True, road_only=True, node_budget=BUDGET)
    assert T.compare(_rows(ref, rows), got) == []


def test_the_modes_alternate_on_one_engine(engines):
    """road-only, default, road-only, default on the same engine and positions: each call gives its own mode's reference"""
    road, plain = R.reference("p5_400", 3, False), R.reference("p5_400", 3, False, None, False)
    rows = slice(0, 200)
    assert int((road["value"][rows] != plain["value"][rows]).sum()) >= 50
    states = R.positions("p5_400")[rows]
    for road_only in (True, False, True, False):
        got = engines[5].solve(states, 3, road_only=road_only, node_budget=BUDGET)
        assert T.compare(_rows(road if road_only else plain, rows), got) == [], road_only


@pytest.mark.parametrize("block,depth", [("five", 5), ("six", 4)])
def test_forced_line_plays_the_proof_to_its_road(engines, orc, block, depth):
    """every committed case with |value| >= 3: the line, replayed on the oracle's rules alone, is legal, |value| moves long and ends
    in a road of the side with the proof; and it is the line the same walk gives on tinue_ref"""
    from tak_amd.analysis import forced_line

    n = R.BOARD[R.cases()[block]["set"]]
    states, ref = R.table(block, depth)
    deep = np.nonzero(np.abs(ref["value"]) >= 3)[0]
    T.require_classes(ref["value"][deep], (3, -4) + ((5,) if depth == 5 else ()))
    for j in deep:
        value = int(ref["value"][j])
        line = forced_line(engines[n], states[j], depth, road_only=True, node_budget=BUDGET)
        assert len(line) == abs(value), (block, j)
        cur = states[j : j + 1]
        mover = int(cur[0, -16 + 1])
        for m in line:
            assert int(orc.result(n, cur)[0]) == 0
            moves, counts = orc.movegen(n, cur)
            assert m in moves[0, : counts[0]], (block, j, m)
            cur, status = orc.play(n, cur, [m])
            assert not status.any()
        winner = mover if value > 0 else mover ^ 1
        assert int(orc.result(n, cur)[0]) == (1 if winner == 0 else 3), (block, j)
        assert line == forced_line(R.RefSolver(n), states[j], abs(value), road_only=True), (block, j)
    assert forced_line(engines[n], states[int(np.nonzero(ref["value"] == 0)[0][0])], 3, road_only=True, node_budget=BUDGET) == []


# 5×5, a1 alone empty: white (to move) fills the board and wins on flats with any stone on a1, the first moves of the list, and
# completes row 5 with a4+ (the white flat a4 onto the black flat a5), a later one
_W = "d5 c5 b5 a4 e2 c2 a2 d1 b1 Se3 Sd3".split()
_B = "d4 c4 b4 a5 d2 b2 e1 c1 Sc3 Sb3 Sa3".split()
ROAD_OR_FLATS = ["e4", "e5"] + [m for pair in zip(_W, _B) for m in pair]


def test_player_takes_the_road_over_the_flat_win(engines, orc):
    import tak_amd

    state = orc.from_ptn(5, ROAD_OR_FLATS)
    road, plain = R.TinueRef(5).solve(state[None], 3, False), T.Ref(5).solve(state[None], 3, False)
    assert int(road["value"][0]) == 1 and int(plain["value"][0]) == 1 and int(road["best"][0]) != int(plain["best"][0])
    after = lambda m: int(orc.result(5, orc.play(5, state[None], [m])[0])[0])  # noqa: E731
    assert after(int(road["best"][0])) == 1 and after(int(plain["best"][0])) == 2  # WhiteRoad, WhiteFlat
    assert orc.format_move(5, int(road["best"][0])) == "a4+" and orc.format_move(5, int(plain["best"][0])) == "a1"
    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_FC5)
    try:
        for road_only, want in ((True, road), (False, plain)):
            p = tak_amd.Player(e, 1, False, state, arena_nodes=1 << 14, tactics_road_only=road_only)
            for _ in range(int(road["counts"][0])):
                p.rollout()
            assert p.pick_move(True, tactics=3) == int(want["best"][0]), road_only
            assert int(p.last_tactics["value"][0]) == 1
    finally:
        e.close()


def test_the_flag_bits(engines):
    import ctypes as C

    from tak_amd.engine import TG_SOLVE_ALL_MOVES, TG_SOLVE_ROAD_ONLY, TgSolveConfig, _p

    assert (TG_SOLVE_ALL_MOVES, TG_SOLVE_ROAD_ONLY) == (1, 4)
    e = engines[5]
    states = np.ascontiguousarray(R.positions("m5_400")[:2])
    for flags, ok in ((2, False), (8, False), (6, False), (4, True), (5, True)):
        rc = e.lib.tg_solve(e.h, 2, _p(states), C.byref(TgSolveConfig(3, flags, 0)), None, None, None, None, None, None, None)
        assert (rc == 0) == ok and (ok or (rc == -1 and "flags" in e.lib.tg_last_error().decode())), flags
    ref = R.reference("m5_400", 3, True)
    assert T.compare(_rows(ref, slice(0, 2)), e.solve(states, 3, flags=5, node_budget=BUDGET)) == []
