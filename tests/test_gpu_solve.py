"""GPU gate of the forced-win solver (tg_solve / tg_search_solve) against tests/tactics_ref.py, the plain statement of the
definitions in include/takgpu.h.  Integer work: every comparison is exact.  Each test first asserts, by the reference alone,
that its set holds at least 2 positions of every class it claims to cover."""
import json
import os

import numpy as np
import pytest

import tactics_ref as T

pytestmark = pytest.mark.gpu

BUDGET = 1 << 22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_cases.json")


@pytest.fixture(scope="module")
def engines():
    import tak_amd

    es = {n: tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=64,
                            policy_head=tak_amd.HEAD_FC5 if n == 5 else tak_amd.HEAD_CONV) for n in (5, 6)}
    yield es
    for e in es.values():
        e.close()


def _check(name, depth, all_moves, engines, classes):
    ref = T.reference(name, depth, all_moves)
    T.require_classes(ref["value"], classes)
    got = engines[T.BOARD[name]].solve(T.positions(name), depth, all_moves=all_moves, node_budget=BUDGET)
    print(f"solve {name} depth {depth} all_moves {all_moves}: values {T.class_counts(got['value'])}, nodes {int(got['nodes'].sum())}")
    assert T.compare(ref, got) == []
    return ref, got


def test_depth3_all_moves_playouts_5x5(engines):
    _check("p5_400", 3, True, engines, (1, -2, 3))


def test_depth3_all_moves_random_positions_5x5(engines):
    ref = T.reference("r5_400", 3, True)
    assert T.class_counts(ref["value"]).get(0, 0) >= 300  # the unproven bulk: every move of every position walked to depth 3
    got = engines[5].solve(T.positions("r5_400"), 3, all_moves=True, node_budget=BUDGET)
    assert T.compare(ref, got) == []


@pytest.mark.parametrize("count", [1, 5, 257])
def test_results_do_not_depend_on_the_batch(engines, count):
    """one call of n = 1 (a lone wave), n = 5 (a partial workgroup of the per-position kernels) and n = 257 (an item count that is
    no multiple of anything): the rows are the rows of the whole set's reference"""
    ref = T.reference("p5_400", 3, True)
    T.require_classes(ref["value"][:257], (1, -2, 3))
    first = {1: int(np.nonzero(ref["value"] == 3)[0][0]), 5: int(np.nonzero(ref["value"] == -2)[0][0]), 257: 0}[count]
    rows = slice(first, first + count)
    got = engines[5].solve(T.positions("p5_400")[rows], 3, all_moves=True, node_budget=BUDGET)
    assert T.compare({f: ref[f][rows] for f in T.FIELDS}, got) == []


def test_6x6_depth3(engines):
    _check("p6_200", 3, True, engines, (1, -2, 3))


def test_6x6_depth4(engines):
    _check("p6_80", 4, False, engines, (1, -2, 3, -4))


def test_tall_stacks_depth3(engines):
    """style 3: stacks to height 8, the long spread lists"""
    _check("s5_200", 3, True, engines, (1, -2))


def _golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    idx = [c["index"] for c in doc["cases"]]
    return doc, idx


@pytest.mark.parametrize("depth", [4, 5])
def test_depths_4_and_5_from_the_committed_cases(engines, depth):
    doc, idx = _golden()
    states = T.positions(doc["set"])[idx]
    k = len(idx)
    ref = dict(value=np.zeros(k, np.int8), best=np.zeros(k, np.uint16), counts=np.zeros(k, np.int32),
               moves=np.zeros((k, T.TG_MAX_MOVES), np.uint16), move_values=np.zeros((k, T.TG_MAX_MOVES), np.int8))
    for j, c in enumerate(doc["cases"]):
        e = c[f"depth{depth}"]
        ref["value"][j], ref["best"][j], ref["counts"][j] = e["value"], e["best"], c["counts"]
        ref["moves"][j, : c["counts"]] = c["moves"]
        ref["move_values"][j, : c["counts"]] = e["move_values"]
    T.require_classes(ref["value"], (1, -2, 3, -4) + ((5,) if depth == 5 else ()))
    got = engines[5].solve(states, depth, all_moves=False, node_budget=BUDGET)
    print(f"solve golden depth {depth}: nodes {int(got['nodes'].sum())}, largest position {int(got['nodes'].max())}")
    assert T.compare(ref, got) == []


def test_early_stop_and_clipping(engines):
    ref = T.reference("p5_400", 3, False)
    T.require_classes(ref["value"], (1, -2, 3))
    full = T.reference("p5_400", 3, True)
    assert T.compare(full, ref, budget_free=False) != []  # the two modes differ on this set, so the test can tell them apart
    got = engines[5].solve(T.positions("p5_400"), 3, all_moves=False, node_budget=BUDGET)
    assert T.compare(ref, got) == []
    # an ALL_MOVES table at depth 5 cut to |d| <= 3 is the ALL_MOVES table at depth 3 (on the first 48 positions: depth 5 on every move)
    deep = engines[5].solve(T.positions("p5_400")[:48], 5, all_moves=True, node_budget=BUDGET)
    assert not deep["budget_hit"].any()
    assert T.compare({f: full[f][:48] for f in T.FIELDS}, T.clip(deep, 3)) == []


def test_finished_positions_give_zero_rows(engines, orc):
    po = orc.playouts(5, 400, 7)
    ref = T.reference("p5_400", 3, True)
    assert (orc.result(5, po["final"][:20]) != 0).all()
    mixed = np.concatenate([po["final"][:3], po["prev"][:7], po["final"][3:5], po["prev"][7:20], po["final"][5:6]])
    live = np.r_[3:10, 12:25]
    got = engines[5].solve(mixed, 3, all_moves=True, node_budget=BUDGET)
    dead = np.setdiff1d(np.arange(len(mixed)), live)
    for f in T.FIELDS + ("budget_hit", "nodes"):
        assert not got[f][dead].any(), f
    assert T.compare({f: ref[f][:20] for f in T.FIELDS}, {f: got[f][live] for f in T.FIELDS + ("budget_hit",)}) == []


def test_budget_keeps_every_proof_sound(engines):
    doc, idx = _golden()
    states = T.positions(doc["set"])[idx]
    exact = engines[5].solve(states, 4, all_moves=True, node_budget=BUDGET)
    assert not exact["budget_hit"].any()
    cases = {c["index"]: c["depth4"]["value"] for c in doc["cases"]}
    assert [int(v) for v in exact["value"]] == [cases[i] for i in idx]  # (the value does not depend on the mode)
    tight = engines[5].solve(states, 4, all_moves=True, node_budget=64)
    assert tight["budget_hit"].sum() >= 1
    assert np.array_equal(tight["counts"], exact["counts"]) and np.array_equal(tight["moves"], exact["moves"])
    nz = tight["move_values"] != 0
    assert (np.sign(tight["move_values"][nz]) == np.sign(exact["move_values"][nz])).all()
    assert (np.abs(tight["move_values"][nz]) >= np.abs(exact["move_values"][nz])).all()
    vz = tight["value"] != 0
    assert (np.sign(tight["value"][vz]) == np.sign(exact["value"][vz])).all() and (np.abs(tight["value"][vz]) >= np.abs(exact["value"][vz])).all()
    clean = tight["budget_hit"] == 0
    assert np.array_equal(tight["move_values"][clean], exact["move_values"][clean])
    assert (tight["nodes"] <= tight["counts"].astype(np.uint64) * 4 * (64 + T.TG_MAX_MOVES)).all()
    assert (exact["nodes"] <= exact["counts"].astype(np.uint64) * 4 * (BUDGET + T.TG_MAX_MOVES)).all()


def test_search_solve_matches_solve_and_leaves_the_trees_alone(engines, orc):
    import tak_amd

    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_FC5)
    try:
        with pytest.raises(tak_amd.TgError) as ei:
            e.search_solve(2)
        assert ei.value.code == -7  # TG_ERR_STATE: no search object
        roots = T.positions("p5_400")[[int(i) for i in np.nonzero(T.reference("p5_400", 3, False)["value"] == 0)[0][:6]]]
        e.search_create(6, arena_nodes=1 << 14, seed=5)
        e.search_reset(roots)
        live = np.ones(6, np.uint8)
        for _ in range(3):  # a few plies; a game that ends on the way stays where it ended
            e.search_run(30, active=live)
            r = e.search_root()
            live = (r["counts"] > 0).astype(np.uint8)
            picks = [int(r["moves"][g, int(np.argmax(r["visits"][g, : r["counts"][g]]))]) if live[g] else 0 for g in range(6)]
            e.search_play(np.array(picks, np.uint16), active=live)
        e.search_run(30, active=live)
        before = [e.search_dump(g) for g in range(6)]
        active = np.array([1, 0, 1, 1, 0, 1], np.uint8)
        got = e.search_solve(3, active=active, all_moves=True, node_budget=BUDGET)
        want = e.solve(e.search_states(), 3, all_moves=True, node_budget=BUDGET)
        for f in T.FIELDS + ("budget_hit", "nodes"):
            assert np.array_equal(got[f][active == 1], want[f][active == 1]), f
            assert not got[f][active == 0].any(), f
        assert (want["counts"][active == 1] > 0).sum() >= 2
        assert T.compare(T.Ref(5).solve(e.search_states(), 3, True), want) == []
        after = [e.search_dump(g) for g in range(6)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    finally:
        e.close()


def test_depth1_is_the_instant_win_rule(engines, orc):
    """a move value is +1 exactly where the position after the move is won for the mover (self_play.rs:118-171 as k_sp_instant_win
    states it), over three sets"""
    for name in ("p5_400", "p6_200", "s5_200"):
        n, states = T.BOARD[name], T.positions(name)
        got = engines[n].solve(states, 1, all_moves=True)
        moves, counts = orc.movegen(n, states)
        assert np.array_equal(got["counts"], counts) and np.array_equal(got["moves"], moves)
        wins = 0
        for i in range(len(states)):
            c = int(counts[i])
            ch, _ = orc.play(n, np.repeat(states[i : i + 1], c, axis=0), moves[i, :c])
            res = orc.result(n, ch)
            mover = int(states[i, -16 + 1])
            won = np.isin(res, (1, 2) if mover == 0 else (3, 4))
            assert np.array_equal(got["move_values"][i, :c] == 1, won), (name, i)
            wins += int(won.any())
            assert (int(got["value"][i]) == 1) == bool(won.any())
        assert wins >= 2


def test_player_takes_the_forced_win(engines):
    import tak_amd

    ref = T.reference("p5_400", 3, False)
    i = int(np.nonzero(ref["value"] == 3)[0][0])
    state = T.positions("p5_400")[i]
    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_FC5)
    try:
        p = tak_amd.Player(e, 1, False, state, arena_nodes=1 << 14)
        for _ in range(int(ref["counts"][i])):  # one rollout per move
            p.rollout()
        calls = []
        real = e.search_solve
        e.search_solve = lambda *a, **k: (calls.append(a), real(*a, **k))[1]
        plain = p.pick_move(True)
        assert calls == [] and p.last_tactics is None  # tactics = 0: no solver launch
        assert plain == p.pick_move(True, tactics=0) and calls == []
        assert p.pick_move(True, tactics=3) == int(ref["best"][i])
        assert len(calls) == 1 and int(p.last_tactics["value"][0]) == 3 and int(p.last_tactics["nodes"][0]) > 0
    finally:
        e.close()


def test_argument_errors_name_the_field(engines):
    import ctypes as C

    import tak_amd
    from tak_amd.engine import TgSolveConfig, _p

    e = engines[5]
    states = np.ascontiguousarray(T.positions("p5_400")[:2])

    def call(cfg, st=states, n=2):
        rc = e.lib.tg_solve(e.h, n, _p(st), C.byref(cfg) if cfg is not None else None, None, None, None, None, None, None, None)
        return rc, e.lib.tg_last_error().decode()

    for cfg, word in ((TgSolveConfig(0, 0, 0), "depth"), (TgSolveConfig(7, 0, 0), "depth"), (TgSolveConfig(3, 2, 0), "flags"),
                      (TgSolveConfig(3, 0, 0, (C.c_int32 * 4)(0, 0, 1, 0)), "reserved")):
        rc, msg = call(cfg)
        assert rc == -1 and word in msg, (rc, msg)
    rc, msg = call(TgSolveConfig(3, 0, 0), st=None)
    assert rc == -1 and "states" in msg
    rc, msg = call(None)
    assert rc == -1 and "cfg" in msg
    assert call(TgSolveConfig(3, 0, 0))[0] == 0  # every output pointer may be NULL
    with pytest.raises(tak_amd.TgError):
        e.solve(states, 7)
