"""GPU gate of the forced-win solver (tg_solve / tg_search_solve) against tests/tactics_ref.py, the plain statement of the
definitions in include/takgpu.h.  Integer work: every comparison is exact.  Each test first asserts, by the reference alone,
that its set holds at least 2 positions of every class it claims to cover — or, for the tests of more than one chunk, of the
reversible-plies draw and of the budget, the condition that lets the test tell the right answer from the likely wrong one."""
import functools
import json
import os

import numpy as np
import pytest

import posgen
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


def _table(block, depth):
    """→ (rows of the block's position set, the committed early-stop table) of the block's cases that carry `depth`"""
    cases = [c for c in block["cases"] if f"depth{depth}" in c]
    k = len(cases)
    ref = dict(value=np.zeros(k, np.int8), best=np.zeros(k, np.uint16), counts=np.zeros(k, np.int32),
               moves=np.zeros((k, T.TG_MAX_MOVES), np.uint16), move_values=np.zeros((k, T.TG_MAX_MOVES), np.int8))
    for j, c in enumerate(cases):
        e = c[f"depth{depth}"]
        ref["value"][j], ref["best"][j], ref["counts"][j] = e["value"], e["best"], c["counts"]
        ref["moves"][j, : c["counts"]] = c["moves"]
        ref["move_values"][j, : c["counts"]] = e["move_values"]
    return T.positions(block["set"])[[c["index"] for c in cases]], ref


def _cat(tables):
    return {f: np.concatenate([t[f] for t in tables]) for f in tables[0]}


def _five(depth):
    """the 5×5 cases that carry `depth`: the play-out block, then the tall-stack block"""
    doc, _ = _golden()
    (s0, r0), (s1, r1) = _table(doc, depth), _table(doc["tall_stacks"], depth)
    return np.concatenate([s0, s1]), _cat([r0, r1])


def _six(depth):
    doc, _ = _golden()
    return _table(doc["six"], depth)


def _report(what, got):
    print(f"{what}: values {T.class_counts(got['value'])}, nodes {int(got['nodes'].sum())}, largest position {int(got['nodes'].max())}, "
          f"budget_hit rows {int(np.count_nonzero(got['budget_hit']))} of {len(got['value'])}")


@pytest.mark.parametrize("depth", [4, 5])
def test_depths_4_and_5_from_the_committed_cases(engines, depth):
    doc, idx = _golden()
    states, ref = _table(doc, depth)
    assert len(states) == len(idx)
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


# ---- depth 6, 6×6 to depth 5, from the committed cases (tests/golden/make_solve_cases.py) -----------------------------------


def test_depth6_on_the_5x5_cases(engines):
    """k_solve_level<6>: the deepest instantiation, and the only one that can give −6"""
    states, ref = _five(6)
    T.require_classes(ref["value"], (1, -2, 3, -4, 5, -6))
    assert (ref["value"] == -6).sum() >= 3 and (ref["value"] == 0).sum() >= 4
    got = engines[5].solve(states, 6, all_moves=False, node_budget=BUDGET)
    _report("solve golden 5x5 depth 6", got)
    assert not got["budget_hit"].any()
    assert T.compare(ref, got) == []


@pytest.mark.parametrize("depth", [5, 6])
def test_6x6_depths_5_and_6_from_the_committed_cases(engines, depth):
    states, ref = _six(depth)
    if depth == 5:
        T.require_classes(ref["value"], (1, -2, 3, -4, 5))
    else:  # the deep ones again (the same table under the early stop) and the lightest positions that depth 5 leaves open
        T.require_classes(ref["value"], (3, -4, 5))
        assert (ref["value"] == 0).sum() + (ref["value"] == -6).sum() >= 4
    got = engines[6].solve(states, depth, all_moves=False, node_budget=BUDGET)
    _report(f"solve golden 6x6 depth {depth}", got)
    assert T.compare(ref, got) == []


@functools.lru_cache(maxsize=None)
def _clip_cases():
    """the ALL_MOVES tables at depth 5 and 3 of: the −6 positions of the tall-stack block and two more of its positions (open at
    depth 5, so their committed depth-5 tables, made with the early stop, are the ALL_MOVES ones), and the first two +3 positions of the
    play-out block (ALL_MOVES at depth 5 by the reference, here)"""
    doc, _ = _golden()
    tall = doc["tall_stacks"]
    minus6 = [j for j, c in enumerate(tall["cases"]) if c["depth6"]["value"] == -6]
    rows = minus6 + [j for j in range(len(tall["cases"])) if j not in minus6][:2]
    st, r5 = _table(tall, 5)
    assert not r5["value"].any()
    idx = [tall["cases"][j]["index"] for j in rows]
    full3 = T.reference("s5_200", 3, True)
    three = [c["index"] for c in doc["cases"] if c["depth5"]["value"] == 3][:2]
    p = T.positions("p5_160")[three]
    states = np.concatenate([st[rows], p])
    ref = T.Ref(5)
    want5 = _cat([{f: r5[f][rows] for f in T.FIELDS}, {f: v for f, v in ref.solve(p, 5, True).items() if f in T.FIELDS}])
    want3 = _cat([{f: full3[f][idx] for f in T.FIELDS}, {f: v for f, v in ref.solve(p, 3, True).items() if f in T.FIELDS}])
    return states, want5, want3, len(minus6)


def test_all_moves_at_depth6_clipped_to_5_and_3(engines):
    states, want5, want3, minus6 = _clip_cases()
    assert minus6 >= 2 and len(states) <= minus6 + 4
    assert (want5["value"] == 3).sum() >= 2 and T.compare(want5, want3, budget_free=False) != []  # the two cuts differ
    assert (np.abs(want5["move_values"][want5["value"] == 3]) > 3).any()  # moves valued past the level that decides: the early stop would not have them
    deep = engines[5].solve(states, 6, all_moves=True, node_budget=BUDGET)
    _report("solve ALL_MOVES depth 6", deep)
    assert not deep["budget_hit"].any()
    assert (deep["value"][:minus6] == -6).all()
    assert T.compare(want5, T.clip(deep, 5)) == []
    assert T.compare(want3, T.clip(deep, 3)) == []


# ---- more than one chunk of positions (SOLVE_CHUNK = 4096 in csrc/solve.hip) ---------------------------------------------------
CHUNK = 4096


def _rows(n):
    return (7 * np.arange(n) + 3) % 400


def test_a_second_chunk_of_133_positions(engines):
    """n = 4096 + 133 at depth 3: the second chunk's rows land at row 4096 of all seven outputs, on scratch re-bound to 133 rows"""
    n = CHUNK + 133
    rows = _rows(n)
    full = T.reference("p5_400", 3, True)
    want = {f: full[f][rows] for f in T.FIELDS}
    tail, head = {f: want[f][CHUNK:] for f in T.FIELDS}, {f: want[f][:133] for f in T.FIELDS}
    assert T.compare(head, tail, budget_free=False) != []  # written at row 0 the second chunk would not pass
    assert T.compare({f: want[f][CHUNK - 1: n - 1] for f in T.FIELDS}, tail, budget_free=False) != []  # nor one row off
    cc = T.class_counts(tail["value"])
    assert all(cc.get(c, 0) >= 2 for c in (1, -2, 3)), cc
    got = engines[5].solve(T.positions("p5_400")[rows], 3, all_moves=True, node_budget=BUDGET)
    _report(f"solve {n} positions depth 3", got)
    assert T.compare(want, got) == []
    first = got["nodes"][:400]
    assert first[full["counts"][rows[:400]] > 0].all()
    assert np.array_equal(got["nodes"], first[np.arange(n) % 400])  # the same position costs the same in any chunk


@pytest.mark.parametrize("n", [CHUNK, CHUNK + 1])
def test_one_full_chunk_and_a_last_chunk_of_one(engines, orc, n):
    """depth 1: a move value is +1 exactly where the position after the move is won for the mover (the instant-win rule, stated
    through the oracle), −1 where it is won for the other side"""
    rows = _rows(n)
    base = T.positions("p5_400")
    moves, counts = orc.movegen(5, base)
    vals = np.zeros((400, T.TG_MAX_MOVES), np.int8)
    for i in range(400):
        c = int(counts[i])
        ch, _ = orc.play(5, np.repeat(base[i: i + 1], c, axis=0), moves[i, :c])
        res, mover = orc.result(5, ch), int(base[i, -16 + 1])
        vals[i, :c] = np.where(np.isin(res, (1, 2) if mover == 0 else (3, 4)), 1, np.where(np.isin(res, (3, 4) if mover == 0 else (1, 2)), -1, 0))
    assert (vals == 1).any(axis=1).sum() >= 2 and (vals == -1).any(axis=1).sum() >= 2 and counts[rows[-1]] > 0  # (the last row is no zero row)
    got = engines[5].solve(base[rows], 1, all_moves=True)
    assert np.array_equal(got["counts"], counts[rows]) and np.array_equal(got["moves"], moves[rows])
    assert np.array_equal(got["move_values"], vals[rows])
    assert np.array_equal(got["value"] == 1, (vals[rows] == 1).any(axis=1)) and not got["budget_hit"].any()
    assert T.compare({f: T.reference("p5_400", 1, True)[f][rows] for f in T.FIELDS}, got) == []


def test_search_solve_on_more_games_than_a_chunk(orc):
    """4096 + 5 roots of a caller-driven search, set by search_reset alone: finished positions and inactive games on both sides of
    row 4096"""
    import tak_amd

    G = CHUNK + 5
    rows = _rows(G)
    full = T.reference("p5_400", 3, True)
    roots = T.positions("p5_400")[rows].copy()
    finals = orc.playouts(5, 400, 7)["final"]
    finished = np.array([5, CHUNK - 6, CHUNK - 1, CHUNK])
    assert (orc.result(5, finals[:4]) != 0).all()
    roots[finished] = finals[:4]
    active = np.ones(G, np.uint8)
    active[[7, CHUNK - 6, CHUNK - 2, CHUNK + 3]] = 0
    live = np.ones(G, bool)
    live[finished] = False
    on = live & (active == 1)
    assert on[:CHUNK].sum() >= 2 and on[CHUNK:].sum() >= 2 and (~on[:CHUNK]).sum() >= 2 and (~on[CHUNK:]).sum() >= 2
    assert (full["counts"][rows[CHUNK:][on[CHUNK:]]] > 0).all()
    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=G, policy_head=tak_amd.HEAD_FC5)
    try:
        e.search_create(G, arena_nodes=1024, seed=5)  # (1024: the smallest arena search_create takes)
        e.search_reset(roots)
        sample = [0, 7, CHUNK - 2, CHUNK + 1, CHUNK + 3, CHUNK + 4]
        before = [e.search_dump(g, capacity=1 << 12) for g in sample]
        got = e.search_solve(3, active=active, all_moves=True, node_budget=BUDGET)
        _report(f"search_solve {G} games depth 3", got)
        assert T.compare({f: full[f][rows[on]] for f in T.FIELDS}, {f: got[f][on] for f in T.FIELDS + ("budget_hit",)}) == []
        assert (got["nodes"][on] > 0).all()
        for f in T.FIELDS + ("budget_hit", "nodes"):
            assert not got[f][~on].any(), f
        after = [e.search_dump(g, capacity=1 << 12) for g in sample]
        assert all(len(a) >= 1 and a.tobytes() == b.tobytes() for a, b in zip(before, after))
    finally:
        e.close()


# ---- the 50-reversible-plies draw inside the tree --------------------------------------------------------------------------


def _draws_at_the_horizon(name, orc):
    """positions 50 − r plies below the roots whose result is TG_DRAW_REVERSIBLE.  A spread adds one to the counter and a placement
    clears it, so the draw stands at that ply and no sooner: after a root move for r = 49 (ITEM_DRAWN), after a reply for r = 48
    (the draw that refutes an X test), one ply further for r = 47 (the draw that ends a line of a W test).  Walked over at most 200
    ongoing positions per ply."""
    base, _, r = T.REVERSIBLE[name]
    n, front = T.BOARD[name], T.positions(name)
    for step in range(50 - r):
        front = front[orc.result(n, front) == 0]
        front = front[posgen.header(front, "reversible_plies") == r + step][:200]  # (only a line of spreads gets there)
        moves, counts = orc.movegen(n, front)
        idx = np.repeat(np.arange(len(front)), counts)
        col = np.arange(len(idx)) - np.repeat(np.cumsum(counts) - counts, counts)
        front, status = orc.play(n, front[idx], moves[idx, col])
        assert not status.any()
    return int((orc.result(n, front) == T.TG_DRAW_REVERSIBLE).sum())


# the sets on which the draw changes the VALUE of at least 2 positions; on the others it changes move values only
VALUE_MOVES = ("p5_400_r49", "p5_400_r48", "s5_200_r49", "p6_200_r49", "p6_200_r48")


def _check_reversible(name, depth, all_moves, engines, orc):
    base, k, r = T.REVERSIBLE[name]
    ref, plain = T.reference(name, depth, all_moves), T.reference(base, depth, all_moves)
    assert np.array_equal(ref["moves"], plain["moves"][:k])  # the counter changes no move list
    changed = int((ref["move_values"] != plain["move_values"][:k]).any(axis=1).sum())
    values = int((ref["value"] != plain["value"][:k]).sum())
    draws = _draws_at_the_horizon(name, orc)
    print(f"solve {name} depth {depth} all_moves {all_moves}: values {T.class_counts(ref['value'])}, rows whose table moves {changed}, "
          f"whose value moves {values}, draws {50 - r} plies down {draws}")
    assert changed >= 2 and draws >= 2
    if name in VALUE_MOVES:
        assert values >= 2
    got = engines[T.BOARD[name]].solve(T.positions(name), depth, all_moves=all_moves, node_budget=BUDGET)
    _report(f"solve {name}", got)
    assert T.compare(ref, got) == []


@pytest.mark.parametrize("name", sorted(n for n in T.REVERSIBLE if not n.endswith("r47")))
def test_the_reversible_draw_one_and_two_plies_down(engines, orc, name):
    _check_reversible(name, 3, True, engines, orc)


def test_the_reversible_draw_three_plies_down(engines, orc):
    _check_reversible("s5_200_r47", 4, True, engines, orc)


def test_the_reversible_draw_under_the_early_stop(engines, orc):
    _check_reversible("p6_200_r49", 3, False, engines, orc)


# ---- the budget where it is used ------------------------------------------------------------------------------------------


def _sound(tight, exact, budget, depth, all_moves):
    """what include/takgpu.h promises of a run that met its budget, against the exact run: the same lists; no proof that the exact run
    does not have — a non-zero value has the exact sign and a distance not below the exact one; rows that did not meet the budget
    equal; `nodes` bounded.  Under the early stop the exact table ends at the level that decided the position, and a run that gave
    that level up goes on: a move it values where the exact table has 0 must then lie beyond that level (with ALL_MOVES, and for a
    position the exact run leaves open, no such move can exist)."""
    assert np.array_equal(tight["counts"], exact["counts"]) and np.array_equal(tight["moves"], exact["moves"])
    stop = np.abs(exact["value"]).astype(np.int64)  # the last level the exact run completed for the position
    stop[(stop == 0) | bool(all_moves)] = depth
    t, x = tight["move_values"].astype(np.int64), exact["move_values"].astype(np.int64)
    both, only = (t != 0) & (x != 0), (t != 0) & (x == 0)
    assert (np.sign(t[both]) == np.sign(x[both])).all() and (np.abs(t[both]) >= np.abs(x[both])).all()
    assert (np.abs(t) > stop[:, None])[only].all() and (np.abs(t) <= depth).all()
    nz = tight["value"] != 0
    assert (np.sign(tight["value"][nz]) == np.sign(exact["value"][nz])).all()
    assert (np.abs(tight["value"][nz].astype(np.int64)) >= np.abs(exact["value"][nz].astype(np.int64))).all()
    clean = tight["budget_hit"] == 0
    for f in T.FIELDS:
        assert np.array_equal(tight[f][clean], exact[f][clean]), f
    assert (tight["nodes"] <= tight["counts"].astype(np.uint64) * depth * (budget + T.TG_MAX_MOVES)).all()


@pytest.mark.parametrize("all_moves", [False, True])
@pytest.mark.parametrize("board", [5, 6])
def test_the_default_budget_at_depth5(engines, board, all_moves):
    """node_budget = 0 is 2^10 positions per (position, root move, level): most positions that depth 5 leaves open meet it"""
    states, committed = _five(5) if board == 5 else _six(5)
    if all_moves:
        exact = engines[board].solve(states, 5, all_moves=True, node_budget=BUDGET)
        assert not exact["budget_hit"].any() and np.array_equal(exact["value"], committed["value"])  # (the value does not depend on the mode)
    else:
        exact = committed
    got = engines[board].solve(states, 5, all_moves=all_moves, node_budget=0)
    _report(f"solve {board}x{board} depth 5 all_moves {all_moves} default budget", got)
    _sound(got, exact, 1 << 10, 5, all_moves)
    assert got["budget_hit"].sum() >= 1
    assert ((exact["value"] != 0) & (got["budget_hit"] == 0)).sum() >= 2
    named = engines[board].solve(states, 5, all_moves=all_moves, node_budget=1 << 10)
    for f in T.FIELDS + ("budget_hit", "nodes"):
        assert np.array_equal(named[f], got[f]), f  # 0 is TG_SOLVE_DEFAULT_BUDGET


@pytest.mark.parametrize("budget", [64, 4096])
def test_tight_budgets_at_depth6(engines, budget):
    states, exact = _five(6)
    got = engines[5].solve(states, 6, all_moves=False, node_budget=budget)
    _report(f"solve 5x5 depth 6 budget {budget}", got)
    _sound(got, exact, budget, 6, False)
    assert got["budget_hit"].sum() >= 1


def test_the_budget_clamp_and_a_budget_of_one(engines, orc):
    doc, _ = _golden()
    states, exact = _table(doc, 4)
    for budget in (1 << 40, (1 << 31) - 1):  # above 2^31 − 1 the budget is 2^31 − 1
        assert T.compare(exact, engines[5].solve(states, 4, all_moves=False, node_budget=budget)) == []
    # one position per item and level: the replayed root move is all an item may create, so no level above 1 proves anything
    one = engines[5].solve(states, 4, all_moves=False, node_budget=1)
    _sound(one, exact, 1, 4, False)
    first = T.Ref(5).solve(states, 1, False)
    assert T.compare(first, one, budget_free=False) == []
    deeper = np.zeros(len(states), bool)  # level 2 had an item to run: the position is open after level 1 and a root move leaves it ongoing
    for i in range(len(states)):
        c = int(first["counts"][i])
        ch, _ = orc.play(5, np.repeat(states[i: i + 1], c, axis=0), first["moves"][i, :c])
        deeper[i] = first["value"][i] == 0 and ((orc.result(5, ch) == 0) & (first["move_values"][i, :c] == 0)).any()
    assert deeper.sum() >= 2 and (~deeper).sum() >= 2
    assert np.array_equal(one["budget_hit"] != 0, deeper)  # set wherever a level above 1 ran


# ---- tg_search_solve on the other objects -----------------------------------------------------------------------------------


def test_search_solve_on_a_6x6_search(engines):
    import tak_amd

    G = 6
    e = tak_amd.Engine(6, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    try:
        roots = T.positions("p6_200")[[int(i) for i in np.nonzero(T.reference("p6_200", 3, True)["value"] == 0)[0][:G]]]
        e.search_create(G, arena_nodes=1 << 14, seed=5)
        e.search_reset(roots)
        live = np.ones(G, np.uint8)
        for _ in range(3):
            e.search_run(30, active=live)
            r = e.search_root()
            live = (r["counts"] > 0).astype(np.uint8)
            picks = [int(r["moves"][g, int(np.argmax(r["visits"][g, : r["counts"][g]]))]) if live[g] else 0 for g in range(G)]
            e.search_play(np.array(picks, np.uint16), active=live)
        e.search_run(30, active=live)
        before = [e.search_dump(g) for g in range(G)]
        got = e.search_solve(3, all_moves=True, node_budget=BUDGET)
        want = e.solve(e.search_states(), 3, all_moves=True, node_budget=BUDGET)
        for f in T.FIELDS + ("budget_hit", "nodes"):
            assert np.array_equal(got[f], want[f]), f
        assert (want["counts"] > 0).sum() >= 2
        assert T.compare(T.Ref(6).solve(e.search_states(), 3, True), got) == []
        after = [e.search_dump(g) for g in range(G)]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    finally:
        e.close()


def test_search_solve_on_a_selfplay_object():
    """the roots of the self-play driver's games, and the driver goes on as if nothing had been asked: stats, roots and drained
    examples of a run with a search_solve in the middle are those of a run without one (same seed, two engines)"""
    import tak_amd

    games = 6
    kw = dict(rollouts=16, noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=9)
    runs = []
    for ask in (True, False):
        e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64)
        try:
            e.selfplay_create(games, arena_nodes=1 << 15, seed=5, max_examples=1 << 13, **kw)
            e.selfplay_step(14)
            if ask:
                roots = e.search_states()
                assert (T.oracle.result(5, roots) == 0).sum() >= 2 and (posgen.header(roots, "ply") >= 2).sum() >= 2
                got = e.search_solve(3, all_moves=True, node_budget=BUDGET)
                want = e.solve(roots, 3, all_moves=True, node_budget=BUDGET)
                for f in T.FIELDS + ("budget_hit", "nodes"):
                    assert np.array_equal(got[f], want[f]), f
                assert T.compare(T.Ref(5).solve(roots, 3, True), got) == []
                assert np.array_equal(e.search_states(), roots)
            e.selfplay_step(46)
            runs.append((e.selfplay_stats(), e.selfplay_drain(1 << 13), e.search_states()))
        finally:
            e.close()
    (sa, da, ra), (sb, db, rb) = runs
    assert sa == sb and sa["examples"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(da, db)) and np.array_equal(ra, rb)
