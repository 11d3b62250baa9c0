"""GPU gate of the move-list capacity TG_MAX_MOVES = 512 at the entry points that take positions from callers, on the positions
of posgen.long_list_states (6×6; up to 1076 legal moves), against the oracle (whose lists have no capacity: oracle.movegen_full)
and tests/tactics_ref.py with the give-up rule of include/takgpu.h.  What the positions are is asserted by the oracle alone in
tests/test_long_move_lists.py; the facts a test here relies on are asserted again before the GPU is asked."""
import functools

import numpy as np
import pytest

import posgen
import tactics_ref as T
import tinue_ref as R

pytestmark = pytest.mark.gpu

N = 6
BUDGET = 1 << 22  # never met here: only a cut list gives up


@functools.lru_cache(maxsize=None)
def family():
    from oracle import oracle

    return posgen.long_list_states(oracle, N)


def _roots():
    return np.stack([r for r, _, _ in family()["roots"].values()])


def _row(name):
    return list(family()["roots"]).index(name)


@pytest.fixture(scope="module")
def engine():
    import tak_amd

    e = tak_amd.Engine(N, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    yield e
    e.close()


def test_board_operators_on_the_family(engine, orc):
    import tak_amd

    fam = family()
    sts = np.stack(list(fam["states"].values()) + [r for r, _, _ in fam["roots"].values()])
    assert np.array_equal(engine.result(sts), orc.result(N, sts))
    assert np.array_equal(engine.encode(sts), orc.encode(N, sts))
    for st in sts:
        assert tak_amd.format_tps(N, st) == orc.to_tps(N, st)
        back = tak_amd.parse_tps(N, orc.to_tps(N, st))
        assert np.array_equal(back[: -16], st[: -16])
        assert np.array_equal(back[-16: -8], st[-16: -8])  # what TPS determines of the header: size, side to move, ply, the four reserves
    for name in ("max", "S", "e513"):  # every move of the uncut list, the ones behind index 512 included
        moves, counts = orc.movegen_full(N, fam["states"][name])
        c = int(counts[0])
        assert c > 512
        parents = np.repeat(fam["states"][name][None], c, axis=0)
        want, wst = orc.play(N, parents, moves[0, :c])
        got, gst = engine.play(parents, moves[0, :c])
        assert not wst.any() and np.array_equal(gst, wst) and np.array_equal(got, want), name
        assert np.array_equal(engine.result(got), orc.result(N, want))


def _same_lists(a, b, counts):
    """the rows agree on their lists (tg_movegen leaves the rest of a row as it was)"""
    return all(np.array_equal(a[i, :c], b[i, :c]) for i, c in enumerate(counts))


def test_movegen_at_the_edge(engine, orc):
    import tak_amd

    fam = family()
    ordinary = orc.random_positions(N, 20, seed=9, max_plies=60)
    for name in ("e512", "e512_bare"):  # exactly TG_MAX_MOVES: the whole list, TG_OK
        batch = np.concatenate([ordinary[:7], fam["states"][name][None], ordinary[7:]])
        moves, counts = engine.movegen(batch)
        om, oc = orc.movegen(N, batch)
        assert counts[7] == 512 and np.array_equal(counts, oc) and _same_lists(moves, om, oc)
    batch = np.concatenate([ordinary[:7], fam["states"]["e513"][None], ordinary[7:]])
    with pytest.raises(tak_amd.TgError) as err:  # one more: refused
        engine.movegen(batch)
    assert err.value.code == -1 and "TG_MAX_MOVES" in str(err.value)
    moves, counts = engine.movegen(ordinary)  # and the engine goes on
    om, oc = orc.movegen(N, ordinary)
    assert np.array_equal(counts, oc) and _same_lists(moves, om, oc)


def test_perft(engine, orc):
    import tak_amd

    fam = family()
    sts = np.stack([fam["states"][k] for k in ("S", "max", "e512", "e513")])
    assert list(engine.perft(sts, 1)) == [763, 1076, 512, 513]  # depth 1 is only counted: the true count
    ordinary = orc.random_positions(N, 3, seed=4, max_plies=30)
    root, move, _ = fam["roots"]["R"]
    with pytest.raises(tak_amd.TgError) as err:  # depth 2 would expand S: refused on the host, naming the root
        engine.perft(np.concatenate([ordinary[:1], root[None]]), 3)
    assert err.value.code == -1 and "root 1" in str(err.value) and "TG_MAX_MOVES" in str(err.value)
    with pytest.raises(tak_amd.TgError) as err:
        engine.perft(fam["states"]["S"][None], 2)
    assert err.value.code == -1 and "root 0" in str(err.value)
    # a frontier of exactly 512 moves is expanded whole
    assert int(engine.perft(fam["states"]["e512"][None], 2)[0]) == orc.perft(N, fam["states"]["e512"], 2)
    assert int(engine.perft(root[None], 2)[0]) == orc.perft(N, root, 2)  # (S is on the last level: counted, not expanded)
    assert [int(x) for x in engine.perft(ordinary, 2)] == [orc.perft(N, s, 2) for s in ordinary]


@functools.lru_cache(maxsize=None)
def _reference(road, depth, capacity):
    out = (R.TinueRef if road else T.Ref)(N, capacity=capacity).solve(_roots(), depth, False)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize("road", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_solver_gives_up_on_a_cut_list(engine, road, depth):
    """row for row the reference with the give-up rule; sound against the reference on whole lists; the move into S unproven and
    reported; a win among the first 512 moves of a cut list kept.  (At depth 3 the first 512 moves of S all lose at once: a solver
    that takes them for the whole list answers +3 — tests/test_long_move_lists.py plants that.)"""
    rule, exact = _reference(road, depth, 512), _reference(road, depth, None)
    got = engine.solve(_roots(), depth, node_budget=BUDGET, road_only=road)
    print(f"road {road} depth {depth}: value {got['value']} budget_hit {got['budget_hit']} nodes {got['nodes']}")
    assert T.compare_with_give_up(rule, got) == []
    assert T.sound(exact, got, depth) == []
    for name in ("R", "R_swapped", "R_mirror"):
        i = _row(name)
        j = list(got["moves"][i]).index(family()["roots"][name][1])
        assert got["move_values"][i, j] == 0 and got["budget_hit"][i] == 1
    assert got["value"][_row("R_W")] == -2 == exact["value"][_row("R_W")]


def test_solver_searches_a_list_of_exactly_512_completely(engine):
    st = family()["states"]["e512"][None]
    rule, exact = T.Ref(N).solve(st, 2, True), T.Ref(N, capacity=None).solve(st, 2, True)
    assert rule["counts"][0] == 512 and not rule["budget_hit"].any() and T.compare(exact, rule) == []
    got = engine.solve(st, 2, all_moves=True, node_budget=BUDGET)
    assert T.compare(exact, got) == [] and got["budget_hit"][0] == 0


@pytest.mark.parametrize("road", [False, True])
@pytest.mark.parametrize("depth", [2, 3])
def test_solver_at_the_edge_inside_the_tree(engine, road, depth):
    """E512: every child has at most 512 moves, 39 of them exactly 512 — searched completely, budget_hit 0 (a kernel that gives up at
    >= 512, or one that reports a give-up it never met, fails here).  E513, one move more: budget_hit 1."""
    fam = family()
    roots = np.stack([fam["edge_roots"]["E512"], fam["edge_roots"]["E513"]])
    cls = R.TinueRef if road else T.Ref
    rule, off_by_one = cls(N).solve(roots, depth, False), cls(N, capacity=511).solve(roots, depth, False)
    assert list(rule["budget_hit"]) == [0, 1] and list(off_by_one["budget_hit"]) == [1, 1]
    assert T.compare(cls(N, capacity=None).solve(roots[:1], depth, False), {f: rule[f][:1] for f in T.FIELDS}) == []  # E512: exact
    got = engine.solve(roots, depth, node_budget=BUDGET, road_only=road)
    assert T.compare_with_give_up(rule, got) == [] and list(got["budget_hit"]) == [0, 1]
    assert T.compare_with_give_up(off_by_one, got) != []


@pytest.mark.parametrize("road", [False, True])
def test_solver_depth4_against_the_committed_answers(engine, road):
    """depth 4 (two template levels above the cut list) on R, R_mirror and R_W: the reference takes minutes there, so its answers are
    committed (tests/golden/make_long_list_cases.py); where the file holds R's answer on whole lists, soundness against it"""
    import hashlib
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_list_depth4.json")) as f:
        doc = json.load(f)
    roots = np.stack([family()["roots"][k][0] for k in doc["names"]])
    assert hashlib.sha256(roots.tobytes()).hexdigest() == doc["sha256"], "the committed answers belong to other positions"
    ref = _table(doc["road_only" if road else "default"])
    got = engine.solve(roots, doc["depth"], node_budget=BUDGET, road_only=road)
    assert T.compare_with_give_up(ref, got) == []
    i = doc["names"].index("R")
    j = list(got["moves"][i]).index(family()["roots"]["R"][1])
    assert got["move_values"][i, j] == 0 and got["budget_hit"][i] == 1
    if "exact_R" in doc and not road:
        exact = _table([doc["exact_R"]])
        assert T.sound(exact, {f: got[f][i: i + 1] for f in ("value", "move_values")}, doc["depth"]) == []


def _table(rows):
    k = len(rows)
    out = dict(value=np.zeros(k, np.int8), best=np.zeros(k, np.uint16), counts=np.zeros(k, np.int32), budget_hit=np.zeros(k, np.uint8),
               moves=np.zeros((k, T.TG_MAX_MOVES), np.uint16), move_values=np.zeros((k, T.TG_MAX_MOVES), np.int8))
    for i, r in enumerate(rows):
        c = r["counts"]
        out["value"][i], out["best"][i], out["counts"][i], out["budget_hit"][i] = r["value"], r["best"], c, r["budget_hit"]
        out["moves"][i, :c], out["move_values"][i, :c] = r["moves"], r["move_values"]
    return out


def test_solver_refuses_a_root_above_the_capacity(engine, orc):
    import tak_amd

    ordinary = orc.random_positions(N, 12, seed=6, max_plies=60)
    ordinary = ordinary[orc.result(N, ordinary) == 0]
    batch = np.concatenate([ordinary[:3], family()["states"]["e513"][None], ordinary[3:]])
    for road in (False, True):
        with pytest.raises(tak_amd.TgError) as err:
            engine.solve(batch, 3, node_budget=BUDGET, road_only=road)
        assert err.value.code == -1 and "position 3" in str(err.value) and "TG_MAX_MOVES" in str(err.value)
    got = engine.solve(ordinary, 2, all_moves=True, node_budget=BUDGET)  # the same engine afterwards
    assert T.compare(T.Ref(N).solve(ordinary, 2, True), got) == []


def test_search_solve_on_live_roots(orc):
    import tak_amd

    roots = _roots()
    e = tak_amd.Engine(N, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    e.search_create(len(roots), arena_nodes=1 << 12)
    e.search_reset(roots)
    got = e.search_solve(3, node_budget=BUDGET)
    assert T.compare_with_give_up(_reference(False, 3, 512), got) == []
    e.close()


def test_search_root_above_the_capacity_is_a_limit(orc):
    import tak_amd

    ordinary = orc.random_positions(N, 8, seed=2, max_plies=40)
    ordinary = ordinary[orc.result(N, ordinary) == 0][:4]
    assert len(ordinary) == 4
    e = tak_amd.Engine(N, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    e.search_create(4, arena_nodes=1 << 14)
    e.search_reset(np.concatenate([ordinary[:2], family()["states"]["S"][None], ordinary[3:]]))
    with pytest.raises(tak_amd.TgError) as err:
        e.search_run(1)
        e.search_counters()
    assert err.value.code == -9 and "TG_MAX_MOVES" in str(err.value)  # TG_ERR_LIMIT
    # tg_search_reset clears the sticky error and the pool is whole: ordinary roots give the oracle's trees bit for bit
    e.search_reset(ordinary)
    e.search_run(30)
    s = orc.Search(N, head=orc.HEAD_CONV, evaluator=orc.EVAL_HASH)
    s.reset(ordinary)
    s.run(30)
    for g in range(4):
        a, b = e.search_dump(g), s.dump(g)
        assert len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names), f"tree {g} differs"
    e.close()


# ---- a list above the capacity met INSIDE a search tree (the tree kernel's branch) ------------------------------------------------
def _search_roots(orc):
    ordinary = orc.random_positions(N, 8, seed=2, max_plies=40)
    ordinary = ordinary[orc.result(N, ordinary) == 0][:3]
    assert len(ordinary) == 3
    return np.concatenate([ordinary[:2], family()["roots"]["R"][0][None], ordinary[2:]]), 2  # R among ordinary roots, its row


def _first_long_iteration(orc, roots, row, batch):
    """the first iteration at which the oracle's Search (no capacity) initialises a node of more than 512 children in tree `row`"""
    s = orc.Search(N, head=orc.HEAD_CONV, evaluator=orc.EVAL_HASH, batch=batch)
    s.reset(roots)
    for t in range(1, 9):
        s.run(1)
        nc = s.dump(row)["n_children"].astype(np.int64)
        if ((nc > 512) & (nc != 0xFFFF)).any():  # (0xFFFF marks a child that is not initialised yet)
            return t
    raise AssertionError("the oracle never reached a long list")


def _raises_limit(e):
    import tak_amd

    with pytest.raises(tak_amd.TgError) as err:
        e.search_run(1)
        e.search_counters()
    assert err.value.code == -9 and "TG_MAX_MOVES" in str(err.value)  # TG_ERR_LIMIT


@pytest.mark.parametrize("batch", [1, 4])
def test_search_meets_a_long_list_inside_the_tree(orc, batch):
    """every move of R leads to a position of more than 512 moves (its move f3 to S): one iteration short of the first that
    initialises such a child the trees are the oracle's bit for bit, at it the engine reports TG_ERR_LIMIT; tg_search_reset clears it"""
    import tak_amd

    roots, row = _search_roots(orc)
    t = _first_long_iteration(orc, roots, row, batch)
    assert t == (2 if batch == 1 else 1)  # the root's first rollout initialises it, its second descends into a child of R
    e = tak_amd.Engine(N, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    e.search_create(len(roots), arena_nodes=1 << 14, batch=batch)
    for states, iters in ((roots, t - 1), (None, 0), (np.concatenate([roots[:row], roots[:1], roots[row + 1:]]), 25)):
        if states is None:
            _raises_limit(e)
            continue
        e.search_reset(states)
        e.search_run(iters)
        e.search_counters()  # no error
        s = orc.Search(N, head=orc.HEAD_CONV, evaluator=orc.EVAL_HASH, batch=batch)
        s.reset(states)
        s.run(iters)
        for g in range(len(states)):
            a, b = e.search_dump(g), s.dump(g)
            assert len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names), f"tree {g} differs after {iters} iterations"
    e.close()


@pytest.mark.parametrize("mode", [dict(symmetry="hashed"), dict(proof="on")])
def test_search_meets_a_long_list_under_the_other_modes(orc, mode):
    import tak_amd

    roots, row = _search_roots(orc)
    t = _first_long_iteration(orc, roots, row, 1)
    assert t >= 1
    import torch_ref

    # (the hashed symmetry needs the network evaluator: a small random one; which leaf is met first does not depend on its values,
    # every child of R has a long list)
    e = tak_amd.Engine(N, res_blocks=2, filters=32, evaluator=tak_amd.EVAL_RESNET, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    e.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(N, 2, 32, "conv", seed=0)))
    e.search_create(len(roots), arena_nodes=1 << 14, **mode)
    e.search_reset(roots)
    e.search_run(t - 1)
    e.search_counters()
    _raises_limit(e)
    e.close()


def test_reanalyse_meets_a_long_list(orc):
    """window rows 0 - 2 ordinary, row 3 = R (its own list is short: the push accepts it), rows 4 - 5 ordinary, searched in slices of 3:
    TG_ERR_LIMIT; the slice of R is unchanged byte for byte, the slice before it is stored"""
    import tak_amd

    ordinary = orc.random_positions(N, 16, seed=12, max_plies=40)
    ordinary = ordinary[orc.result(N, ordinary) == 0][:5]
    assert len(ordinary) == 5
    sts = np.concatenate([ordinary[:3], family()["roots"]["R"][0][None], ordinary[3:]])
    om, oc = orc.movegen(N, sts)
    visits = (np.arange(512)[None, :] < oc[:, None]).astype(np.uint32) * 7
    e = tak_amd.Engine(N, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    e.window_create(len(sts))
    e.window_push(sts, oc, om, visits, np.zeros(len(sts), np.float32))
    e.search_create(3, arena_nodes=1 << 14)
    with pytest.raises(tak_amd.TgError) as err:
        e.reanalyse(0, len(sts), 10)
    assert err.value.code == -9 and "TG_MAX_MOVES" in str(err.value)
    _, states, moves, got = e.window_read(0, len(sts))
    assert np.array_equal(states, sts) and np.array_equal(moves, om)
    assert np.array_equal(got[3:], visits[3:])  # the failing slice: nothing stored
    s = orc.Search(N, head=orc.HEAD_CONV, evaluator=orc.EVAL_HASH)
    s.reset(sts[:3])
    s.run(10)
    assert np.array_equal(got[:3], s.root()["visits"]) and not np.array_equal(got[:3], visits[:3])  # the slice before it: stored
    e.close()


# ---- self-play: roots handed to a self-play object through tg_search_reset (it only needs a search object) --------------------------
SP_G, SP_SLOT, SP_PLIES = 8, 5, 150
SP_KW = dict(rollouts=12, noise_plies=6, exploit_plies=4, total_games=0, seed=21, arena_nodes=1 << 14, max_examples=1 << 14)


def _selfplay_games(orc, inject):
    import tak_amd

    e = tak_amd.Engine(N, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_CONV)
    e.selfplay_create(SP_G, **SP_KW)
    starts = np.repeat(orc.new_game(N, half_komi=4)[None], SP_G, axis=0)
    starts[SP_SLOT] = inject
    e.search_reset(starts)
    e.selfplay_step(SP_PLIES)
    st = e.selfplay_stats()  # raises if the engine carries a sticky error
    hdr, states, moves, visits = e.selfplay_drain(1 << 14)
    e.selfplay_step(1)       # … and it keeps going
    e.close()
    games = {}
    for i in range(len(hdr)):
        games.setdefault(int(hdr["game_id"][i]), []).append((states[i].tobytes(), moves[i].tobytes(), visits[i].tobytes(), float(hdr["result"][i])))
    return st, games


@pytest.mark.parametrize("which", ["S", "R"])
def test_selfplay_retires_the_game_with_a_long_list_alone(orc, which):
    """S as a root: the instant-win scan of the roots meets the long list.  R as a root: the tree kernel meets it one ply down.  Either
    way that game alone is retired (aborted_games = 1, no examples of it), and every other completed game is, example for example, the
    game of a run with an ordinary position in that slot."""
    fam = family()
    inject = fam["states"]["S"] if which == "S" else fam["roots"]["R"][0]
    ordinary = orc.random_positions(N, 8, seed=3, max_plies=30)
    ordinary = ordinary[(orc.result(N, ordinary) == 0) & posgen.reserves_consistent(ordinary, N)][0]
    st, games = _selfplay_games(orc, inject)
    ctl_st, ctl = _selfplay_games(orc, ordinary)
    print(f"inject {which}: {st}\ncontrol: {ctl_st}")
    assert ctl_st["aborted_games"] == 0 and st["aborted_games"] == 1 and st["alive_games"] == SP_G
    assert st["games_finished"] == len(games) and st["white_wins"] + st["black_wins"] + st["draws"] == st["games_finished"]
    assert not any(v[0][0] == inject.tobytes() for v in games.values())  # no example of the retired game
    common = [gid for gid in set(games) & set(ctl) if games[gid][0][0] == ctl[gid][0][0]]
    others = {gid for gid in ctl if (gid & 0xFFFFF) != SP_SLOT}  # (game_id = generation << 20 | slot)
    assert len(others) >= 2 and others <= set(common)  # every game the control run completed in another slot
    for gid in common:
        assert games[gid] == ctl[gid], f"game {gid:#x} differs from the run with an ordinary position in slot {SP_SLOT}"
