"""Batched virtual rollouts in the self-play driver (TgSelfPlayConfig.batch) and the one tree kernel per batched iteration.

`Player`'s batching (alpha-tak/src/player.rs:77-110): B virtual rollouts in one tree, one network call, B de-virtualisations in
rollout order.  The caller-driven search had it; here (1) `tg_search_run(iters = N)` at batch B goes through the fused
backup + select kernel and must leave the trees of `oracle.Search(batch = B)`, bit for bit, as must N calls of one iteration (the
two-kernel schedule); (2) the self-play driver at batch B is replayed ply by ply on `oracle.Search(batch = B)` — the oracle's
own `SelfPlay` knows one leaf per game only, so the phases of `self_play_parallel` around the search (opening, instant-win scan,
noise, pick, play, finish: oracle/tak_mcts.hpp `SelfPlay::ply_step`) are restated here on `oracle.movegen / play / result`;
(3) batch 0 and 1 are the driver as it was; (4) the limits of the field are argument errors; (5) a game that runs into a
capacity in the middle of a batch is retired alone.

The FC head's gather epilogue serves more than 2048 rows per forward only (FC_GATHER_ABOVE_ROWS), which 3 games × 16 rollouts
never reach: the cases with 3 games run the FC network through the backup's own gather, and one further case (130 games × 16)
runs it through the epilogue."""
import numpy as np
import pytest

from search_helpers import (BLACK_FLAT, BLACK_ROAD, WHITE_FLAT, WHITE_ROAD, Replay, _assert_same_examples, _assert_same_trees,
                            _engine_examples, _engines, _three_roots)

pytestmark = pytest.mark.gpu


# ---- 1. fused batched iterations -----------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [2, 5, 16])
@pytest.mark.parametrize("kind,n", [("hash", 5), ("hash", 6), ("net5_fc_2x32", 5), ("net6_conv_1x32", 6)])
def test_fused_batched_iterations_equal_the_oracle(orc, kind, n, batch):
    games, iters = 3, 40  # 3 games: the one workgroup of 4 waves is ragged
    sts = _three_roots(n)
    e, ev, okw = _engines(kind, n, max_batch=64)
    e.search_create(games, arena_nodes=1 << 16, batch=batch, seed=5)
    s = orc.Search(n, batch=batch, seed=5, **okw)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(iters)  # select | net | backup + select | … | backup: one tree kernel per iteration
    s.run(iters)
    _assert_same_trees(e, s, games)
    assert e.search_counters() == s.counters()
    assert e.search_counters()[0] == games * batch * iters > e.search_counters()[1]  # terminal leaves occurred
    # the same iterations one call each: the select and backup kernels on their own
    e.search_reset(sts)
    for _ in range(iters):
        e.search_run(1)
    _assert_same_trees(e, s, games)
    e.close()
    if ev:
        ev.close()


def test_fused_batched_iterations_through_the_fc_gather_epilogue(orc):
    n, games, batch, iters = 5, 130, 16, 6  # 2080 leaves per forward: above the 2048 rows the epilogue starts at; 130 = 32·4 + 2
    sts = orc.random_positions(n, games * 3, seed=17, max_plies=30, half_komi=4)
    sts = sts[orc.result(n, sts) == 0][:games]
    assert len(sts) == games
    e, ev, okw = _engines("net5_fc_2x32", n, max_batch=games * batch)
    e.search_create(games, arena_nodes=1 << 14, batch=batch)
    s = orc.Search(n, batch=batch, **okw)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(iters)
    s.run(iters)
    _assert_same_trees(e, s, games)
    assert e.search_counters() == s.counters()
    e.close()
    ev.close()


# ---- 2. the self-play driver at batch B against a replay on the oracle ------------------------------------------------------


def _replayed_selfplay(orc, kind, n, games, batch, rollouts, exploit_plies, max_plies=700):
    e, ev, okw = _engines(kind, n, max_batch=64)
    kw = dict(rollouts=rollouts, noise_plies=6, exploit_plies=exploit_plies, noise_alpha=0.2, noise_ratio=0.3, komi=2)
    e.selfplay_create(games, arena_nodes=1 << 16, seed=9, max_examples=1 << 13, total_games=games, batch=batch, **kw)
    rp = Replay(orc, n, games, batch, seed=9, **kw, **okw)
    got = []
    for ply in range(max_plies):
        moves, visits, counts = rp.before_the_pick()
        e.selfplay_step(1)
        after = e.search_states()
        got += _engine_examples(e.selfplay_drain(2048))
        if exploit_plies == 0:
            picked = rp.exploit_pick(moves, visits, counts)
        else:
            # a sampled pick: the move the engine played is read off its root state, or — the game ended with it and the slot
            # holds a fresh game — off the result its examples were completed with
            picked = np.zeros(games, np.uint16)
            sts = rp.s.states()
            for g in np.nonzero(rp.alive)[0]:
                c = int(counts[g])
                nxt, status = orc.play(n, np.repeat(sts[g][None], c, 0), moves[g, :c])
                assert not status.any()
                hit = np.nonzero((nxt == after[g]).all(1))[0]
                if len(hit) == 0:
                    mine = [x for x in got if x[0] == g]
                    assert mine, (ply, g)
                    white = mine[-1][2] if rp._to_move(mine[-1][3]) == 0 else -mine[-1][2]
                    res = orc.result(n, nxt)
                    want = (WHITE_ROAD, WHITE_FLAT) if white > 0 else (BLACK_ROAD, BLACK_FLAT) if white < 0 else (5, 6)
                    hit = np.nonzero(np.isin(res, want) & (visits[g, :c] > 0))[0]
                assert len(hit) >= 1, (ply, g)
                assert visits[g, hit[0]] > 0, (ply, g)  # a move without visits has probability 0
                picked[g] = moves[g, hit[0]]
        rp.play(picked, moves, visits, counts)
        # root states after every ply (a retired slot holds a fresh game in the engine and is not compared)
        now = rp.s.states()
        for g in np.nonzero(rp.alive)[0]:
            assert np.array_equal(after[g], now[g]), (ply, g)
        st = e.selfplay_stats()
        assert st["alive_games"] == int(rp.alive.sum()), (ply, st)
        assert st["expansions"] == rp.rollouts_run(), (ply, st["expansions"], rp.rollouts_run())
        if exploit_plies != 0:  # trees stay equal under the moves read back from the engine
            for g in np.nonzero(rp.alive)[0][:2]:
                a, b = e.search_dump(int(g)), rp.s.dump(int(g))
                assert len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names), (ply, g)
        if not rp.alive.any():
            break
    assert not rp.alive.any(), "games still running"
    while True:  # (whatever one drain per ply left behind)
        rest = _engine_examples(e.selfplay_drain(2048))
        if not rest:
            break
        got += rest
    _assert_same_examples(got, rp.examples)
    st = e.selfplay_stats()
    for k, v in rp.stats.items():
        assert st[k] == v, (k, st[k], v)
    assert st["aborted_games"] == 0 and st["dropped_examples"] == 0
    assert st["expansions"] == rp.rollouts_run()
    # what the parent commit, which ignored the field, fails: the visits of a searched example sum to about rollouts × batch
    searched = [x for x in got if not (x[5].max() == 1000 and set(x[5].tolist()) <= {1, 1000})]  # (not the instant-win scan's)
    assert searched and np.median([int(x[5].sum()) for x in searched]) >= rollouts * batch * 0.6
    e.close()
    if ev:
        ev.close()


@pytest.mark.parametrize("kind,n,games,batch,rollouts", [("hash", 5, 5, 4, 12), ("net6_conv_1x32", 6, 3, 8, 6)])
def test_selfplay_at_batch_b_equals_a_replay_on_the_oracle(orc, kind, n, games, batch, rollouts):
    _replayed_selfplay(orc, kind, n, games, batch, rollouts, exploit_plies=0)


def test_selfplay_at_batch_b_with_sampled_picks(orc):
    _replayed_selfplay(orc, "hash", 5, 5, 4, 12, exploit_plies=40)


# ---- 3. batch 0 and batch 1 are the driver as it was -------------------------------------------------------------------------


def test_batch_0_and_1_are_the_unbatched_driver(orc):
    import tak_amd

    n, games, plies = 5, 6, 60
    kw = dict(rollouts=16, noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=9)
    runs = []
    for batch in (0, 1):
        e = tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=64)
        e.selfplay_create(games, arena_nodes=1 << 15, seed=5, max_examples=1 << 13, batch=batch, **kw)
        e.selfplay_step(plies)
        runs.append((e.selfplay_stats(), e.selfplay_drain(1 << 13), e.search_states()))
        e.close()
    sp = orc.SelfPlay(n, games, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH, seed=5, **kw)  # one leaf per game: today's driver
    sp.step(plies)
    want = (sp.stats(), sp.drain(1 << 13))
    assert want[0]["examples"] > 0
    for st, drained, states in runs:
        assert st == want[0]
        assert all(np.array_equal(a, b) for a, b in zip(drained, want[1]))
        assert np.array_equal(states, runs[0][2])


# ---- 4. validation -------------------------------------------------------------------------------------------------------


def test_the_limits_of_the_batch_are_argument_errors():
    import tak_amd

    e = tak_amd.Engine(5, res_blocks=1, filters=32, evaluator=tak_amd.EVAL_RESNET, max_batch=64)
    e.init_random(seed=1)
    kw = dict(arena_nodes=1 << 12, rollouts=4, max_examples=256)
    for games, batch, names in [(9, 8, "max_batch"), (4, -1, "4096"), (1, 4097, "4096")]:
        with pytest.raises(tak_amd.TgError) as ei:
            e.selfplay_create(games, batch=batch, **kw)
        assert ei.value.code == -1 and names in str(ei.value), str(ei.value)  # TG_ERR_INVALID_ARG, naming the limit
    e.selfplay_create(8, batch=8, **kw)  # games × batch = max_batch is served
    e.selfplay_step(1)
    assert e.selfplay_stats()["plies"] == 1
    e.close()
    h = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64)
    for batch in (-1, 4097):
        with pytest.raises(tak_amd.TgError) as ei:
            h.selfplay_create(4, batch=batch, **kw)
        assert ei.value.code == -1 and "4096" in str(ei.value)
    h.close()


# ---- 5. a game retired in the middle of a batch ------------------------------------------------------------------------------


def test_a_game_retired_inside_a_batch_is_retired_alone(orc):
    """visit_limit as in test_gpu_limits, at batch 8.  Which games run into the table's end follows from the oracle: the
    select refuses a node whose visits + virtual visits reach visit_limit, the root has the largest sum of its tree, and before
    the j-th rollout of a ply the root holds the visits it was kept with plus j — so a game is retired in the ply in which
    kept + batch·(rollouts + 1) − 1 ≥ visit_limit (noise on every ply: rollouts + 1 iterations), by one of the LAST rollouts of
    that ply's last batch, the rest of which must be skipped.  The replay gives every first-generation game's largest such sum;
    with the limit at their median, the games above it must be retired (handled: no sticky error, the slot restarts) and
    the games below it must finish exactly as the unlimited replay plays them, example for example."""
    import tak_amd

    n, games, batch, rollouts = 5, 12, 8, 8
    kw = dict(rollouts=rollouts, noise_plies=512, exploit_plies=0, noise_alpha=0.2, noise_ratio=0.3, komi=2)
    rp = Replay(orc, n, games, batch, seed=21, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH, **kw)
    peak = np.zeros(games, np.int64)
    plies = 0
    while rp.alive.any():
        kept = rp.s.root()["root_visits"].astype(np.int64)
        if plies == 0:
            kept[:] = 0  # (the opening resets the trees)
        moves, visits, counts = rp.before_the_pick()
        searched = rp.alive.copy()  # (a game the instant-win scan ended was not searched in this ply)
        peak[searched] = np.maximum(peak[searched], kept[searched] + batch * (rollouts + 1) - 1)
        rp.play(rp.exploit_pick(moves, visits, counts), moves, visits, counts)
        plies += 1
        assert plies < 512
    limit = int(np.sort(peak)[games // 2])
    retired = {g for g in range(games) if peak[g] >= limit}
    finishing = set(range(games)) - retired
    assert retired and finishing and limit >= 16, (limit, sorted(peak.tolist()))
    print(f"visit_limit {limit}: largest root sums {sorted(peak.tolist())}, {len(retired)} games to retire, {plies} plies")

    e = tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=64)
    e.selfplay_create(games, arena_nodes=1 << 15, seed=21, total_games=0, max_examples=1 << 14, visit_limit=limit, batch=batch, **kw)
    e.selfplay_step(plies + 1)
    st = e.selfplay_stats()  # raises if the engine carries a sticky error
    hdr, states, moves, visits = e.selfplay_drain(1 << 14)
    e.selfplay_step(1)       # … and it keeps going
    e.sync()
    e.close()
    assert st["aborted_games"] >= len(retired) and st["alive_games"] == games and st["examples"] == len(hdr) > 0
    total = 2 * (21 + 1)  # stones and capstones of both sides on 5×5: on the board or in reserve, never gone
    h = states.shape[1] - 16
    for i in range(len(hdr)):
        assert 1 <= hdr["n_moves"][i] <= 512
        heights = states[i, 8 * n * n: 9 * n * n] & 63
        assert int(heights.sum()) + int(states[i, h + 4: h + 8].sum()) == total, i
        assert visits[i, : hdr["n_moves"][i]].sum() > 0
    got = _engine_examples((hdr, states, moves, visits))
    first = {x[0] for x in got if x[0] >> 20 == 0}
    assert first == finishing, (sorted(first), sorted(finishing))
    for g in sorted(finishing):
        _assert_same_examples([x for x in got if x[0] == g], [x for x in rp.examples if x[0] == g])
