"""The self-play driver's rollout schedule (tg_selfplay_set_schedule: QUAD_ROLLOUT_PLIES, train/src/self_play.rs:19,63): a move
of a game whose ply < boost_plies gets boost_factor × rollouts iterations, the extra ones over a compacted list of the games that
are owed them.

(1) the budget: the driver replayed ply by ply on `oracle.Search`, phase (d) restated as `rollouts` iterations over all live games
followed by (factor − 1) · rollouts over the live games under boost_plies — without recycling all live games share a ply, so this
is the budget and the all-games path; (2) compaction: an endless run, where slots restart at different times and the list is
partial, against one single-slot engine per slot (one game: the list is empty or everything, never partial); (3) a schedule that
is off is the driver as it was; (4) everything boosted equals more rollouts; (5) a game that runs into a capacity inside a boost
is retired alone; (6) argument and state errors."""
import numpy as np
import pytest

from search_helpers import (BLACK_FLAT, BLACK_ROAD, WHITE_FLAT, WHITE_ROAD, Replay, _assert_same_examples, _engine_examples, _engines,
                            _golden_net)

pytestmark = pytest.mark.gpu

TG_ERR_INVALID_ARG, TG_ERR_STATE = -1, -7
TG_LIMIT_GAME_PLIES = 512


class BoostedReplay(Replay):
    """`Replay` with phase (d) of a scheduled ply: `rollouts` iterations over the live games, then (factor − 1) · rollouts over the
    live games whose root ply < boost_plies"""

    def __init__(self, *args, boost_plies=0, boost_factor=1, **kw):
        super().__init__(*args, **kw)
        self.boost_plies, self.boost_factor = boost_plies, boost_factor

    def before_the_pick(self):
        orc, n, G = self.orc, self.n, self.G
        sts = self.s.states()
        # (a) opening
        if all(self._ply(sts[g]) == 0 for g in range(G)):
            sts, status = orc.play(n, sts, np.zeros(G, np.uint16))
            assert not status.any()
            corner = np.zeros(G, np.uint16)
            for g in range(G):
                r = orc.philox(self.seed, g, 0, 0 | (1 << 16), 0)
                corner[g] = (n - 1) * n + (0 if int(r[0]) & 1 else n - 1)
            sts, status = orc.play(n, sts, corner)
            assert not status.any()
            self.s.reset(sts)
        # (b) instant-win scan
        mv, cnt = orc.movegen(n, sts)
        for g in range(G):
            if not self.alive[g]:
                continue
            c = int(cnt[g])
            nxt, status = orc.play(n, np.repeat(sts[g][None], c, 0), mv[g, :c])
            assert not status.any()
            res = orc.result(n, nxt)
            mine = (WHITE_ROAD, WHITE_FLAT) if self._to_move(sts[g]) == 0 else (BLACK_ROAD, BLACK_FLAT)
            wins = np.isin(res, mine)
            if wins.any():
                self.staged[g].append((sts[g].copy(), mv[g, :c].copy(), np.where(wins, 1000, 1).astype(np.uint32)))
                self.stats["instant_wins"] += 1
                self._finish(g, WHITE_FLAT if self._to_move(sts[g]) == 0 else BLACK_FLAT)
        # (c) one batch, then Dirichlet noise
        noisy = np.array([self.alive[g] and self._ply(sts[g]) < self.noise_plies for g in range(G)], np.uint8)
        if noisy.any():
            self.s.run(1, noisy)
            self.s.apply_dirichlet(self.noise_alpha, self.noise_ratio, noisy)
        # (d) the plain budget for every live game, then the rest of the boosted budget for the games under boost_plies
        if self.alive.any():
            self.s.run(self.rollouts, self._mask())
        boosted = np.array([self.alive[g] and self._ply(sts[g]) < self.boost_plies for g in range(G)], np.uint8)
        if boosted.any() and self.boost_factor > 1:
            self.s.run((self.boost_factor - 1) * self.rollouts, boosted)
        r = self.s.root()
        return r["moves"], r["visits"], r["counts"]


def _hash_engine(n, max_batch=64):
    import tak_amd

    return tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=max_batch, policy_head=tak_amd.HEAD_FC5 if n == 5 else tak_amd.HEAD_CONV)


def _searched(examples):
    """the examples of searched moves (not the instant-win scan's fake visits)"""
    return [x for x in examples if not (x[5].max() == 1000 and set(x[5].tolist()) <= {1, 1000})]


# ---- 1. the budget against the oracle ------------------------------------------------------------------------------------


def _replayed_schedule(orc, kind, n, games, batch, rollouts, exploit_plies, boost_plies, boost_factor, max_plies=700):
    """test_gpu_selfplay_batch._replayed_selfplay with a schedule: the same drive, ply by ply"""
    e, ev, okw = _engines(kind, n, max_batch=64)
    kw = dict(rollouts=rollouts, noise_plies=6, exploit_plies=exploit_plies, noise_alpha=0.2, noise_ratio=0.3, komi=2)
    e.selfplay_create(games, arena_nodes=1 << 16, seed=9, max_examples=1 << 13, total_games=games, batch=batch,
                      boost_plies=boost_plies, boost_factor=boost_factor, **kw)
    rp = BoostedReplay(orc, n, games, batch, seed=9, boost_plies=boost_plies, boost_factor=boost_factor, **kw, **okw)
    got = []
    for ply in range(max_plies):
        moves, visits, counts = rp.before_the_pick()
        e.selfplay_step(1)
        after = e.search_states()
        got += _engine_examples(e.selfplay_drain(2048))
        if exploit_plies == 0:
            picked = rp.exploit_pick(moves, visits, counts)
        else:  # a sampled pick is read off the engine's root state, or off the result the game's examples were completed with
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
                assert visits[g, hit[0]] > 0, (ply, g)
                picked[g] = moves[g, hit[0]]
        rp.play(picked, moves, visits, counts)
        now = rp.s.states()
        for g in np.nonzero(rp.alive)[0]:  # root states after every ply
            assert np.array_equal(after[g], now[g]), (ply, g)
        st = e.selfplay_stats()
        assert st["alive_games"] == int(rp.alive.sum()), (ply, st)
        assert st["expansions"] == rp.rollouts_run(), (ply, st["expansions"], rp.rollouts_run())
        if exploit_plies != 0:
            for g in np.nonzero(rp.alive)[0][:2]:
                a, b = e.search_dump(int(g)), rp.s.dump(int(g))
                assert len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names), (ply, g)
        if not rp.alive.any():
            break
    assert not rp.alive.any(), "games still running"
    while True:
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
    sched = e.selfplay_schedule_stats()
    e.close()
    if ev:
        ev.close()
    # the searched moves under boost_plies were given about boost_factor times the visits of the later ones (the slack of
    # test_gpu_selfplay_batch: 0.6), and boost_factor × rollouts × batch of their own
    searched = _searched(got)
    below = [int(x[5].sum()) for x in searched if rp._ply(x[3]) < boost_plies]
    above = [int(x[5].sum()) for x in searched if rp._ply(x[3]) >= boost_plies]
    print(f"visit sums: median {np.median(below)} under ply {boost_plies} ({len(below)} examples), {np.median(above)} from it on ({len(above)}); {sched}")
    assert below and above
    assert np.median(below) >= boost_factor * rollouts * batch * 0.6
    assert np.median(below) >= boost_factor * np.median(above) * 0.6
    # every live game shared a ply: each boosted ply listed all the games still playing; plies 2 … boost_plies − 1 of every game
    assert sched["boosted_moves"] >= len(below) and sched["boosted_moves"] <= games * (boost_plies - 2)


@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("exploit_plies", [0, 40])
def test_the_boosted_budget_equals_a_replay_on_the_oracle(orc, batch, exploit_plies):
    _replayed_schedule(orc, "hash", 5, 5, batch, 12, exploit_plies, boost_plies=6, boost_factor=4)


def test_the_boosted_budget_equals_a_replay_on_the_oracle_with_a_network(orc):
    _replayed_schedule(orc, "net6_conv_1x32", 6, 3, 8, 6, 0, boost_plies=4, boost_factor=3)


# ---- 2. compaction under mixing --------------------------------------------------------------------------------------------

# oracle.SelfPlay (hash evaluator, 5×5, noise_plies 6, exploit_plies 4, total_games 0) needs 203 – 263 plies until every one of
# 6 slots (173 – 228: of 3 slots) has finished two games, over seeds 5 and 9 and 8, 16 and 64 rollouts per move; the oracle's
# driver knows neither the batch nor the schedule, so this is the order of magnitude, taken with a margin — the test asserts
# the condition itself on what the engine drained.
MIX_PLIES = 400
MIX_KW = dict(rollouts=8, noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0, batch=2,
              boost_plies=8, boost_factor=4, seed=5, arena_nodes=1 << 15, max_examples=1 << 14)


def _mix_engine(kind, n, max_batch=64):
    if kind == "hash":
        return _hash_engine(n)
    import tak_amd

    gn, blocks, filters, head, tensors = _golden_net(kind)
    assert gn == n and head == "fc5"
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5, evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch)
    e.load_state_dict(tensors)
    return e


# (the 4×4 case at batch 1: the one-leaf list-mapped kernels without proofs, which no other test's lists reach — the replays above
# list every game still playing, which is the dense path while none has ended)
@pytest.mark.parametrize("kind,games,n,batch", [("hash", 6, 5, 2), ("net5_fc_2x32", 3, 5, 2), ("hash", 4, 4, 1)],
                         ids=["hash-6", "net5_fc_2x32-3", "hash-4-4x4-batch1"])
def test_a_partial_list_plays_every_slot_as_a_single_slot_engine_does(kind, games, n, batch):
    kw = dict(MIX_KW, batch=batch)
    e = _mix_engine(kind, n)
    e.selfplay_create(games, **kw)
    e.selfplay_step(MIX_PLIES)
    sched = e.selfplay_schedule_stats()
    st = e.selfplay_stats()
    hdr, states, moves, visits = e.selfplay_drain(1 << 14)
    e.close()
    assert st["dropped_examples"] == 0 and st["aborted_games"] == 0 and st["examples"] == len(hdr)
    # real partial lists occurred: compacted iterations, and narrower than all games
    print(f"{kind}: {sched}, mean width {sched['compact_leaves'] / max(sched['compact_iterations'], 1) / batch:.2f} of {games}")
    assert sched["compact_iterations"] > 0
    assert sched["compact_leaves"] < sched["compact_iterations"] * games * batch
    slot = hdr["game_id"] & 0xFFFFF
    gen = hdr["game_id"] >> 20
    for g in range(games):  # every slot has finished at least two games
        assert {0, 1} <= set(gen[slot == g].tolist()), (g, sorted(set(gen[slot == g].tolist())))
    for g in range(games):
        one = _mix_engine(kind, n)
        one.selfplay_create(1, slot_base=g, **kw)
        one.selfplay_step(MIX_PLIES)
        s1 = one.selfplay_schedule_stats()
        h1, st1, m1, v1 = one.selfplay_drain(1 << 14)
        one.close()
        assert s1["compact_iterations"] == 0 and s1["compact_leaves"] == 0 and s1["boosted_moves"] > 0  # one game: none or all
        keep = slot == g
        assert len(h1) == int(keep.sum()) > 0, (g, len(h1), int(keep.sum()))
        assert np.array_equal(h1, hdr[keep]), g  # game_id, n_moves, result
        assert np.array_equal(st1, states[keep]) and np.array_equal(m1, moves[keep]) and np.array_equal(v1, visits[keep]), g


# ---- 3. off is the driver as it was --------------------------------------------------------------------------------------


@pytest.mark.parametrize("batch", [1, 4])
def test_a_schedule_that_is_off_is_the_driver_without_one(orc, batch):
    """batch 1 against oracle.SelfPlay, with recycling.  The oracle's driver knows one leaf per game only: at batch 4 the oracle is
    `Replay` on `oracle.Search(batch = 4)`, which plays without recycling and picks the most visited move."""
    n, games, plies = 5, 4, 30
    kw = dict(rollouts=16, noise_plies=6, noise_alpha=0.2, noise_ratio=0.3, komi=2)
    kw.update(dict(exploit_plies=4, total_games=0) if batch == 1 else dict(exploit_plies=0, total_games=games))
    runs = []
    for setter in (None, (0, 4), (6, 1)):
        e = _hash_engine(n)
        e.selfplay_create(games, arena_nodes=1 << 15, seed=5, max_examples=1 << 13, batch=batch, **kw)
        if setter:
            e.selfplay_set_schedule(*setter)
        e.selfplay_step(plies)
        assert e.selfplay_schedule_stats() == dict(boosted_moves=0, compact_iterations=0, compact_leaves=0)
        runs.append((e.selfplay_stats(), e.selfplay_drain(1 << 13), e.search_states()))
        e.close()
    for st, drained, states in runs[1:]:
        assert st == runs[0][0]
        assert all(np.array_equal(a, b) for a, b in zip(drained, runs[0][1]))
        assert np.array_equal(states, runs[0][2])
    st, drained, states = runs[0]
    assert st["plies"] == plies and st["expansions"] > 0
    if batch == 1:
        sp = orc.SelfPlay(n, games, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH, seed=5, **kw)
        sp.step(plies)
        assert st == sp.stats()
        assert all(np.array_equal(a, b) for a, b in zip(drained, sp.drain(1 << 13)))
        assert np.array_equal(states, sp.states()[0])
    else:
        rp = Replay(orc, n, games, batch, seed=5, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH,
                    **{k: v for k, v in kw.items() if k != "total_games"})
        for _ in range(plies):
            if not rp.alive.any():
                break
            moves, visits, counts = rp.before_the_pick()
            rp.play(rp.exploit_pick(moves, visits, counts), moves, visits, counts)
        _assert_same_examples(_engine_examples(drained), rp.examples)
        for k, v in rp.stats.items():
            assert st[k] == v, (k, st[k], v)
        assert st["expansions"] == rp.rollouts_run() and st["alive_games"] == int(rp.alive.sum())
        now = rp.s.states()
        for g in np.nonzero(rp.alive)[0]:
            assert np.array_equal(states[g], now[g]), g


# ---- 4. everything boosted equals more rollouts ----------------------------------------------------------------------------


@pytest.mark.parametrize("n,batch,plies", [(5, 1, 160), (6, 2, 300)])
def test_all_plies_boosted_equals_the_multiple_of_the_rollouts(n, batch, plies):
    games, R, factor = 4, 6, 3
    kw = dict(noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0, arena_nodes=1 << 15, seed=7,
              max_examples=1 << 13, batch=batch)
    runs = []
    for rollouts, schedule in ((R, dict(boost_plies=TG_LIMIT_GAME_PLIES, boost_factor=factor)), (factor * R, {})):
        e = _hash_engine(n)
        e.selfplay_create(games, rollouts=rollouts, **schedule, **kw)
        e.selfplay_step(plies)
        runs.append((e.selfplay_stats(), e.selfplay_drain(1 << 13), e.search_states(), e.selfplay_schedule_stats()))
        e.close()
    (st_a, ex_a, roots_a, sched_a), (st_b, ex_b, roots_b, sched_b) = runs
    assert st_a["examples"] > 0 and st_a["games_finished"] > 0  # with recycling: slots restarted
    assert st_a == st_b
    assert all(np.array_equal(a, b) for a, b in zip(ex_a, ex_b))
    assert np.array_equal(roots_a, roots_b)
    assert sched_a["boosted_moves"] > 0 and sched_b == dict(boosted_moves=0, compact_iterations=0, compact_leaves=0)


def test_a_partial_list_through_the_fc_gather_epilogue():
    """The FC head's gather epilogue serves forwards of more than 2048 rows (test_gpu_selfplay_batch), which the small cases above
    never reach: their compacted iterations read the logits rows.  140 games × 16 rollouts without recycling and with every ply
    boosted: as soon as a game has ended the list is partial, and while at least 129 games play its forwards keep more than 2048
    rows.  Equal to the plain run with the multiple of the rollouts, whose dense iterations go through the epilogue at 2240 rows."""
    n, games, batch, R, factor, max_plies = 5, 140, 16, 2, 2, 150
    kw = dict(noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=games, arena_nodes=1 << 15, seed=11,
              max_examples=1 << 15, batch=batch)
    e = _mix_engine("net5_fc_2x32", n, max_batch=games * batch)
    e.selfplay_create(games, rollouts=R, boost_plies=TG_LIMIT_GAME_PLIES, boost_factor=factor, **kw)
    widths, last, plies = [], e.selfplay_schedule_stats(), 0
    while plies < max_plies:
        e.selfplay_step(1)
        plies += 1
        now = e.selfplay_schedule_stats()
        if now["compact_iterations"] > last["compact_iterations"]:
            widths.append((now["compact_leaves"] - last["compact_leaves"]) // (now["compact_iterations"] - last["compact_iterations"]))
        last = now
        if len([w for w in widths if w > 2048]) >= 3 or (widths and widths[-1] <= 2048):
            break
    print(f"{plies} plies, leaves per compacted forward {widths}")
    assert any(2048 < w < games * batch for w in widths), widths  # partial lists above the epilogue's threshold occurred
    got = (e.selfplay_stats(), e.selfplay_drain(1 << 15), e.search_states())
    e.close()
    p = _mix_engine("net5_fc_2x32", n, max_batch=games * batch)
    p.selfplay_create(games, rollouts=factor * R, **kw)
    p.selfplay_step(plies)
    want = (p.selfplay_stats(), p.selfplay_drain(1 << 15), p.search_states())
    p.close()
    assert got[0] == want[0] and got[0]["games_finished"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(got[1], want[1]))
    assert np.array_equal(got[2], want[2])


# ---- 5. a game retired inside a boost ---------------------------------------------------------------------------------------


def test_a_game_retired_inside_a_boost_is_retired_alone(orc):
    """visit_limit as in test_gpu_selfplay_batch: the select refuses a node whose visits + virtual visits reach visit_limit, the
    root holds the largest sum of its tree, and before the j-th rollout of a ply it holds the visits it was kept with plus j.  With
    noise on every ply a boosted ply runs 1 + factor · rollouts iterations, so in it game g reaches kept[g] + batch · (1 + factor ·
    rollouts) − 1.  In ply 2, the first searched one, every root starts empty; later the kept visits differ from game to game.
    The replay on the oracle is played until one game's sum stands at least 2 above every other game's and above every sum of
    the plies before; the limit is put one above the second largest.  That game is retired by one of the last rollouts of the
    ply's last batch but not by the very last — the rest of the batch must be skipped — and in the boosted part of the ply
    (asserted against the plain part's kept + batch · (1 + rollouts) − 1); every other game stays under the limit."""
    n, games, batch, rollouts, factor, boost_plies = 5, 6, 4, 16, 4, 8
    kw = dict(rollouts=rollouts, noise_plies=512, exploit_plies=0, noise_alpha=0.2, noise_ratio=0.3, komi=2)
    rp = BoostedReplay(orc, n, games, batch, seed=1, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH, boost_plies=boost_plies,
                       boost_factor=factor, **kw)

    def replay_ply():
        moves, visits, counts = rp.before_the_pick()
        assert rp.alive.all()  # (no instant win this early)
        rp.play(rp.exploit_pick(moves, visits, counts), moves, visits, counts)

    replay_ply()  # ply 2
    steps, highest, victim, limit = 1, batch * (1 + factor * rollouts) - 1, None, 0
    while steps + 2 < boost_plies:  # the ply about to be searched is steps + 2
        kept = rp.s.root()["root_visits"].astype(np.int64)
        peak = kept + batch * (1 + factor * rollouts) - 1
        order = np.argsort(peak)
        if peak[order[-1]] >= max(int(peak[order[-2]]), highest) + 2:
            victim, limit = int(order[-1]), max(int(peak[order[-2]]), highest) + 1
            break
        highest = max(highest, int(peak.max()))
        replay_ply()
        steps += 1
    assert victim is not None, "no ply under boost_plies singles a game out"
    assert peak[victim] > limit >= 16 and all(peak[g] < limit for g in range(games) if g != victim), (limit, peak.tolist())
    assert kept[victim] + batch * (1 + rollouts) - 1 < limit  # not before the boosted part of the ply
    print(f"visit_limit {limit}: root sums of ply {steps + 2} {sorted(peak.tolist())}, game {victim} to retire")
    replay_ply()  # that ply, unlimited: what the other games must look like

    e = _hash_engine(n)
    e.selfplay_create(games, arena_nodes=1 << 16, seed=1, total_games=0, max_examples=1 << 12, visit_limit=limit, batch=batch,
                      boost_plies=boost_plies, boost_factor=factor, **kw)
    e.selfplay_step(steps)
    before = e.selfplay_stats()
    assert before["aborted_games"] == 0
    e.selfplay_step(1)
    st = e.selfplay_stats()  # raises if the engine carries a sticky error
    assert st["aborted_games"] == before["aborted_games"] + 1 and st["alive_games"] == games
    roots, want = e.search_states(), rp.s.states()
    others = [g for g in range(games) if g != victim]
    for g in others:
        assert np.array_equal(roots[g], want[g]), g
        a, b = e.search_dump(g), rp.s.dump(g)
        assert len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names), g
    assert rp._ply(roots[victim]) == 0  # the slot holds a fresh game
    # … and the run keeps going: the restarted slot opens and searches its ply 2 beside the others' later plies.  The limit
    # was made for one ply: in the next one it retires the games whose kept visits carry them to it, by the same sum
    nxt = rp.s.root()["root_visits"].astype(np.int64) + batch * (1 + factor * rollouts) - 1
    late = [g for g in others if nxt[g] >= limit]
    replay_ply()
    e.selfplay_step(1)
    st = e.selfplay_stats()
    assert st["aborted_games"] == before["aborted_games"] + 1 + len(late) and st["plies"] == steps + 2 and st["alive_games"] == games
    roots, want = e.search_states(), rp.s.states()
    for g in others:
        if g in late:
            assert rp._ply(roots[g]) == 0, g
        else:
            assert np.array_equal(roots[g], want[g]), g
    assert rp._ply(roots[victim]) == 3
    e.close()


# ---- 6. argument and state errors -------------------------------------------------------------------------------------------


def test_argument_and_state_errors_of_the_schedule():
    import tak_amd

    e = _hash_engine(5)
    with pytest.raises(tak_amd.TgError) as ei:  # before tg_selfplay_create
        e.selfplay_set_schedule(10, 4)
    assert ei.value.code == TG_ERR_STATE and "tg_selfplay_create" in str(ei.value)
    e.search_create(4, arena_nodes=1 << 12)  # a caller-driven search is not a self-play driver either
    with pytest.raises(tak_amd.TgError) as ei:
        e.selfplay_set_schedule(10, 4)
    assert ei.value.code == TG_ERR_STATE and "tg_selfplay_create" in str(ei.value)
    kw = dict(arena_nodes=1 << 12, max_examples=256)
    e.selfplay_create(4, rollouts=4, **kw)
    for args, field in [((-1, 4), "boost_plies"), ((TG_LIMIT_GAME_PLIES + 1, 4), "boost_plies"), ((10, -1), "boost_factor"),
                        ((10, 0), "boost_factor"), ((10, 65), "boost_factor"), ((10, 4, (1, 0)), "reserved"),
                        ((10, 4, (0, -1)), "reserved")]:
        with pytest.raises(tak_amd.TgError) as ei:
            e.selfplay_set_schedule(*args)
        assert ei.value.code == TG_ERR_INVALID_ARG and field in str(ei.value), (args, str(ei.value))
    with pytest.raises(tak_amd.TgError) as ei:  # the keywords of selfplay_create reach the same check
        e.selfplay_create(4, rollouts=4, boost_plies=-1, boost_factor=4, **kw)
    assert ei.value.code == TG_ERR_INVALID_ARG and "boost_plies" in str(ei.value)
    e.selfplay_create(4, rollouts=1 << 26, **kw)
    with pytest.raises(tak_amd.TgError) as ei:  # 2^26 × 64 = 2^32
        e.selfplay_set_schedule(10, 64)
    assert ei.value.code == TG_ERR_INVALID_ARG and "boost_factor" in str(ei.value) and "rollouts" in str(ei.value)
    e.selfplay_set_schedule(10, 31)  # 2^26 × 31 < 2^31: served
    e.selfplay_create(4, rollouts=4, **kw)
    e.selfplay_set_schedule(TG_LIMIT_GAME_PLIES, 64)  # the largest values allowed; a second call before the first step replaces the first
    e.selfplay_set_schedule(10, 4)
    e.selfplay_step(1)
    with pytest.raises(tak_amd.TgError) as ei:  # after the first step
        e.selfplay_set_schedule(10, 4)
    assert ei.value.code == TG_ERR_STATE and "tg_selfplay_step" in str(ei.value)
    assert e.selfplay_schedule_stats()["boosted_moves"] == 4
    e.selfplay_create(4, rollouts=4, **kw)  # tg_selfplay_create clears schedule, counters and the state
    assert e.selfplay_schedule_stats() == dict(boosted_moves=0, compact_iterations=0, compact_leaves=0)
    e.selfplay_step(1)
    assert e.selfplay_schedule_stats() == dict(boosted_moves=0, compact_iterations=0, compact_leaves=0)
    assert e.selfplay_stats()["expansions"] == 4 * (1 + 4)  # noise iteration + rollouts, nothing boosted
    e.close()
