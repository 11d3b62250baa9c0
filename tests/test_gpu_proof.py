"""Proven values in the search tree (tg_search_set_proof) on the GPU, against tests/proof_ref.py: the reference's MCTS with
the solver backup on the oracle's rules, whose arithmetic tests/test_proof_ref.py pins to oracle.Search bit for bit.  Trees,
result codes, counters, the proof-aware pick of self-play and of Player are the reference's exactly; mode off is the engine as
it was."""
import numpy as np
import pytest

import proof_ref as P
import tactics_ref
from search_helpers import _assert_same_examples, _assert_same_trees, _engine_examples, _engines

pytestmark = pytest.mark.gpu

TG_ERR_INVALID_ARG, TG_ERR_STATE = -1, -7


def _same_dump(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, np.nonzero(a[f] != b[f])[0][:4])


def _statuses_from_dump(d):
    """(root code, codes of the root's children) read from a TgNodeRecord dump: the children are the records at depth 1"""
    codes, i = [], 1
    for _ in range(int(d["n_children"][0])):
        codes.append(int(d["result"][i]))
        # skip the child's subtree: an initialised record is followed by its n_children subtrees
        pending = 1
        while pending:
            nc = int(d["n_children"][i])
            pending += -1 + (0 if nc == 0xFFFF else nc)
            i += 1
    return int(d["result"][0]), codes


# ---- 1, 2: trees, codes, tg_search_proof and the counters ----------------------------------------------------------------
@pytest.mark.parametrize("n", (5, 6))
@pytest.mark.parametrize("batch", (1, 4))
def test_trees_equal_the_reference(n, batch):
    """6 games (two blocks of waves): the dumps with their result codes, the statuses and the counters after ROLLOUTS rollouts,
    and again after tg_search_play on every game (the re-root carries the statuses; rollouts end on proven and finished roots)"""
    import tak_amd

    r = P.reference(n, batch)
    sts = P.inputs(n)
    games = len(sts)
    e, _, _ = _engines("hash", n, max_batch=64)
    e.search_create(games, arena_nodes=1 << 17, batch=batch, proof="on")
    assert e.search_get_proof() == (tak_amd.PROOF_ON, 0, 0)
    e.search_reset(sts)
    for rnd in range(2):
        e.search_run(r["iters"])
        dumps = [e.search_dump(g) for g in range(games)]
        for g in range(games):
            _same_dump(dumps[g], r["dumps"][rnd][g], (n, batch, rnd, g))
        p = e.search_proof()
        assert p["root_status"].tolist() == r["roots"][rnd]
        for g in range(games):
            root, kids = _statuses_from_dump(dumps[g])
            assert int(p["root_status"][g]) == root and int(p["counts"][g]) == len(kids)
            assert p["child_status"][g, : len(kids)].tolist() == kids and not p["child_status"][g, len(kids):].any()
        mode, proven, ended = e.search_get_proof()
        print(f"{n}x{n} batch {batch} round {rnd}: {proven} nodes proven, {ended} of {e.search_counters()[0]} rollouts ended on a proven node")
        assert (mode, proven, ended) == (tak_amd.PROOF_ON, *r["counters"][rnd])
        if rnd == 0:
            for g in range(games):
                mv, vis, codes = r["children"][g]
                assert p["child_status"][g, : len(codes)].tolist() == codes.tolist()
            e.search_play(r["picked"])
    assert any(c >= P.PROVEN_WHITE for d in dumps for c in d["result"][1:])


# ---- 6: off after on ------------------------------------------------------------------------------------------------------------
def test_off_after_on_is_the_plain_search(orc):
    import tak_amd

    n, batch, iters = 5, 4, 100
    sts = P.inputs(n)
    e, _, okw = _engines("hash", n, max_batch=64)
    e.search_create(len(sts), arena_nodes=1 << 15, batch=batch, proof=True)
    e.search_reset(sts)
    e.search_run(iters)
    assert e.search_get_proof()[1] > 0
    e.search_create(len(sts), arena_nodes=1 << 15, batch=batch)  # a create resets the mode
    assert e.search_get_proof() == (tak_amd.PROOF_OFF, 0, 0)
    e.search_reset(sts)
    e.search_run(iters)
    s = orc.Search(n, batch=batch, **okw)
    s.reset(sts)
    s.run(iters)
    _assert_same_trees(e, s, len(sts))
    assert e.search_get_proof() == (tak_amd.PROOF_OFF, 0, 0)
    assert not (e.search_proof()["child_status"] >= P.PROVEN_WHITE).any()
    # set and set back on the same object
    e.search_set_proof("on")
    e.search_set_proof("off")
    e.search_reset(sts)
    e.search_run(iters)
    _assert_same_trees(e, s, len(sts))
    with pytest.raises(tak_amd.TgError) as ei:
        e.search_set_proof(2)
    assert ei.value.code == TG_ERR_INVALID_ARG
    # trees that may hold proven codes are not handed to the off mode: off is refused until they are reset
    e.search_set_proof("on")
    e.search_reset(sts)
    e.search_run(iters)
    with pytest.raises(tak_amd.TgError) as ei:
        e.search_set_proof("off")
    assert ei.value.code == TG_ERR_STATE and e.search_get_proof()[0] == tak_amd.PROOF_ON
    e.search_reset(sts)
    e.search_set_proof("off")
    e.search_run(iters)
    _assert_same_trees(e, s, len(sts))


# ---- 3, 4: self-play -----------------------------------------------------------------------------------------------------------
def _selfplay_against_the_reference(n, games, total_games, seed, rollouts=48, exploit_plies=6, **schedule):
    kw = dict(rollouts=rollouts, noise_plies=4, exploit_plies=exploit_plies, total_games=total_games, seed=seed)
    ref = P.SelfPlay(n, games, **kw, **schedule)
    e, _, _ = _engines("hash", n, max_batch=64)
    e.selfplay_create(games, arena_nodes=1 << 15, max_examples=1 << 12, proof="on", **kw, **schedule)
    plies = 0
    while any(ref.alive):
        assert plies < 200
        ref.step()
        e.selfplay_step(1)
        plies += 1
        # every pick of this ply, the last of a game included: the position it led to (the start position again once a game has ended)
        assert np.array_equal(e.search_states(), np.stack([t.state for t in ref.trees])), plies
    st = e.selfplay_stats()
    assert st["alive_games"] == 0 and st["aborted_games"] == 0
    for k, v in ref.stats.items():
        assert st[k] == v, (k, st[k], v)
    c = ref.counters()
    assert (st["expansions"], st["evals"]) == (c["rollouts"], c["evals"])
    assert e.search_get_proof()[1:] == (c["nodes_proven"], c["ended_on_proven"])
    # every example (the state before each pick, the root's real visits, the outcome) — and with them every pick: the state of
    # an example is the position the previous pick of its game led to
    _assert_same_examples(_engine_examples(e.selfplay_drain(1 << 12)), ref.examples)
    return e, ref


def test_selfplay_equals_a_replay_driven_by_the_reference():
    """4×4, 6 slots, 9 games through slot recycling, played to the end; the seed is one for which the reference decides a move
    by step 1 and leaves candidates out in step 2"""
    e, ref = _selfplay_against_the_reference(4, 6, 10, seed=3)
    step1 = sum(1 for p in ref.picks if p[4] == 1)
    excluded = sum(1 for p in ref.picks if p[5] > 0)
    print(f"{len(ref.picks)} picks: {step1} decided by step 1, {excluded} with candidates left out; {ref.stats}")
    assert step1 >= 1 and excluded >= 1 and ref.stats["games_finished"] == 9 and max(ref.generation) >= 2


@pytest.mark.parametrize("batch,rollouts", [(1, 48), (2, 16)])
def test_selfplay_with_partial_compacted_lists(batch, rollouts):
    """a schedule with boost_factor 2: once a slot has been recycled the games under boost_plies are some of the live ones
    only, so the boosted rounds run through the list-mapped kernels; batch 2: through k_backup_select_batch<.., LIST, PROOF>, the
    one instantiation of the tree kernels that no other test reaches"""
    e, ref = _selfplay_against_the_reference(4, 6, 10, seed=3, rollouts=rollouts, batch=batch, boost_plies=6, boost_factor=2)
    sched = e.selfplay_schedule_stats()
    print(sched, ref.partial_lists, ref.counters())
    assert ref.partial_lists > 0 and sched["compact_iterations"] == ref.partial_lists * rollouts
    assert ref.counters()["nodes_proven"] > 0


@pytest.mark.parametrize("n,games,rollouts,seed", [(5, 6, 24, 0), (6, 5, 8, 1)])
def test_selfplay_explores_with_candidates_left_out(n, games, rollouts, seed):
    """exploit_plies beyond every game: each pick is the draw, so the children decided for the opponent are left out INSIDE the
    draw (their visits taken as 0).  Every ply is boosted and a finished slot retires, so from the first finished game on the
    boosted rounds run over a partial list: the list-mapped kernels compiled for 5 and 6.  The seeds are ones for which the reference
    alone makes such picks"""
    e, ref = _selfplay_against_the_reference(n, games, games, seed, rollouts=rollouts, exploit_plies=10000, boost_plies=512, boost_factor=2)
    masked = [p for p in ref.picks if p[5] > 0 and p[4] == 2 and not p[6]]
    print(f"{n}x{n}: {len(ref.picks)} picks, all drawn; {len(masked)} with candidates left out; {ref.partial_lists} partial lists; {ref.counters()}")
    assert len(masked) >= 4 and all(p[2] < 10000 for p in ref.picks)
    assert ref.partial_lists > 0 and e.selfplay_schedule_stats()["compact_iterations"] == ref.partial_lists * rollouts


# ---- 5: a network -------------------------------------------------------------------------------------------------------------
def test_trees_equal_the_reference_with_a_network():
    """TG_EVAL_RESNET on a golden net, 32 games: the reference is fed by tg_policy_eval of a second engine, one call per
    iteration on the leaves of all games"""
    n, games, batch, iters = 5, 32, 2, 40
    e, ev, _ = _engines("net5_fc_2x32", n, max_batch=64)
    sts = np.ascontiguousarray(tactics_ref.positions("p5_160")[:games])
    trees = [P.Tree(n, st, None, batch=batch, proof=True) for st in sts]
    P.Tree.run_lockstep(trees, iters, ev.policy_eval)
    e.search_create(games, arena_nodes=1 << 14, batch=batch, proof="on")
    e.search_reset(sts)
    e.search_run(iters)
    for g, t in enumerate(trees):
        _same_dump(e.search_dump(g), t.dump(), g)
    proven, ended = sum(t.nodes_proven for t in trees), sum(t.ended_on_proven for t in trees)
    assert proven >= 8 and ended > 0
    assert e.search_get_proof()[1:] == (proven, ended)
    assert e.search_counters() == (sum(t.rollouts for t in trees), sum(t.evals for t in trees))


# ---- 7: Player ------------------------------------------------------------------------------------------------------------------
def test_player_plays_a_won_position_out_by_proven_moves():
    """position 155 of the solver's cases: white wins within 3 plies.  The search proves the root; from then on every move of
    white is one into a position decided for white (step 1), whatever black answers, until white has won"""
    import tak_amd

    n = 5
    st = tactics_ref.positions("p5_160")[155]
    assert P.to_move(st) == P.W
    e, _, _ = _engines("hash", n, max_batch=64)
    p = tak_amd.Player(e, 8, False, st, arena_nodes=1 << 18, proof=True)
    for _ in range(32):
        if e.search_proof()["root_status"][0] == P.PROVEN_WHITE:
            break
        e.search_run(125)
    assert e.search_proof()["root_status"][0] == P.PROVEN_WHITE
    plies, res = 0, 0
    while res == 0:
        assert plies < 40
        white = P.to_move(p.state()) == P.W
        mv = p.pick_move(exploitation=not white)
        proof = p.last_proof
        moves = p.improved_policy()[0]
        k = int(np.nonzero(moves == mv)[0][0])
        status = int(tak_amd.node_status(proof["child_status"][0, k]))
        if white:
            assert status == P.W, (plies, k, proof["child_status"][0, : len(moves)])
        p.play_move(mv)
        res = int(e.result(p.state()[None])[0])
        plies += 1
    assert res in (P.WHITE_ROAD, P.WHITE_FLAT)


def test_argument_errors_on_the_device():
    import tak_amd

    e, _, _ = _engines("hash", 5, max_batch=64)
    with pytest.raises(tak_amd.TgError) as ei:
        e.search_set_proof("on")  # no search object
    assert ei.value.code == TG_ERR_STATE
    e.search_create(2)
    for bad in (-1, 2, 7):
        with pytest.raises(tak_amd.TgError) as ei:
            e.search_set_proof(bad)
        assert ei.value.code == TG_ERR_INVALID_ARG
    assert e.lib.tg_search_proof(e.h, None, None, None) == 0 and e.lib.tg_search_get_proof(e.h, None, None, None) == 0
