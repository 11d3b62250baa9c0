"""TG_SYMM_HASHED (tg_search_set_symmetry) on the GPU: one hashed dihedral image per evaluated leaf.  The oracle's search is given an
evaluator that does the same from the outside — s by tests/symm_ref.py (oracle.state_hash + Philox), tg_policy_eval on oracle.augment's
image, the policy back through the test-built permutation — and the trees, the self-play examples and the pit's games must be the
oracle's bit for bit; the engine's count of transformed leaves is the evaluator's count of calls with s ≠ 0.  Off, set back to off,
and a fresh create are the plain search (the existing parity); a sharded run equals the full run."""
import functools

import numpy as np
import pytest

import symm_ref
import torch_ref
from search_helpers import _assert_same_examples, _assert_same_trees, _engine_examples, _roots

pytestmark = pytest.mark.gpu

TG_ERR_INVALID_ARG, TG_ERR_STATE = -1, -7
NETS = {"fc5": (5, 2, 64, "fc5", 3), "conv6": (6, 1, 32, "conv", 4), "conv4": (4, 1, 32, "conv", 5)}


@functools.lru_cache(maxsize=None)
def _tensors(kind):
    n, blocks, filters, head, seed = NETS[kind]
    return torch_ref.abi_tensors(torch_ref.make_net(n, blocks, filters, head, seed=seed))


def _net_engine(kind, max_batch=64):
    import tak_amd

    n, blocks, filters, head, _ = NETS[kind]
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch,
                       policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV)
    e.load_state_dict(_tensors(kind))
    return e


def _oracle_side(orc, kind, ev, seed):
    """(oracle head, the hashed evaluator around engine `ev`'s plain tg_policy_eval)"""
    n, _, _, head, _ = NETS[kind]
    ohead = orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV
    return ohead, symm_ref.HashedEvaluator(orc, n, ohead, ev.policy_eval, symm_ref.perm_tables(n, head == "fc5"), seed)


@pytest.mark.parametrize("kind,games,iters,batch", [("fc5", 6, 60, 1), ("fc5", 6, 60, 4), ("conv6", 3, 40, 1)])
def test_hashed_trees_equal_the_oracle_with_the_hashed_evaluator(orc, kind, games, iters, batch):
    import tak_amd

    n = NETS[kind][0]
    e, ev = _net_engine(kind), _net_engine(kind)
    roots = _roots(orc, n, games, seed=21, max_plies=30)
    seed = 0xC0FFEE + batch
    before = e.search_get_symmetry()
    assert before == (tak_amd.SYMM_OFF, 0)
    e.search_create(games, arena_nodes=1 << 15, seed=seed, batch=batch, symmetry="hashed")
    assert e.search_get_symmetry()[0] == tak_amd.SYMM_HASHED
    e.search_reset(roots)
    e.search_run(iters)
    ohead, hashed = _oracle_side(orc, kind, ev, seed)
    s = orc.Search(n, head=ohead, py_eval=hashed, seed=seed, batch=batch)
    s.reset(roots)
    s.run(iters)
    _assert_same_trees(e, s, games)
    mode, transformed = e.search_get_symmetry()
    print(f"{kind} batch {batch}: {transformed} of {e.search_counters()[1]} evaluated leaves went to the network under s != 0")
    assert transformed == hashed.transformed > 0
    assert e.search_counters() == s.counters()
    # the image does change the search: the plain oracle grows other trees (the network is not equivariant)
    plain = orc.Search(n, head=ohead, py_eval=ev.policy_eval, seed=seed, batch=batch)
    plain.reset(roots)
    plain.run(iters)
    assert any(not np.array_equal(e.search_dump(g)["visits"], plain.dump(g)["visits"]) for g in range(games))
    # set back to OFF: the plain search again, on the same search object after a reset …
    e.search_set_symmetry("off")
    e.search_reset(roots)
    e.search_run(iters)
    _assert_same_trees(e, plain, games)
    assert e.search_get_symmetry() == (tak_amd.SYMM_OFF, transformed)
    # … and a create resets a mode that was on
    e.search_set_symmetry(tak_amd.SYMM_HASHED)
    e.search_create(games, arena_nodes=1 << 15, seed=seed, batch=batch)
    assert e.search_get_symmetry()[0] == tak_amd.SYMM_OFF
    e.search_reset(roots)
    e.search_run(iters)
    _assert_same_trees(e, plain, games)
    e.close()
    ev.close()


def test_a_sharded_run_equals_the_full_run(orc):
    """s is a function of the position and the seed, not of the slot: the games of a shard (slot_base) grow the trees they grow in
    the full run"""
    n, games, iters, seed = 5, 6, 40, 77
    roots = _roots(orc, n, games, seed=22, max_plies=30)
    full = _net_engine("fc5")
    full.search_create(games, arena_nodes=1 << 15, seed=seed, symmetry="hashed")
    full.search_reset(roots)
    full.search_run(iters)
    for base in (0, 3):
        shard = _net_engine("fc5")
        shard.search_create(3, arena_nodes=1 << 15, seed=seed, slot_base=base, symmetry="hashed")
        shard.search_reset(roots[base: base + 3])
        shard.search_run(iters)
        for g in range(3):
            a, b = shard.search_dump(g), full.search_dump(base + g)
            assert len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in a.dtype.names), (base, g)
        shard.close()
    full.close()


def test_hashed_selfplay_equals_the_oracle_driver(orc):
    """4 slots, 12 plies, 16 rollouts against oracle.SelfPlay with the hashed evaluator: statistics, root states, examples and their order.
    No schedule here: slots in lock-step cannot give a partial list within 12 plies, so the compacted list has the test below to
    itself, played until games end; on the FC5 head the mapped child_pidx under the gather epilogue is covered by dense
    iterations only (this test, the trees and the pit)."""
    n, games, plies, seed = 5, 4, 12, 13
    kw = dict(rollouts=16, noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0)
    e, ev = _net_engine("fc5"), _net_engine("fc5")
    e.selfplay_create(games, arena_nodes=1 << 15, seed=seed, max_examples=1 << 12, symmetry="hashed", **kw)
    e.selfplay_step(plies)
    ohead, hashed = _oracle_side(orc, "fc5", ev, seed)
    sp = orc.SelfPlay(n, games, head=ohead, py_eval=hashed, seed=seed, **kw)
    sp.step(plies)
    assert e.selfplay_stats() == sp.stats()
    assert np.array_equal(e.search_states(), sp.states()[0])
    assert all(np.array_equal(a, b) for a, b in zip(e.selfplay_drain(1 << 12), sp.drain(1 << 12)))
    assert e.search_get_symmetry()[1] == hashed.transformed > 0
    e.close()
    ev.close()


def test_hashed_selfplay_with_a_compacted_list_equals_the_replay(orc):
    """The rollout schedule with every ply boosted (boost_plies = 512) and no recycling: once the first game has ended the boosted
    iterations run over a compacted list of the games still playing — list slots, not game slots, carry the leaves.  4×4, where games
    are short, on a tower that takes planes: under the hashed mode the tree kernel hands over packed leaves instead.  The replay is
    test_gpu_rollout_schedule's, on oracle.Search with the hashed evaluator; moves are the most visited ones (exploit_plies 0)."""
    from test_gpu_rollout_schedule import BoostedReplay

    n, games, batch, seed = 4, 4, 2, 9
    kw = dict(rollouts=6, noise_plies=4, exploit_plies=0, noise_alpha=0.2, noise_ratio=0.3, komi=2)
    e, ev = _net_engine("conv4"), _net_engine("conv4")
    e.selfplay_create(games, arena_nodes=1 << 15, seed=seed, max_examples=1 << 12, total_games=games, batch=batch, boost_plies=512,
                      boost_factor=2, symmetry="hashed", **kw)
    ohead, hashed = _oracle_side(orc, "conv4", ev, seed)
    rp = BoostedReplay(orc, n, games, batch, seed=seed, boost_plies=512, boost_factor=2, head=ohead, py_eval=hashed, **kw)
    got = []
    for ply in range(200):
        moves, visits, counts = rp.before_the_pick()
        e.selfplay_step(1)
        got += _engine_examples(e.selfplay_drain(2048))
        rp.play(rp.exploit_pick(moves, visits, counts), moves, visits, counts)
        after, now = e.search_states(), rp.s.states()
        for g in np.nonzero(rp.alive)[0]:
            assert np.array_equal(after[g], now[g]), (ply, g)
        if not rp.alive.any():
            break
    assert not rp.alive.any(), "games still running"
    got += _engine_examples(e.selfplay_drain(2048))
    _assert_same_examples(got, rp.examples)
    sched = e.selfplay_schedule_stats()
    print(f"hashed self-play with a schedule: {ply + 1} plies, {sched}, {e.search_get_symmetry()[1]} transformed leaves")
    assert sched["compact_iterations"] > 0 and sched["compact_leaves"] < sched["compact_iterations"] * games * batch  # a partial list ran
    assert e.search_get_symmetry()[1] == hashed.transformed > 0
    assert e.selfplay_stats()["expansions"] == rp.rollouts_run()
    e.close()
    ev.close()


def test_hashed_pit_equals_the_oracle_replay(orc):
    """one pair, both engines hashed (the setter on each engine before the call; tg_pit creates the searches), against
    test_gpu_pit's replay with a hashed evaluator per network"""
    import tak_amd
    from test_gpu_pit import _oracle_pit

    n, seed = 5, 11
    new, old = _net_engine("fc5"), _net_engine("fc5")
    old.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(5, 2, 64, "fc5", seed=8)))
    ev_new, ev_old = _net_engine("fc5"), _net_engine("fc5")
    ev_old.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(5, 2, 64, "fc5", seed=8)))
    kw = dict(pairs=1, rollouts=8, batch=2, idle_rollouts=1, random_plies=2, komi=2, seed=seed, max_plies=24)
    got = tak_amd.pit(new, old, arena_nodes=1 << 15, symmetry="hashed", **kw)
    assert new.search_get_symmetry()[0] == tak_amd.SYMM_HASHED and old.search_get_symmetry()[0] == tak_amd.SYMM_HASHED
    hashed = [_oracle_side(orc, "fc5", ev, seed)[1] for ev in (ev_new, ev_old)]
    want = _oracle_pit(orc, n, hashed, kw["pairs"], kw["rollouts"], kw["idle_rollouts"], 2, 2, seed, max_plies=24, batch=2)
    for k in ("wins", "losses", "draws", "plies", "unfinished", "ref_wins", "ref_losses", "ref_draws", "ref_pairs"):
        assert got[k] == want[k], (got, want)
    assert new.search_get_symmetry()[1] == hashed[0].transformed > 0
    assert old.search_get_symmetry()[1] == hashed[1].transformed > 0
    # the same match with the mode off on both engines: the counts stay where they were
    plain = tak_amd.pit(new, old, arena_nodes=1 << 15, symmetry="off", **kw)
    assert new.search_get_symmetry() == (tak_amd.SYMM_OFF, hashed[0].transformed)  # nothing was transformed with the mode off
    assert plain["plies"] > 0
    for x in (new, old, ev_new, ev_old):
        x.close()


def test_argument_and_state_errors():
    import tak_amd

    e = _net_engine("fc5")
    e.search_set_symmetry("hashed")  # without a search: kept for the searches tg_pit creates
    assert e.search_get_symmetry()[0] == tak_amd.SYMM_HASHED
    e.search_set_symmetry("off")
    with pytest.raises(tak_amd.TgError) as ei:
        e.search_set_symmetry(2)
    assert ei.value.code == TG_ERR_INVALID_ARG
    e.close()
    h = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=8)
    h.search_create(2, arena_nodes=1 << 12)
    with pytest.raises(tak_amd.TgError) as ei:
        h.search_set_symmetry("hashed")
    assert ei.value.code == TG_ERR_STATE
    h.close()
