"""GPU-resident MCTS and self-play driver (through the C ABI) against the CPU oracle: whole trees,
bit for bit (visit counts, f32 priors and values compared as raw bits), with the deterministic test
evaluators and with the real network."""
import numpy as np
import pytest

import torch_ref
from search_helpers import _assert_same_trees, _best, _mk, _roots

pytestmark = pytest.mark.gpu


def test_dummynet_behaviour_3x3(orc):
    # alpha-tak/src/search/tests.rs:37-72 on the GPU (DummyNet: policy 1.0, eval 0)
    import tak_amd

    e = _mk(3, tak_amd.EVAL_DUMMY, 2)
    e.search_create(2, arena_nodes=1 << 15)
    st = np.stack([orc.from_ptn(3, ["a3", "c3", "c2", "a2"]), orc.from_ptn(3, ["a3", "c3", "c2"])])
    e.search_reset(st)
    e.search_run(1000)
    r = e.search_root()
    mv0 = _best(r, 0)
    st2, status = orc.play(3, st[0], [mv0])
    assert status[0] == 0 and orc.result(3, st2)[0] == 1  # win in one: Winner { White, road }
    # same trees as the oracle, bit for bit
    s = orc.Search(3, evaluator=orc.EVAL_DUMMY)
    s.reset(st)
    s.run(1000)
    _assert_same_trees(e, s, 2)
    # prevent win in two: play black's choice, search again, white cannot win immediately
    mv1 = _best(r, 1)
    e.search_play([mv0, mv1])
    s.play([mv0, mv1])
    assert np.array_equal(e.search_states(), s.states())
    act = np.array([0, 1], np.uint8)
    e.search_run(1000, act)
    s.run(1000, act)
    _assert_same_trees(e, s, 2)
    r = e.search_root()
    st3, status = orc.play(3, e.search_states()[1], [_best(r, 1)])
    assert status[0] == 0 and orc.result(3, st3)[0] == 0
    e.close()


@pytest.mark.parametrize("n,games,iters", [(5, 24, 300), (6, 12, 200), (4, 16, 300)])
def test_tree_parity_hash_evaluator(orc, n, games, iters):
    import tak_amd

    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.search_create(games, arena_nodes=1 << 16, seed=99)
    head = orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV
    s = orc.Search(n, head=head, evaluator=orc.EVAL_HASH, seed=99)
    sts = _roots(orc, n, games, seed=n, max_plies=40 if n >= 5 else 16)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(iters)
    s.run(iters)
    _assert_same_trees(e, s, games)
    assert e.search_counters() == s.counters()
    # Dirichlet noise from the counter-based RNG, then more search, then tree reuse — three rounds
    for rnd in range(3):
        e.search_apply_dirichlet(0.2, 0.3)
        s.apply_dirichlet(0.2, 0.3)
        e.search_run(60)
        s.run(60)
        _assert_same_trees(e, s, games)
        r = e.search_root()
        ro = s.root()
        for k in ("moves", "visits", "counts", "root_visits"):
            assert np.array_equal(r[k], ro[k])
        assert np.array_equal(r["prior"].view(np.uint32), ro["prior"].view(np.uint32))
        assert np.array_equal(r["q"].view(np.uint32), ro["q"].view(np.uint32))
        mv = np.array([_best(r, g) for g in range(games)], np.uint16)
        # stop advancing games that the move would end
        nxt, _ = orc.play(n, e.search_states(), mv)
        act = (orc.result(n, nxt) == 0).astype(np.uint8)
        e.search_play(mv, act)
        s.play(mv, act)
        assert np.array_equal(e.search_states(), s.states())
        _assert_same_trees(e, s, games)
        e.search_run(50, act)
        s.run(50, act)
        _assert_same_trees(e, s, games)
    e.close()


def test_caller_noise_and_errors(orc):
    import tak_amd

    e = _mk(5, tak_amd.EVAL_HASH, 4)
    e.search_create(4, arena_nodes=1 << 14)
    s = orc.Search(5, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH)
    sts = _roots(orc, 5, 4, seed=2, max_plies=20)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(10)
    s.run(10)
    noise = np.random.default_rng(0).random((4, 512)).astype(np.float32)
    e.search_apply_noise(noise, 0.25)
    s.apply_noise(noise, 0.25)
    _assert_same_trees(e, s, 4)
    with pytest.raises(tak_amd.TgError) as ei:
        e.search_play(np.full(4, 0xFFFF, np.uint16))  # not a child of any root
    assert ei.value.code == -8
    e.close()


def test_arena_overflow_is_reported(orc):
    import tak_amd

    e = _mk(5, tak_amd.EVAL_DUMMY, 2)
    e.search_create(2, arena_nodes=1024)
    e.search_reset(_roots(orc, 5, 2, seed=4, max_plies=30))
    e.search_run(400)
    with pytest.raises(tak_amd.TgError) as ei:
        e.search_root()
    assert ei.value.code == -5
    # the error is sticky until the trees are reset; afterwards the pool is whole again
    with pytest.raises(tak_amd.TgError):
        e.search_run(1)
        e.search_root()
    e.search_reset(_roots(orc, 5, 2, seed=4, max_plies=30))
    e.search_run(20)
    assert (e.search_root()["root_visits"] == 20).all()
    e.close()


def test_one_pool_for_all_trees(orc):
    """All trees live in one node pool handed out in chunks (search.cuh): one game may grow far beyond the average budget
    while the others stay small, and the chunks of discarded subtrees are reused — 60 plies of search + tree reuse allocate
    many times the pool.  Trees stay bit-identical to the oracle's throughout."""
    import tak_amd

    n, games = 5, 12
    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.search_create(games, arena_nodes=3072, seed=21)  # pool = 36 864 nodes + slack, chunks of 1024
    s = orc.Search(n, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH, seed=21)
    sts = _roots(orc, n, games, seed=8, max_plies=12)
    e.search_reset(sts)
    s.reset(sts)
    only0 = np.zeros(games, np.uint8)
    only0[0] = 1
    e.search_run(400, only0)  # ≈ 25 000 nodes in ONE tree: eight times the per-game average
    s.run(400, only0)
    e.search_run(30)
    s.run(30)
    _assert_same_trees(e, s, games)
    assert len(e.search_dump(0)) > 5 * 3072
    expansions = 0
    for ply in range(60):
        r = e.search_root()
        mv = np.array([_best(r, g) if r["counts"][g] else 0 for g in range(games)], np.uint16)
        nxt, _ = orc.play(n, e.search_states(), mv)
        act = ((orc.result(n, nxt) == 0) & (r["counts"] > 0)).astype(np.uint8)
        if not act.any():
            break
        e.search_play(mv, act)
        s.play(mv, act)
        e.search_run(40, act)
        s.run(40, act)
        expansions += 40 * int(act.sum())
        if ply % 8 == 7:
            _assert_same_trees(e, s, games)
    _assert_same_trees(e, s, games)
    assert e.search_counters() == s.counters()
    assert expansions * 30 > 4 * games * 3072  # far more nodes were allocated than the pool holds at once
    e.close()


# (5×5 with Net6's conv head is not a reference configuration — its move index is the conv formula, as include/takgpu.h defines
# TG_HEAD_CONV; round 6: the oracle took the legacy table for every 5×5 move, whatever the head's size)
@pytest.mark.parametrize("n,blocks,filters,head", [(5, 2, 32, "fc5"), (6, 1, 32, "conv"), (5, 1, 64, "conv")])
def test_tree_parity_with_real_network(orc, n, blocks, filters, head):
    # the oracle's MCTS evaluates its leaves through tg_policy_eval; the GPU search feeds the same
    # kernels from its own leaf batch — identical trees require identical per-position network outputs
    _tree_parity_with_real_network(orc, n, blocks, filters, head, torch_ref.make_net(n, blocks, filters, head, seed=3))


@pytest.mark.parametrize("n,blocks,filters,head", [(5, 2, 64, "fc5"), (6, 1, 128, "conv")])
def test_tree_parity_with_a_trained_like_network(orc, n, blocks, filters, head):
    """the same parity on torch_ref.make_trained_net: peaked priors (median largest p ≥ 0.2) and values near ±1 travel through whole trees
    bit for bit — the backup's stat_exp at arguments down to −30 and beyond, selections decided by priors rather than by ties"""
    import posgen

    planes = orc.encode(n, posgen.distinct_positions(orc, n, 256, seed=41, max_plies=60))
    _tree_parity_with_real_network(orc, n, blocks, filters, head, torch_ref.make_trained_net(n, blocks, filters, head, planes, seed=41))


def _tree_parity_with_real_network(orc, n, blocks, filters, head, net):
    import tak_amd

    games = 12
    tensors = torch_ref.abi_tensors(net)
    h = tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV
    e = _mk(n, tak_amd.EVAL_RESNET, games, head=h, res_blocks=blocks, filters=filters)
    e.load_state_dict(tensors)
    ev = _mk(n, tak_amd.EVAL_RESNET, games, head=h, res_blocks=blocks, filters=filters)
    ev.load_state_dict(tensors)
    e.search_create(games, arena_nodes=1 << 15)
    s = orc.Search(n, head=orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV, py_eval=lambda st: ev.policy_eval(st))
    sts = _roots(orc, n, games, seed=8, max_plies=30)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(150)
    s.run(150)
    _assert_same_trees(e, s, games)
    e.close()
    ev.close()


@pytest.mark.parametrize("n,blocks,filters,head", [(5, 2, 64, "fc5"), (6, 1, 128, "conv")])
def test_tree_parity_on_the_bf16x3_path(orc, n, blocks, filters, head):
    # the split-bf16 tower / policy FC inside the lock-step search: same trees as the oracle's MCTS fed by the same
    # kernels through tg_policy_eval (per-position outputs do not depend on the batch), and a short self-play runs clean
    import tak_amd

    games = 10
    net = torch_ref.make_net(n, blocks, filters, head, seed=4)
    tensors = torch_ref.abi_tensors(net)
    engines = []
    for _ in range(2):
        e = _mk(n, tak_amd.EVAL_RESNET, games, res_blocks=blocks, filters=filters)
        e.set_precision("bf16x3")
        e.load_state_dict(tensors)
        engines.append(e)
    e, ev = engines
    e.search_create(games, arena_nodes=1 << 15)
    s = orc.Search(n, head=orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV, py_eval=lambda st: ev.policy_eval(st))
    sts = _roots(orc, n, games, seed=9, max_plies=30)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(120)
    s.run(120)
    _assert_same_trees(e, s, games)
    e.selfplay_create(games, arena_nodes=1 << 14, seed=2, rollouts=16, max_examples=4096)
    e.selfplay_step(6)
    e.sync()
    st = e.selfplay_stats()
    assert st["expansions"] >= 6 * 16 * games * 0.9 and st["plies"] == 6
    e.close()
    ev.close()


@pytest.mark.parametrize("n,games,batch,iters", [(4, 6, 4, 60), (5, 5, 16, 40), (3, 3, 8, 50)])
def test_batched_virtual_rollouts_match_oracle(orc, n, games, batch, iters):
    # Player's batching (player.rs:77-93): `batch` virtual rollouts per tree, ONE evaluation batch, de-virtualisation in order.
    # Later rollouts of a batch see the virtual visits (and the temporary uniform priors) the earlier ones left.
    import tak_amd

    e = _mk(n, tak_amd.EVAL_HASH, games * batch)
    e.search_create(games, arena_nodes=1 << 17, batch=batch)
    s = orc.Search(n, head=orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV, evaluator=orc.EVAL_HASH, batch=batch)
    sts = _roots(orc, n, games, seed=12, max_plies=20 if n > 3 else 4)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(iters)
    s.run(iters)
    _assert_same_trees(e, s, games)
    assert e.search_counters()[0] == games * batch * iters == s.counters()[0]
    # advance every game by its most visited move and keep searching the reused trees
    r = e.search_root()
    mv = np.array([_best(r, g) for g in range(games)], np.uint16)
    e.search_play(mv)
    s.play(mv)
    e.search_run(10)
    s.run(10)
    _assert_same_trees(e, s, games)
    e.close()


def test_masked_and_short_runs_at_batch_4_match_oracle(orc):
    # the iteration schedules beside the long dense one, at batch > 1: a masked run (select(mask) | evaluate | backup per iteration,
    # nothing fused: the fused kernels take no mask), then the two ends of the fused loop — one iteration (select | backup) and
    # two (select | backup+select | backup)
    import tak_amd

    n, games, batch = 5, 4, 4
    e = _mk(n, tak_amd.EVAL_HASH, games * batch)
    e.search_create(games, arena_nodes=1 << 17, batch=batch)
    s = orc.Search(n, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH, batch=batch)
    sts = _roots(orc, n, games, seed=12, max_plies=20)
    e.search_reset(sts)
    s.reset(sts)
    mask = np.array([1, 0, 1, 1], np.uint8)
    e.search_run(30, mask)
    s.run(30, mask)
    _assert_same_trees(e, s, games)
    for iters in (1, 2):
        e.search_run(iters)
        s.run(iters)
    _assert_same_trees(e, s, games)
    assert e.search_counters() == s.counters() and s.counters()[0] > 0
    e.close()


def test_batched_rollouts_with_real_network(orc):
    import tak_amd

    n, blocks, filters, games, batch = 5, 2, 64, 4, 16
    net = torch_ref.make_net(n, blocks, filters, "fc5", seed=5)
    tensors = torch_ref.abi_tensors(net)
    e = _mk(n, tak_amd.EVAL_RESNET, games * batch, res_blocks=blocks, filters=filters)
    e.load_state_dict(tensors)
    ev = _mk(n, tak_amd.EVAL_RESNET, games * batch, res_blocks=blocks, filters=filters)
    ev.load_state_dict(tensors)
    e.search_create(games, arena_nodes=1 << 17, batch=batch)
    s = orc.Search(n, head=orc.HEAD_FC5, py_eval=lambda st: ev.policy_eval(st), batch=batch)
    sts = _roots(orc, n, games, seed=14, max_plies=25)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(30)
    s.run(30)
    _assert_same_trees(e, s, games)
    with pytest.raises(tak_amd.TgError):
        e.search_create(games, batch=2 * batch)  # games x batch > max_batch
    e.close()
    ev.close()


def test_dirichlet_spec_matches_oracle(orc):
    import tak_amd

    e = _mk(5, tak_amd.EVAL_DUMMY, 3)
    e.search_create(3, arena_nodes=1 << 12, seed=1234)
    sts = _roots(orc, 5, 3, seed=6, max_plies=25)
    e.search_reset(sts)
    e.search_run(1)  # expand the roots: priors become the DummyNet's 1.0
    e.search_apply_dirichlet(0.2, 0.5)
    r = e.search_root()
    for g in range(3):
        c = r["counts"][g]
        ply = int(sts[g][256 - 16 + 2]) | (int(sts[g][256 - 16 + 3]) << 8)
        noise = orc.dirichlet(c, 0.2, 1234, g, 0, ply)
        want = noise * np.float32(0.5) + np.float32(1.0) * (np.float32(1.0) - np.float32(0.5))
        assert np.array_equal(r["prior"][g, :c].view(np.uint32), want.astype(np.float32).view(np.uint32))
        assert abs(float(noise.sum()) - 1.0) < 1e-5
    e.close()


def test_selfplay_config_c1_with_the_real_network(orc):
    """BASELINE config C1 (5×5, 64 games, 100 sims/move) on the C2 network for the first plies of every game: the oracle's
    self_play_parallel evaluates its leaf batches through tg_policy_eval, the engine through its own leaf batch — same
    statistics after every ply, same examples."""
    import tak_amd

    games, rollouts, plies = 64, 100, 10
    net = torch_ref.make_net(5, 6, 64, "fc5", seed=0)
    tensors = torch_ref.abi_tensors(net)
    e = _mk(5, tak_amd.EVAL_RESNET, games, res_blocks=6, filters=64)
    e.load_state_dict(tensors)
    ev = _mk(5, tak_amd.EVAL_RESNET, games, res_blocks=6, filters=64)
    ev.load_state_dict(tensors)
    kw = dict(rollouts=rollouts, noise_plies=80, exploit_plies=40, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0)
    e.selfplay_create(games, arena_nodes=1 << 16, seed=0, max_examples=1 << 14, **kw)
    sp = orc.SelfPlay(5, games, head=orc.HEAD_FC5, py_eval=lambda st: ev.policy_eval(st), seed=0, **kw)
    for step in range(plies):
        e.selfplay_step(1)
        sp.step(1)
        a, b = e.selfplay_stats(), sp.stats()
        assert a == b, (step, a, b)
    assert a["expansions"] >= games * rollouts * (plies - 2)
    gh, gs, gm, gv = e.selfplay_drain(1 << 14)
    oh, os_, om, ov = sp.drain(1 << 14)
    assert np.array_equal(gh, oh) and np.array_equal(gs, os_) and np.array_equal(gm, om) and np.array_equal(gv, ov)
    # the live roots agree too (visit counts of every legal move of every game)
    st_o, alive_o = sp.states()
    assert np.array_equal(e.search_states(), st_o)
    e.close()
    ev.close()


def test_the_references_own_constants_net6_32_games(orc):
    """`extra.reference_constants` of the bench line (round 6): 6×6, 32 lock-step games, `Net6` = 16 blocks × 128 filters, conv head
    (train/src/self_play.rs:10-12,94; alpha-tak/src/model/net6.rs:16-17) — the width at which every network kernel is the small-batch
    form (k_tower_split: a position over 8 workgroups; k_conv_split).  Parity at that width: the forward of the 32 leaves against PyTorch
    fp32 (≤ 1e-4), whole trees after 150 iterations bit for bit against the oracle's MCTS — whose evaluator is ANOTHER engine that sees
    every leaf batch padded to 300 positions, i.e. through the one-workgroup-per-position tower — and three plies of the self-play driver
    (opening, noise, sampling, tree reuse) against the oracle's, statistic for statistic and example for example."""
    import tak_amd

    n, games, blocks, filters = 6, 32, 16, 128
    net = torch_ref.make_net(n, blocks, filters, "conv", seed=6, randomize_bn=True)
    tensors = torch_ref.abi_tensors(net)
    e = _mk(n, tak_amd.EVAL_RESNET, games, res_blocks=blocks, filters=filters)
    e.load_state_dict(tensors)
    ev = _mk(n, tak_amd.EVAL_RESNET, 512, res_blocks=blocks, filters=filters)
    ev.load_state_dict(tensors)
    sts = _roots(orc, n, games, seed=31, max_plies=40)
    pad = np.concatenate([sts] * 10)[:300 - games]

    def padded_eval(st):  # the same positions inside a 300-position batch: k_tower<3,8>, not the split tower
        k = len(st)
        p, v = ev.policy_eval(np.concatenate([st, pad[: 300 - k]]))
        return p[:k], v[:k]

    p, v = e.policy_eval(sts)
    p_ref, v_ref = torch_ref.forward(net, orc.encode(n, sts))
    assert np.abs(p - p_ref).max() <= 1e-4 and np.abs(v - v_ref).max() <= 1e-4
    torch_ref.report("reference constants Net6, 32 games", torch_ref.check_forward(p, v, torch_ref.forward64(net, orc.encode(n, sts)), "f32", "Net6 32 games"))
    p2, v2 = padded_eval(sts)
    assert np.array_equal(p, p2) and np.array_equal(v, v2)
    e.search_create(games, arena_nodes=1 << 15, seed=2)
    e.search_reset(sts)
    e.search_run(150)
    s = orc.Search(n, head=orc.HEAD_CONV, py_eval=padded_eval, seed=2)
    s.reset(sts)
    s.run(150)
    _assert_same_trees(e, s, games)
    kw = dict(rollouts=60, noise_plies=80, exploit_plies=40, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0)
    e.selfplay_create(games, arena_nodes=1 << 15, seed=7, max_examples=1 << 12, **kw)
    sp = orc.SelfPlay(n, games, head=orc.HEAD_CONV, py_eval=padded_eval, seed=7, **kw)
    for step in range(3):
        e.selfplay_step(1)
        sp.step(1)
        assert e.selfplay_stats() == sp.stats(), step
    assert np.array_equal(e.search_states(), sp.states()[0])
    e.close()
    ev.close()


@pytest.mark.parametrize("n,games,rollouts,total", [(4, 8, 24, 20), (5, 6, 16, 9), (5, 64, 100, 80), (6, 8, 24, 14), (6, 16, 48, 24)])
def test_selfplay_driver_matches_oracle(orc, n, games, rollouts, total):
    # self_play_parallel end to end: openings, instant wins, noise, rollouts, sampling / argmax,
    # tree reuse, game recycling and example emission — every example identical, in the same order
    import tak_amd

    # the last case is BASELINE config C1 (5×5, 64 games, 100 sims/move) with the reference's noise / temperature schedule
    c1 = games == 64
    kw = dict(rollouts=rollouts, noise_plies=80 if c1 else 6, exploit_plies=40 if c1 else 4, noise_alpha=0.2, noise_ratio=0.3, komi=2,
              total_games=total)
    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.selfplay_create(games, arena_nodes=1 << 16 if c1 else 1 << 15, seed=5, max_examples=1 << 14, **kw)
    head = orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV
    sp = orc.SelfPlay(n, games, head=head, evaluator=orc.EVAL_HASH, seed=5, **kw)
    for step in range(1500):  # whole games, to completion (6×6 games under a pseudo-random evaluator run long)
        e.selfplay_step(1)
        sp.step(1)
        a, b = e.selfplay_stats(), sp.stats()
        assert a == b, (step, a, b)
        if not sp.states()[1].any():
            break
    assert not sp.states()[1].any(), "games still running"
    assert b["games_finished"] >= total - games + 1 and b["examples"] > 0
    gh, gs, gm, gv = e.selfplay_drain(1 << 14)
    oh, os_, om, ov = sp.drain(1 << 14)
    assert len(gh) == len(oh) == b["examples"]
    assert np.array_equal(gh, oh)
    assert np.array_equal(gs, os_) and np.array_equal(gm, om) and np.array_equal(gv, ov)
    e.close()


def test_examples_written_in_reference_text_format(orc, tmp_path):
    # alpha-tak/src/example.rs:81-133: drained GPU examples → `.data` lines → parsed back
    import tak_amd

    n, games = 4, 6
    kw = dict(rollouts=10, noise_plies=6, exploit_plies=4, total_games=8)
    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.selfplay_create(games, arena_nodes=1 << 14, seed=12, max_examples=1 << 12, **kw)
    e.selfplay_step(120)
    path = tmp_path / "0.data"
    wrote = e.write_examples(str(path))
    assert wrote == e.selfplay_stats()["examples"] > 0
    sp = orc.SelfPlay(n, games, evaluator=orc.EVAL_HASH, seed=12, **kw)
    sp.step(120)
    oh, os_, om, ov = sp.drain(1 << 12)
    lines = path.read_text().splitlines()
    assert len(lines) == len(oh)
    for i, line in enumerate(lines):
        st, mv, vs, res = tak_amd.parse_example(n, line)
        k = int(oh["n_moves"][i])
        want = os_[i].copy()
        want[256 - 16 + 9] = 0
        assert np.array_equal(st, want) and np.array_equal(mv, om[i, :k]) and np.array_equal(vs, ov[i, :k]) and res == oh["result"][i]
    e.close()


def test_arena_auto_sizing(orc):
    """arena_nodes = 0: the engine sizes the node pool from the free device memory (up to 2^20 nodes per game) — a search that
    exhausts a pool of 2^10 nodes per game runs through"""
    import tak_amd

    e = _mk(5, tak_amd.EVAL_HASH, 8)
    sts = _roots(orc, 5, 8, seed=2, max_plies=10)
    e.search_create(8, arena_nodes=1024)
    e.search_reset(sts)
    with pytest.raises(tak_amd.TgError):
        e.search_run(400)
        e.search_root()
    e.search_create(8, arena_nodes=0)
    e.search_reset(sts)
    e.search_run(400)
    assert (e.search_root()["root_visits"] == 400).all()
    e.close()


def test_states_no_game_can_reach_are_refused(orc):
    """tg_search_reset validates caller-supplied states on the host: the tree kernels size child arrays from a state's
    move count, so garbage is an argument error, not something to explore"""
    import tak_amd

    e = _mk(5, tak_amd.EVAL_HASH, 4)
    e.search_create(4, arena_nodes=1 << 12)
    good = _roots(orc, 5, 4, seed=1, max_plies=20)
    e.search_reset(good)
    hdr = 256 - 16
    cases = []
    bad = good.copy(); bad[1, hdr + 0] = 6; cases.append(bad)                      # another board size
    bad = good.copy(); bad[2, 200 + 3] = 63 | (2 << 6); cases.append(bad)           # a 63-high stack on 5×5
    bad = good.copy(); bad[0, hdr + 4] = 200; cases.append(bad)                     # 200 stones in reserve
    bad = good.copy(); bad[3, 200:225] = 0; bad[3, 0:8] = 255; cases.append(bad)    # colour bits on an empty square
    bad = good.copy(); bad[0, hdr + 1] = 7; cases.append(bad)                       # to_move = 7
    rng = np.random.default_rng(0)
    bad = rng.integers(0, 256, good.shape, dtype=np.uint8); cases.append(bad)       # noise
    for bad in cases:
        with pytest.raises(tak_amd.TgError) as ei:
            e.search_reset(bad)
        assert ei.value.code == -1 and "is not a position" in str(ei.value)
    e.search_reset(good)  # the engine is still usable
    e.search_run(20)
    assert (e.search_root()["root_visits"] == 20).all()
    e.close()


def _parse_tree(rec):
    """pre-order dump → children index lists (an uninitialised child is one record with n_children = 0xFFFF)"""
    kids = [[] for _ in range(len(rec))]
    pos = [0]

    def walk():
        me = pos[0]
        pos[0] += 1
        if rec["n_children"][me] == 0xFFFF:
            return
        for _ in range(int(rec["n_children"][me])):
            kids[me].append(pos[0])
            walk()

    walk()
    assert pos[0] == len(rec)
    return kids


def _ucb(rec, ch, node, base=500.0, init=4.0):
    """upper confidence bounds of `node`'s children (mcts.rs:94-118), f32"""
    f32 = np.float32
    prior = rec["prior_bits"].view(np.float32)
    q = rec["q_bits"].view(np.float32)
    ns = f32(int(rec["visits"][node]) + int(rec["virtual_visits"][node]))
    c = f32(np.log(f32((f32(1.0) + ns + f32(base)) / f32(base)))) + f32(init)
    cv, cvirt = rec["visits"][ch].astype(np.float32), rec["virtual_visits"][ch].astype(np.float32)
    cn = cv + cvirt
    qv = np.where(cn > 0, (q[ch] * cv - cvirt) / np.maximum(cn, f32(1)), f32(0)).astype(np.float32)
    return (qv + c * prior[ch] * (np.sqrt(ns) / (f32(1) + cn))).astype(np.float32)


def _closest_call(rec, other, kids):
    """Along the path the NEXT rollout descends in `rec`'s tree: the smallest (top-2 gap of the upper confidence bounds) ÷
    (largest difference between the two sides' bounds at that node) — how many times wider the decision was than the
    numerical disagreement of the two networks.  `other` is the same tree (same structure) with the other side's numbers."""
    node, worst = 0, np.inf
    while True:
        vis, virt = int(rec["visits"][node]), int(rec["virtual_visits"][node])
        if (vis == 0 and virt == 0) or rec["n_children"][node] == 0xFFFF or rec["result"][node] != 0 or not kids[node]:
            return worst
        ch = np.array(kids[node])
        u, v = _ucb(rec, ch, node), _ucb(other, ch, node)
        if len(ch) > 1:
            top = np.sort(u)
            noise = max(float(np.abs(u - v).max()), 1e-7)
            worst = min(worst, float(top[-1] - top[-2]) / noise)
        node = int(ch[len(ch) - 1 - int(np.argmax(u[::-1]))])  # max_by keeps the last maximum


def test_end_to_end_against_oracle_mcts_with_the_pytorch_network(orc):
    """No GPU code on the reference side: the oracle's MCTS evaluates its leaves with PyTorch-CPU fp32 (the ATen ops tch-rs
    calls), the engine runs its own search on its own network kernels.  The two networks agree to ≤ 1e-4, not to the bit, so
    a selection whose two best upper confidence bounds are closer than the two sides' numbers disagree may legitimately go
    either way.  Trees must be identical — same nodes, same moves, same visit counts, same results; priors and values within
    1e-4 — for as long as every selection made so far was at least 4 times wider than that disagreement (measured per node
    from both trees; with random-init weights priors are nearly flat and a fixed margin such as 1e-3 would exclude almost
    every selection, so the margin is relative to the observed noise).  A closer call is reported and ends the strict
    comparison for that game only."""
    import torch

    import tak_amd

    n, blocks, filters, games, iters = 5, 2, 32, 8, 50
    net = torch_ref.make_net(n, blocks, filters, "fc5", seed=6)
    with torch.no_grad():  # a trained network's policy is peaked, a fresh one's is flat: sharpen it so selections are decisions
        net.policy.weight *= 20
        net.value.weight *= 4
    e = _mk(n, tak_amd.EVAL_RESNET, games, res_blocks=blocks, filters=filters)
    e.load_state_dict(torch_ref.abi_tensors(net))
    e.search_create(games, arena_nodes=1 << 14)
    s = orc.Search(n, head=orc.HEAD_FC5, py_eval=lambda st: torch_ref.forward(net, orc.encode(n, st)))
    sts = _roots(orc, n, games, seed=12, max_plies=24)
    e.search_reset(sts)
    s.reset(sts)
    strict = np.ones(games, bool)
    close_calls = []
    compared = 0
    for it in range(iters):
        for g in np.nonzero(strict)[0]:
            a, b = e.search_dump(int(g)), s.dump(int(g))
            ratio = _closest_call(b, a, _parse_tree(b))
            if ratio < 4.0:
                strict[g] = False
                close_calls.append((int(g), it, round(ratio, 2)))
        e.search_run(1)
        s.run(1)
        for g in np.nonzero(strict)[0]:
            a, b = e.search_dump(int(g)), s.dump(int(g))
            assert len(a) == len(b), f"game {g}, iteration {it}: {len(a)} nodes against {len(b)}"
            for f in ("move", "n_children", "visits", "virtual_visits", "result"):
                assert np.array_equal(a[f], b[f]), f"game {g}, iteration {it}: {f} differs (first at node {int(np.argmax(a[f] != b[f]))})"
            pa, pb = a["prior_bits"].view(np.float32), b["prior_bits"].view(np.float32)
            qa, qb = a["q_bits"].view(np.float32), b["q_bits"].view(np.float32)
            assert np.abs(pa - pb).max() <= 1e-4 and np.abs(qa - qb).max() <= 1e-4, (g, it)
            compared += 1
    print(f"end-to-end: {compared} (game, iteration) trees identical; close calls (game, iteration, margin / noise): {close_calls}")
    # (measured: every game stays in strict comparison for the first 30 iterations; with 45 nearly unvisited children per node
    # a decision as narrow as the two networks' disagreement turns up in most games somewhere between iterations 30 and 50)
    assert compared >= games * iters // 2, close_calls
    e.close()
