"""tg_search_debug (Node::debug on the device) against tests/debug_ref.py over tree dumps — the oracle's and the GPU's own — and
Player's analysis end to end.  Floats compare as bits."""
import numpy as np
import pytest

import torch_ref
from debug_ref import assert_same, debug_ref, parse
from search_helpers import _best, _mk, _roots

pytestmark = pytest.mark.gpu

SCRATCH = 1 << 26  # TG_DEBUG_SCRATCH_BYTES


def _check_against(e, dump, games, grid=((0, 0), (0, 3), (1, 3), (10, 512), (1, 512), (10, 0), (0, 512), (10, 3))):
    trees = [parse(dump(g)) for g in games]
    for depth, top_k in grid:
        r = e.search_debug(depth, top_k)
        assert r["cont_moves"].shape == (e.games, top_k, depth)
        for g, t in zip(games, trees):
            assert_same(r, g, debug_ref(t, depth, top_k))


@pytest.mark.parametrize("n,games,iters", [(5, 24, 300), (6, 12, 200), (4, 16, 300)])
def test_hash_evaluator_against_the_oracle(orc, n, games, iters):
    import tak_amd

    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.search_create(games, arena_nodes=1 << 16, seed=99)
    s = orc.Search(n, head=orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV, evaluator=orc.EVAL_HASH, seed=99)
    sts = _roots(orc, n, games, seed=n, max_plies=40 if n >= 5 else 16)
    e.search_reset(sts)
    s.reset(sts)
    e.search_run(iters)
    s.run(iters)
    _check_against(e, s.dump, range(games))
    e.search_apply_dirichlet(0.2, 0.3)
    s.apply_dirichlet(0.2, 0.3)
    e.search_run(40)
    s.run(40)
    _check_against(e, s.dump, range(games))
    r = e.search_root()
    mv = np.array([_best(r, g) for g in range(games)], np.uint16)
    nxt, _ = orc.play(n, e.search_states(), mv)
    act = (orc.result(n, nxt) == 0).astype(np.uint8)
    e.search_play(mv, act)
    s.play(mv, act)
    _check_against(e, s.dump, range(games))  # the re-rooted trees before any new iteration
    e.search_run(30, act)
    s.run(30, act)
    _check_against(e, s.dump, range(games))
    e.close()


@pytest.mark.parametrize("n", [3, 5])
def test_dummynet_mass_ties(orc, n):
    # uniform priors and eval 0: many children share a visit count, at the root and inside the continuations
    import tak_amd

    games = 4
    e = _mk(n, tak_amd.EVAL_DUMMY, games)
    e.search_create(games, arena_nodes=1 << 15)
    s = orc.Search(n, head=orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV, evaluator=orc.EVAL_DUMMY)
    sts = _roots(orc, n, games, seed=3, max_plies=4)
    e.search_reset(sts)
    s.reset(sts)
    for iters in (1, 7, 200):
        e.search_run(iters)
        s.run(iters)
        _check_against(e, s.dump, range(games))
        if iters == 1:  # an expanded root whose children all have 0 visits: one tie over all of them, eval NaN
            r = e.search_debug(10, 512)
            assert (r["visits"][:, 0] == r["visits"][:, 1]).all() and np.isnan(r["eval"]).all()
    e.close()


@pytest.mark.parametrize("n,blocks,filters,head", [(5, 2, 64, "fc5"), (6, 1, 32, "conv")])
def test_player_debug_with_a_trained_like_network(orc, n, blocks, filters, head):
    import posgen

    import tak_amd

    planes = orc.encode(n, posgen.distinct_positions(orc, n, 256, seed=41, max_plies=60))
    net = torch_ref.make_trained_net(n, blocks, filters, head, planes, seed=41)
    tensors = torch_ref.abi_tensors(net)
    h = tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV
    e = _mk(n, tak_amd.EVAL_RESNET, 16, head=h, res_blocks=blocks, filters=filters)
    e.load_state_dict(tensors)
    ev = _mk(n, tak_amd.EVAL_RESNET, 16, head=h, res_blocks=blocks, filters=filters)
    ev.load_state_dict(tensors)
    game = _roots(orc, n, 1, seed=8, max_plies=20)[0]
    p = tak_amd.Player(e, batch=16, save_examples=False, game=game)
    s = orc.Search(n, head=orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV, py_eval=lambda st: ev.policy_eval(st), batch=16)
    s.reset(game[None])
    s.run(1)
    for ply in range(3):
        for _ in range(6):
            p.rollout()
        s.run(6)
        info = p.debug(10)
        r = e.search_debug(10, 512)
        for dump in (e.search_dump(0), s.dump(0)):
            ref = debug_ref(dump, 10, 512)
            assert_same(r, 0, ref)
        assert [i.mov for i in info] == [int(m) for m in ref["moves"][: ref["counts"]]]
        assert [i.continuation for i in info][:3] == [
            [(int(m), int(v)) for m, v in zip(ref["cont_moves"][j, : ref["cont_len"][j]], ref["cont_visits"][j, : ref["cont_len"][j]])]
            for j in range(min(3, int(ref["counts"])))]
        mv = p.pick_move(True)
        p.play_move(mv)
        s.play([mv])
        s.run(1)
    e.close()
    ev.close()


def test_width_4096_games_and_prefix(orc):
    import tak_amd

    n, games = 5, 4096
    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.search_create(games, arena_nodes=1 << 15)
    e.search_reset(_roots(orc, n, games, seed=77, max_plies=30))
    e.search_run(400)
    sample = np.random.default_rng(0).choice(games, 64, replace=False)
    trees = {int(g): parse(e.search_dump(int(g))) for g in sample}
    r = e.search_debug(10, 10)
    for g, t in trees.items():
        assert_same(r, g, debug_ref(t, 10, 10))
    # (depth 10, top_k 5) is a prefix of (depth 20, top_k 512), row for row
    a, b = e.search_debug(10, 5), e.search_debug(20, 512)
    for k in ("moves", "visits", "reward", "policy", "counts", "eval"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert np.array_equal(a["cont_moves"], b["cont_moves"][:, :5, :10])
    assert np.array_equal(a["cont_visits"], b["cont_visits"][:, :5, :10])
    assert np.array_equal(a["cont_len"], np.minimum(b["cont_len"][:, :5], 10))
    e.close()


def test_width_16384_games_across_scratch_slices(orc):
    import tak_amd

    n, games, depth, top_k = 5, 16384, 10, 64
    per_game = 512 * 14 + 8 + top_k * depth * 6 + top_k * 4  # tg_search_debug's scratch per game
    slice_ = SCRATCH // per_game
    assert slice_ < games
    e = _mk(n, tak_amd.EVAL_HASH, games)
    e.search_create(games, arena_nodes=1 << 12)
    e.search_reset(_roots(orc, n, games, seed=78, max_plies=30))
    e.search_run(40)
    r = e.search_debug(depth, top_k)
    edges = sorted({0, games - 1} | {x for b in range(slice_, games, slice_) for x in (b - 1, b)})
    for g in edges:
        assert_same(r, g, debug_ref(e.search_dump(g), depth, top_k))
    assert (r["counts"] > 0).all()
    e.close()


def test_edges(orc):
    import tak_amd
    from tak_amd.engine import TgError, _p

    n = 5
    e = _mk(n, tak_amd.EVAL_HASH, 4)
    # before a search exists: the status tg_search_root gives
    rc_root = e.lib.tg_search_root(e.h, *([None] * 7))
    assert rc_root < 0 and e.lib.tg_search_debug(e.h, 10, 10, *([None] * 9)) == rc_root
    e.search_create(4, arena_nodes=1 << 14)
    # terminal roots and roots one move from the end
    import posgen

    d = posgen.terminal_mix(orc, n, per_style=20, seed=5)
    sts = np.concatenate([d["final"][:2], d["prev"][:2]])
    e.search_reset(sts)
    r = e.search_debug(10, 512)
    assert (r["counts"] == 0).all() and not r["eval"].view(np.uint32).any()  # fresh trees: no children, eval +0.0
    s = orc.Search(n, head=orc.HEAD_FC5, evaluator=orc.EVAL_HASH)
    s.reset(sts)
    e.search_run(50)
    s.run(50)
    _check_against(e, s.dump, range(4))
    r = e.search_debug(10, 512)
    assert (r["counts"][:2] == 0).all() and not r["eval"][:2].view(np.uint32).any()
    # argument ranges
    for depth, top_k in ((-1, 3), (65, 3), (3, -1), (3, 513)):
        with pytest.raises(TgError) as err:
            e.search_debug(depth, top_k)
        assert err.value.code == -1  # TG_ERR_INVALID_ARG
    e.search_debug(64, 512)
    # NULL outputs are accepted, one at a time and all at once
    full = e.search_debug(4, 7)
    lib = e.lib
    assert lib.tg_search_debug(e.h, 4, 7, *([None] * 9)) == 0
    counts = np.zeros(4, np.int32)
    cl = np.zeros((4, 7), np.int32)
    assert lib.tg_search_debug(e.h, 4, 7, None, None, None, None, _p(counts), None, None, None, _p(cl)) == 0
    assert np.array_equal(counts, full["counts"]) and np.array_equal(cl, full["cont_len"])
    e.close()


def _ref_analysis(n, game, dumps, plays):
    from tak_amd.analysis import Analysis, NodeDebugInfo

    sb = len(game)
    a = Analysis(n, int(game[sb - 16 + 8:sb - 16 + 9].view(np.int8)[0]), int(game[sb - 14:sb - 12].view("<u2")[0]))
    for dump, (mv, with_info) in zip(dumps, plays):
        if with_info:
            r = debug_ref(dump, 10, 512)
            info = NodeDebugInfo.from_search_debug(n, {k: np.asarray(v)[None] for k, v in r.items()}, 0)
            a.update(info, mv)
        else:
            a.add_move_without_info(mv)
    return a


@pytest.mark.parametrize("opening", [[], ["a1"]])
def test_player_analysis_end_to_end(orc, opening):
    import re

    import tak_amd

    n, batch = 4, 8
    e = _mk(n, tak_amd.EVAL_HASH, batch, head=tak_amd.HEAD_CONV)
    game = orc.from_ptn(n, opening, half_komi=-3 if opening else 4)
    p = tak_amd.Player(e, batch=batch, save_examples=False, game=game, create_analysis=True)
    s = orc.Search(n, head=orc.HEAD_CONV, evaluator=orc.EVAL_HASH, batch=batch)
    s.reset(game[None])
    s.run(1)
    dumps, plays = [], []
    st = game
    for ply in range(12):
        if orc.result(n, st)[0] != 0:
            break
        for _ in range(4):
            p.rollout()
        s.run(4)
        mv = p.pick_move(True)
        with_info = ply % 3 != 2
        dumps.append(s.dump(0))
        plays.append((mv, with_info))
        p.play_move(mv, with_info=with_info)
        s.play([mv])
        s.run(1)
        st = orc.play(n, st, [mv])[0][0]
    text = str(p.get_analysis())
    assert text == str(_ref_analysis(n, game, dumps, plays))
    assert text.startswith(f'[Size "{n}"]\n[Komi "{"-1.5" if opening else "2"}"]\n')
    assert text.split("\n")[2].startswith("1. -- ") == bool(opening)
    # every move of the main line parses back to the move played
    main = text.split("\n\n")[0].split("\n")[2:]
    toks = [t for ln in main for t in re.sub(r"\{[^}]*\}", " ", ln).split()[1:] if t != "--"]
    toks = [t.rstrip("?!") for t in toks]
    assert [tak_amd.parse_move(n, t) for t in toks] == [mv for mv, _ in plays]
    assert str(p.get_analysis()) == ""  # taken: the Player keeps an empty default one
    e.close()
