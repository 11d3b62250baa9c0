"""The example window on the GPU (tg_window_*, the `examples` of training_loop, train/src/main.rs:26,56-123): what enters it is what
tg_selfplay_drain would have handed to the host, what leaves it trains the network to the bits tg_train reaches on the same examples.

Twin engines with the same seed play identical games (TG_EVAL_HASH needs no network), so one of them can drain where the other
absorbs.  The training case's shapes and the teeth of its comparison are in tests/window_ref.py and tests/test_window_ring.py."""
import numpy as np
import pytest

import eval_examples_ref as ref
import torch_ref
import window_ref as wr

pytestmark = pytest.mark.gpu

SP = dict(rollouts=8, noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0)  # endless
GAMES = 6
PARTS = ("hdr", "states", "moves", "visits")


def _hash_engine(n, seed, max_examples=1 << 12, **kw):
    import tak_amd

    e = tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=64)
    e.selfplay_create(GAMES, arena_nodes=1 << 14, seed=seed, max_examples=max_examples, **{**SP, **kw})
    return e


def _empty(e):
    import tak_amd

    return [np.zeros(0, tak_amd.engine.EXAMPLE_HEADER), np.zeros((0, e.sb), np.uint8), np.zeros((0, 512), np.uint16), np.zeros((0, 512), np.uint32)]


def _cat(a, b):
    return [np.concatenate([x, y]) for x, y in zip(a, b)]


def _tail(parts, k):
    return [p[len(p) - k:] for p in parts]


def _assert_same_examples(got, want, what=""):
    """field for field: game_id, n_moves, result, reserved (the header's 16 bytes), state bytes, all 512 moves and visits of every
    row — the zeros past n_moves are part of the comparison"""
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    for f in ("game_id", "n_moves", "result", "reserved"):
        assert np.array_equal(got[0][f], want[0][f]), (what, f)
    for name, a, b in zip(PARTS[1:], got[1:], want[1:]):
        assert a.shape == b.shape and np.array_equal(a, b), (what, name)
    nm = want[0]["n_moves"]
    past = np.arange(512)[None, :] >= nm[:, None]
    assert not got[2][past].any() and not got[3][past].any(), what


# ---- 1. absorb = drain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 6])
def test_absorb_is_drain(n):
    cap = 37
    a, b = _hash_engine(n, seed=7), _hash_engine(n, seed=7)
    b.window_create(cap)
    drained, absorbed = _empty(a), 0
    for _ in range(120):
        a.selfplay_step(3)
        b.selfplay_step(3)
        drained = _cat(drained, a.selfplay_drain(1 << 12))
        absorbed += b.window_absorb()
        if len(drained[0]) >= 3 * cap:
            break
    total = len(drained[0])
    assert total >= 3 * cap, total  # the window has wrapped at least twice
    assert absorbed == total
    assert b.window_info() == {"capacity": cap, "count": cap, "entered": total, "evicted": total - cap}
    _assert_same_examples(b.window_read(0, cap), _tail(drained, cap), f"{n}x{n}")
    assert (drained[0]["n_moves"] < 512).all() and len(set(drained[0]["game_id"].tolist())) >= 2  # short rows, more than one game
    # a part of it, from the middle
    _assert_same_examples(b.window_read(5, 20), [p[total - cap + 5: total - cap + 25] for p in drained], "middle")
    assert b.selfplay_stats() == a.selfplay_stats()
    a.close()
    b.close()


# ---- 2. one absorb larger than the window ----------------------------------------------------------------------------------------
def test_one_absorb_larger_than_the_window_keeps_the_newest():
    cap = 11
    a, b = _hash_engine(5, seed=9), _hash_engine(5, seed=9)
    b.window_create(cap)
    for _ in range(120):
        a.selfplay_step(3)
        b.selfplay_step(3)
        if b.selfplay_stats()["examples"] > cap:
            break
    waiting = b.selfplay_stats()["examples"]
    assert waiting > cap
    assert b.window_absorb() == waiting
    want = a.selfplay_drain(1 << 12)
    assert len(want[0]) == waiting
    assert b.window_info() == {"capacity": cap, "count": cap, "entered": waiting, "evicted": waiting - cap}
    _assert_same_examples(b.window_read(0, cap), _tail(want, cap))
    assert b.window_absorb() == 0 and b.window_info()["entered"] == waiting  # nothing enters twice
    # … and into a window that already holds some, at a row that is not 0: again more than it holds
    for _ in range(120):
        a.selfplay_step(3)
        b.selfplay_step(3)
        if b.selfplay_stats()["examples"] - waiting > cap:
            break
    more = a.selfplay_drain(1 << 12)
    assert len(more[0]) > cap and b.window_absorb() == len(more[0])
    _assert_same_examples(b.window_read(0, cap), _tail(more, cap), "second")
    assert b.window_info()["evicted"] == waiting + len(more[0]) - cap
    a.close()
    b.close()


# ---- 3. ring overrun -------------------------------------------------------------------------------------------------------------
def test_ring_overrun_leaves_absorb_and_drain_the_same_survivors():
    """A ring of 8 is overwritten by every game that ends (a game stages one example per ply).  Visits every 8 plies: absorb and drain
    skip the same overwritten examples, count them the same, and hand on the same survivors.  One wave per game writes the ring, so
    when TWO games end in the same ply and overrun it together, which of them wrote a row last is not defined — for drain as for
    absorb; the survivors of such a visit are compared by number only, and at least two overrun visits without one must be seen."""
    ring, cap = 8, 64
    a, b = _hash_engine(5, seed=11, max_examples=ring), _hash_engine(5, seed=11, max_examples=ring)
    b.window_create(cap)
    received, dropped, clean_overruns = 0, 0, 0
    for _ in range(80):
        two_at_once = False
        for _ in range(8):
            finished = a.selfplay_stats()["games_finished"]
            a.selfplay_step(1)
            b.selfplay_step(1)
            two_at_once |= a.selfplay_stats()["games_finished"] - finished > 1
        part = a.selfplay_drain(1 << 10)
        k = b.window_absorb()
        assert k == len(part[0]) <= ring
        received += k
        sa, sb = a.selfplay_stats(), b.selfplay_stats()
        assert sa == sb and sa["examples"] == sa["dropped_examples"] + received
        info = b.window_info()
        assert info["entered"] == received and info["count"] == min(received, cap)
        if not two_at_once:
            _assert_same_examples(b.window_read(info["count"] - k, k), part)
            clean_overruns += sa["dropped_examples"] > dropped
        dropped = sa["dropped_examples"]
        if clean_overruns >= 2:
            break
    assert clean_overruns >= 2 and dropped > 0, (clean_overruns, dropped)
    a.close()
    b.close()


# ---- 4. mixed cursor -------------------------------------------------------------------------------------------------------------
def test_drain_and_absorb_share_one_cursor():
    m, t = _hash_engine(5, seed=13), _hash_engine(5, seed=13)
    m.window_create(1 << 10)
    merged, full, seen = _empty(m), _empty(t), 0
    sources = set()
    for i in range(60):
        m.selfplay_step(3)
        t.selfplay_step(3)
        full = _cat(full, t.selfplay_drain(1 << 12))
        part = m.selfplay_drain(5)  # at most five go to the host …
        merged = _cat(merged, part)
        if len(part[0]):
            sources.add("drain")
        k = m.window_absorb()       # … the rest of what has finished to the window
        if k:
            sources.add("absorb")
            merged = _cat(merged, m.window_read(seen, k))
            seen += k
        if i % 2:                   # and the other way round: absorb first leaves the drain nothing
            assert m.window_absorb() == 0 and len(m.selfplay_drain(5)[0]) == 0
        if len(full[0]) >= 80 and sources == {"drain", "absorb"}:
            break
    assert len(full[0]) >= 80 and sources == {"drain", "absorb"}
    assert m.window_info()["entered"] == seen and 0 < seen < len(full[0])
    _assert_same_examples(merged, full)
    assert m.selfplay_stats()["dropped_examples"] == 0
    m.close()
    t.close()


# ---- 5. push and read ------------------------------------------------------------------------------------------------------------
def _as_parts(ex, ids):
    import tak_amd

    hdr = np.zeros(len(ids), tak_amd.engine.EXAMPLE_HEADER)
    hdr["game_id"], hdr["n_moves"], hdr["result"] = ids, ex["n_moves"], ex["results"]
    return [hdr, ex["states"], ex["moves"], ex["visits"]]


def test_push_wraps_and_read_returns_canonical_rows(orc):
    import tak_amd

    cap, total = 7, 40
    ex = ref.make_examples(orc, 5, total, seed=3)
    dirty = {k: v.copy() for k, v in ex.items()}
    past = np.arange(512)[None, :] >= ex["n_moves"][:, None]
    dirty["moves"][past], dirty["visits"][past] = 0xBEEF, 0xDEADBEEF  # what a caller's buffers may hold past n_moves
    ids = np.arange(1000, 1000 + total, dtype=np.int32)
    want = _as_parts(wr.canonical(ex), ids)
    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64)
    e.window_create(cap)
    assert e.window_info() == {"capacity": cap, "count": 0, "entered": 0, "evicted": 0}
    assert len(e.window_read(0, 0)[0]) == 0
    done = 0
    for k in (3, 5, 0, 4, 6, 7, 2, 9, 4):  # wraps three times at every offset; 7 = a whole window, 9 = more than one
        sel = slice(done, done + k)
        e.window_push(*ref.args(ref.take(dirty, sel)), game_ids=ids[sel])
        done += k
        info = e.window_info()
        assert info == {"capacity": cap, "count": min(done, cap), "entered": done, "evicted": done - min(done, cap)}
        _assert_same_examples(e.window_read(0, info["count"]), [p[done - info["count"]:done] for p in want], f"after {done}")
    assert done == total and done >= 3 * cap
    e.window_push(*ref.args(ref.take(ex, slice(0, 2))))  # game_ids = NULL: zeros
    assert e.window_read(cap - 2, 2)[0]["game_id"].tolist() == [0, 0]
    before = e.window_read(0, cap)
    # one bad example among good ones: refused as a whole, the index named, the window as it was
    for index, spoil, why in [(3, "visits", "without visits"), (0, "n_moves", "n_moves"), (4, "state", "not a position"), (2, "n_moves_big", "n_moves")]:
        bad = ref.take({k: v.copy() for k, v in ex.items()}, slice(10, 16))
        if spoil == "visits":
            bad["visits"][index] = 0
        elif spoil == "n_moves":
            bad["n_moves"][index] = 0
        elif spoil == "n_moves_big":
            bad["n_moves"][index] = 513
        else:
            bad["states"][index, 256 - 16] = 6  # TgHeader.n: a 6x6 state handed to a 5x5 engine
        with pytest.raises(tak_amd.TgError) as ei:
            e.window_push(*ref.args(bad))
        assert ei.value.code == -1 and f"example {index} " in str(ei.value) and why in str(ei.value), str(ei.value)
        assert e.window_info()["entered"] == total + 2
        _assert_same_examples(e.window_read(0, cap), before, spoil)
    e.window_clear()
    assert e.window_info() == {"capacity": cap, "count": 0, "entered": 0, "evicted": 0}
    e.window_push(*ref.args(ref.take(ex, slice(0, 3))))
    _assert_same_examples(e.window_read(0, 3), [p[:3] for p in _as_parts(wr.canonical(ex), np.zeros(total, np.int32))], "after clear")
    e.close()


# ---- 6. train = tg_train ---------------------------------------------------------------------------------------------------------
def _net_engine(name):
    import tak_amd

    net, n, blocks, filters, head = ref.golden_net(name)
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                       evaluator=tak_amd.EVAL_RESNET, max_batch=64)
    e.load_state_dict(torch_ref.abi_tensors(net))
    return e, n, tak_amd.tensor_shapes(n, blocks, filters, e.head)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _assert_same_training(w, t, got, want, shapes, what):
    assert got[2] == want[2], (what, got, want)
    assert _bits(got[0]) == _bits(want[0]) and _bits(got[1]) == _bits(want[1]), (what, got, want)
    for name, shape in shapes.items():  # parameters and BatchNorm running statistics
        assert np.array_equal(_bits(w.train_get_tensor(name, shape)), _bits(t.train_get_tensor(name, shape))), (what, name)


@pytest.mark.parametrize("name", ["net5_fc_2x32", "net6_conv_1x32"])
def test_window_train_is_tg_train(orc, name):
    w, n, shapes = _net_engine(name)
    t, _, _ = _net_engine(name)
    ex = ref.make_examples(orc, n, wr.PUSHED, seed=17)
    assert len(set(ex["results"].tolist())) == 3
    for e in (w, t):
        e.train_create(chunk_size=wr.CHUNK, chunks_in_step=wr.CHUNKS_IN_STEP)
    initial = {nm: t.train_get_tensor(nm, shape) for nm, shape in shapes.items()}
    w.window_create(wr.CAPACITY)
    done = 0
    for k in wr.PUSHES:
        w.window_push(*ref.args(ref.take(ex, slice(done, done + k))))
        done += k
    info = w.window_info()
    assert info == {"capacity": wr.CAPACITY, "count": wr.CAPACITY, "entered": wr.PUSHED, "evicted": wr.PUSHED - wr.CAPACITY}
    assert info["entered"] % wr.CAPACITY == wr.HEAD  # logical 0 at row 30: [3, 40) = rows 33 … 47, 0 … 21
    before = w.window_read(0, wr.CAPACITY)
    hdr, states, moves, visits = w.window_read(wr.FIRST, wr.COUNT)
    lo = wr.PUSHED - wr.CAPACITY + wr.FIRST
    _assert_same_examples([hdr, states, moves, visits], [p[lo:lo + wr.COUNT] for p in _as_parts(wr.canonical(ex), np.zeros(wr.PUSHED, np.int32))])
    copy = (states, hdr["n_moves"], moves, visits, hdr["result"])
    # 37 examples: 4 chunks of 8 (both example sets twice, an optimiser step after the second chunk and after the fourth), 5 dropped
    got, want = w.window_train(wr.FIRST, wr.COUNT, seed=wr.SEEDS[0]), t.train(*copy, seed=wr.SEEDS[0])
    assert want[2] == 2 and want[0] > 0 and want[1] > 0
    _assert_same_training(w, t, got, want, shapes, "first call")
    assert sum(not np.array_equal(t.train_get_tensor(nm, shape), initial[nm]) for nm, shape in shapes.items()) > len(shapes) // 2  # it trained
    # fewer examples than a chunk: nothing runs, zero losses, as tg_train
    got, want = w.window_train(wr.FIRST, 7, seed=5), t.train(*[a[:7] for a in copy], seed=5)
    assert want == (0.0, 0.0, 0) and got == want
    _assert_same_training(w, t, got, want, shapes, "no chunk")
    # a second call, another seed: a fresh optimiser on both
    got, want = w.window_train(wr.FIRST, wr.COUNT, seed=wr.SEEDS[1]), t.train(*copy, seed=wr.SEEDS[1])
    _assert_same_training(w, t, got, want, shapes, "second call")
    # the whole window, from logical 0: 6 chunks, both runs of the ring in one call
    whole = w.window_read(0, wr.CAPACITY)
    got = w.window_train(0, wr.CAPACITY, seed=3)
    want = t.train(whole[1], whole[0]["n_moves"], whole[2], whole[3], whole[0]["result"], seed=3)
    assert want[2] == 3
    _assert_same_training(w, t, got, want, shapes, "whole window")
    _assert_same_examples(w.window_read(0, wr.CAPACITY), before, "the window after training")
    w.close()
    t.close()


# ---- 7. lifetime and errors ------------------------------------------------------------------------------------------------------
def test_the_window_outlives_selfplay_trainers_and_commits_and_errors_leave_it_readable(orc):
    import tak_amd

    STATE, INVALID = -7, -1
    e, n, _ = _net_engine("net5_fc_2x32")

    def raises(code, fn, *a):
        with pytest.raises(tak_amd.TgError) as ei:
            fn(*a)
        assert ei.value.code == code, str(ei.value)
        return str(ei.value)

    ex = ref.make_examples(orc, n, 12, seed=4)
    # no window yet
    for fn, a in [(e.window_info, ()), (e.window_clear, ()), (e.window_absorb, ()), (e.window_push, ref.args(ex)), (e.window_read, (0, 0)),
                  (e.window_train, (0, 0))]:
        assert "tg_window_create" in raises(STATE, fn, *a)
    raises(INVALID, e.window_create, -1)
    raises(STATE, e.window_info)  # a refused create leaves no window
    e.window_create(9)
    e.window_push(*ref.args(ex))
    kept = e.window_read(0, 9)
    _assert_same_examples(kept, [p[3:] for p in _as_parts(wr.canonical(ex), np.zeros(12, np.int32))])
    info = e.window_info()

    def unchanged(what):
        assert e.window_info() == info, what
        _assert_same_examples(e.window_read(0, 9), kept, what)

    assert "tg_selfplay_create" in raises(STATE, e.window_absorb)  # no self-play
    assert "tg_train_create" in raises(STATE, e.window_train, 0, 9)  # no trainer
    unchanged("state errors")
    e.search_create(4, arena_nodes=1 << 12)
    assert "tg_selfplay_create" in raises(STATE, e.window_absorb)  # a caller-driven search is not self-play
    unchanged("search_create")
    e.selfplay_create(4, arena_nodes=1 << 12, seed=1, rollouts=4, max_examples=256)
    unchanged("selfplay_create")
    e.train_create(chunk_size=4, chunks_in_step=1)
    unchanged("train_create")
    for a in [(0, 10), (1, 9), (9, 1), (-1, 2), (0, -1), (10, 0), (2**31 - 1, 2**31 - 1)]:
        assert "[0, 9)" in raises(INVALID, e.window_read, *a)
        assert "[0, 9)" in raises(INVALID, e.window_train, *a)
    assert len(e.window_read(9, 0)[0]) == 0 and e.window_train(9, 0) == (0.0, 0.0, 0)  # the empty range at the end is inside
    unchanged("range errors")
    lp, lz, steps = e.window_train(0, 9, seed=1)
    assert steps == 2 and lp > 0
    e.train_commit()
    unchanged("train + commit")
    e.selfplay_create(4, arena_nodes=1 << 12, seed=2, rollouts=4, max_examples=256)  # the loop recreates self-play after a pit
    e.selfplay_step(2)
    assert e.window_absorb() == 0  # nothing has finished after two plies
    unchanged("a second selfplay_create")
    e.window_create(0)
    raises(STATE, e.window_info)
    e.window_create(5)  # and again: empty
    assert e.window_info() == {"capacity": 5, "count": 0, "entered": 0, "evicted": 0}
    e.close()
