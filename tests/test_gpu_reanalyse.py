"""tg_reanalyse on the GPU: the visit counts it writes into window rows are those of a fresh search of the same positions through the
parent's entry points (search_reset → search_run → search_root on an engine with the same settings, all rows in ONE reset), and of
oracle.Search directly; everything else of the window stays byte for byte.  All comparisons are exact.

The window (capacity 37) is filled from hash-evaluator self-play as tests/test_gpu_window.py fills its own, until it has wrapped, and a
few of its oldest rows are pushed again so that logical row 0 sits at physical row 20: [3, 32) then occupies rows 23 … 36, 0 … 14."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import search_helpers as sh

pytestmark = pytest.mark.gpu

SP = dict(rollouts=8, noise_plies=6, exploit_plies=4, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0)  # endless
CAP, HEAD, GAMES, ROLLOUTS = 37, 20, 6, 8
FIRST, COUNT = 3, 29  # four full slices of 6 and a short one of 5
PARTS = ("hdr", "states", "moves", "visits")
STATE, INVALID, ARENA = -7, -1, -5


def _hash_engine(n):
    import tak_amd

    return tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=64, policy_head=tak_amd.HEAD_FC5 if n == 5 else tak_amd.HEAD_CONV)


def _net_engine(stem, precision=None):
    import tak_amd

    n, blocks, filters, head, tensors = sh._golden_net(stem)
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                       evaluator=tak_amd.EVAL_RESNET, max_batch=64)
    if precision:
        e.set_precision(precision)
    e.load_state_dict(tensors)
    return e, n


def _push(e, parts):
    hdr, states, moves, visits = parts
    e.window_push(states, hdr["n_moves"], moves, visits, hdr["result"], game_ids=hdr["game_id"])


def _absorbed_engine(n):
    """a hash engine whose window was filled by self-play and absorb until it wrapped, logical row 0 at physical row HEAD"""
    e = _hash_engine(n)
    e.selfplay_create(GAMES, arena_nodes=1 << 14, seed=7, max_examples=1 << 12, **SP)
    e.window_create(CAP)
    for _ in range(200):
        e.selfplay_step(3)
        e.window_absorb()
        info = e.window_info()  # wrapped, and rows of more than one game in it
        if info["entered"] >= CAP + 5 and len(set(e.window_read(0, CAP)[0]["game_id"].tolist())) >= 2:
            break
    info = e.window_info()
    assert info["entered"] >= CAP + 5 and info["count"] == CAP
    k = (HEAD - info["evicted"]) % CAP
    if k:
        _push(e, e.window_read(0, k))
    info = e.window_info()
    assert info["evicted"] > 0 and info["evicted"] % CAP == HEAD and info["count"] == CAP
    return e


@functools.lru_cache(maxsize=None)
def _rows(n):
    """(the 37 rows of _absorbed_engine(n)'s window, evicted): computed once, shared, never changed"""
    e = _absorbed_engine(n)
    parts, evicted = e.window_read(0, CAP), e.window_info()["evicted"]
    e.close()
    for p in parts:
        p.setflags(write=False)
    assert (parts[0]["n_moves"] < 512).all()  # short rows: the zeros past n_moves are part of every comparison
    return parts, evicted


def _fill(e, n):
    """the same window on another engine, by window_push: the same rows at the same cursors"""
    parts, evicted = _rows(n)
    e.window_create(CAP)
    idx = np.concatenate([np.arange(evicted) % CAP, np.arange(CAP)])
    _push(e, [p[idx] for p in parts])
    assert e.window_info() == {"capacity": CAP, "count": CAP, "entered": evicted + CAP, "evicted": evicted}
    return parts, evicted


def _fresh_search(ref, states, rollouts, noise=None, **create):
    """the parent's path on engine `ref`: every state in one search_reset, → (search_root, expansions)"""
    ref.search_create(len(states), arena_nodes=1 << 14, **create)
    ref.search_reset(states)
    if noise:
        ref.search_run(1)
        ref.search_apply_dirichlet(*noise)
    ref.search_run(rollouts)
    return ref.search_root(), ref.search_counters()[0]


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_window(e, before, first, count, visits, what=""):
    """the window of `e` is `before` with the visits of [first, first + count) replaced by `visits`; everything else byte-equal"""
    after = e.window_read(0, len(before[0]))
    for name, a, b in zip(PARTS[:3], after[:3], before[:3]):
        assert _same_bytes(a, b), (what, name)
    want = before[3].copy()
    want[first:first + count] = visits
    diff = np.flatnonzero((after[3] != want).any(axis=1))
    assert diff.size == 0, (what, "rows whose visits differ", diff.tolist())


def _assert_rows_are_the_roots(parts, sel, root, what=""):
    """the rows' move lists are the searched roots' children: the comparison of the visits is between like and like"""
    assert np.array_equal(root["counts"], parts[0]["n_moves"][sel]), what
    assert np.array_equal(root["moves"], parts[2][sel]), what


# ---- 1. rows equal a fresh search ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, 4])
@pytest.mark.parametrize("n", [5, 6])
def test_rows_equal_a_fresh_search_of_all_of_them_at_once(n, batch):
    parts, evicted = _rows(n)
    e = _absorbed_engine(n)
    before = e.window_read(0, CAP)
    for a, b in zip(before, parts):
        assert _same_bytes(a, b)  # self-play is seeded: the shared rows are this window's
    row0 = (evicted + FIRST) % CAP
    assert row0 + COUNT > CAP and evicted + FIRST >= CAP  # the range crosses the physical end of the ring; cursors beyond the capacity
    sel = slice(FIRST, FIRST + COUNT)
    ref = _hash_engine(n)
    root, expansions = _fresh_search(ref, parts[1][sel], ROLLOUTS, batch=batch, seed=5)
    _assert_rows_are_the_roots(parts, sel, root)
    assert (root["visits"].sum(axis=1) > 0).all() and (root["visits"] != parts[3][sel]).any()  # something to write
    e.search_create(GAMES, arena_nodes=1 << 14, batch=batch, seed=5)
    stats = e.reanalyse(FIRST, COUNT, ROLLOUTS)
    assert stats["rows"] == COUNT and stats["updated"] == COUNT and stats["mismatched"] == 0 and stats["unvisited"] == 0
    assert stats["expansions"] == expansions and stats["evals"] > 0
    _assert_window(e, before, FIRST, COUNT, root["visits"], f"{n}x{n} batch {batch}")
    assert e.window_info() == {"capacity": CAP, "count": CAP, "entered": evicted + CAP, "evicted": evicted}
    e.close()
    ref.close()


# ---- 2. the oracle directly ------------------------------------------------------------------------------------------------------
def test_six_rows_equal_the_oracles_search(orc):
    e, _, okw = sh._engines("hash", 5, 64)
    parts, _ = _fill(e, 5)
    sel = slice(30, 36)
    s = orc.Search(5, **okw)
    s.reset(parts[1][sel])
    s.run(16)
    root = s.root()
    _assert_rows_are_the_roots(parts, sel, root)
    e.search_create(GAMES, arena_nodes=1 << 14)
    stats = e.reanalyse(30, 6, 16)
    assert stats["updated"] == 6 and stats["expansions"] == s.counters()[0]
    _assert_window(e, parts, 30, 6, root["visits"])
    e.close()


# ---- 3. slicing independence -----------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_the_number_of_slots():
    windows = []
    for games in (1, 6, 32):  # 29 slices of one row; 4 + a short one; one slice with 3 dead slots
        e = _hash_engine(5)
        parts, _ = _fill(e, 5)
        e.search_create(games, arena_nodes=1 << 14, seed=5)
        assert e.reanalyse(FIRST, COUNT, ROLLOUTS)["updated"] == COUNT
        windows.append(e.window_read(0, CAP))
        e.close()
    assert (windows[0][3] != parts[3]).any()
    for w in windows[1:]:
        for a, b in zip(w, windows[0]):
            assert _same_bytes(a, b)


# ---- 4. noise --------------------------------------------------------------------------------------------------------------------
def test_noise_is_keyed_by_the_rows_cursor():
    alpha, ratio, rollouts = 0.2, 0.3, 12
    sel = slice(FIRST, FIRST + COUNT)
    got = {}
    for games in (6, 4):
        e = _hash_engine(5)
        parts, evicted = _fill(e, 5)
        e.search_create(games, arena_nodes=1 << 14, seed=5, slot_base=777)  # the object's own slot_base plays no part
        assert e.reanalyse(FIRST, COUNT, rollouts, noise_alpha=alpha, noise_ratio=ratio)["updated"] == COUNT
        got[games] = e.window_read(0, CAP)
        if games == 6:  # the same object again, without noise
            _fill(e, 5)
            assert e.reanalyse(FIRST, COUNT, rollouts)["updated"] == COUNT
            plain = e.window_read(0, CAP)
        e.close()
    ref = _hash_engine(5)
    root, _ = _fresh_search(ref, parts[1][sel], rollouts, noise=(alpha, ratio), seed=5, slot_base=(evicted + FIRST) & 0xFFFFFFFF)
    _assert_rows_are_the_roots(parts, sel, root)
    want = parts[3].copy()
    want[sel] = root["visits"]
    assert np.array_equal(got[6][3], want)
    assert np.array_equal(got[4][3], want)
    assert (plain[3] != want).any()  # the noise moved visits: the comparison has teeth
    quiet, _ = _fresh_search(ref, parts[1][sel], rollouts, seed=5)
    assert np.array_equal(plain[3][sel], quiet["visits"])
    ref.close()


# ---- 5. networks -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stem,precision,create", [
    ("net5_fc_2x32", None, {}),
    ("net6_conv_1x32", None, {}),
    ("net5_fc_1x64", "bf16x3", {}),
    ("net5_fc_2x32", None, dict(symmetry="hashed")),
    ("net5_fc_2x32", None, dict(proof="on")),
], ids=["fc5-f32", "conv6-f32", "fc5-bf16x3", "fc5-hashed", "fc5-proof"])
def test_networks_precisions_and_sticky_modes(stem, precision, create):
    first, count = 3, 13  # two full slices and one row
    e, n = _net_engine(stem, precision)
    ref, _ = _net_engine(stem, precision)
    parts, _ = _fill(e, n)
    sel = slice(first, first + count)
    root, expansions = _fresh_search(ref, parts[1][sel], ROLLOUTS, seed=3, **create)
    _assert_rows_are_the_roots(parts, sel, root)
    visited = root["visits"].sum(axis=1) > 0
    assert visited.sum() >= count - 2 and (root["visits"] != parts[3][sel]).any()
    e.search_create(GAMES, arena_nodes=1 << 14, seed=3, **create)
    stats = e.reanalyse(first, count, ROLLOUTS)
    assert stats["updated"] == int(visited.sum()) and stats["unvisited"] == count - int(visited.sum()) and stats["mismatched"] == 0
    assert stats["expansions"] == expansions
    want = np.where(visited[:, None], root["visits"], parts[3][sel])
    _assert_window(e, parts, first, count, want, stem)
    e.close()
    ref.close()


# ---- 6. rows that must not be touched --------------------------------------------------------------------------------------------
def _planted(orc, n, parts):
    """12 rows: good ones of the shared window with three kinds of bad ones between them → (parts, indices of the bad ones)"""
    idx = np.arange(4, 16)
    hdr, states, moves, visits = [p[idx].copy() for p in parts]
    visits[:] = 0
    visits[:, 0] = 1000  # no search of a few rollouts leaves this behind: a rewritten row shows
    short, swapped, finished = 2, 5, 9
    c = int(hdr["n_moves"][short])  # one move short of the legal count
    hdr["n_moves"][short] = c - 1
    moves[short, c - 1] = 0
    moves[swapped, [0, 1]] = moves[swapped, [1, 0]]  # two moves exchanged
    over = orc.playouts(n, 8, seed=3, half_komi=4)
    final = over["final"][over["result"] != 0]
    assert len(final)
    states[finished] = final[0]  # a finished position under somebody else's move list
    return [hdr, states, moves, visits], [short, swapped, finished]


def test_rows_whose_moves_are_not_the_roots_children_stay_byte_identical(orc):
    e = _hash_engine(5)
    planted, bad = _planted(orc, 5, _rows(5)[0])
    e.window_create(16)
    _push(e, planted)
    before = e.window_read(0, 12)
    good = np.setdiff1d(np.arange(12), bad)
    ref = _hash_engine(5)
    root, _ = _fresh_search(ref, before[1][good], ROLLOUTS, seed=1)
    _assert_rows_are_the_roots(before, good, root)
    e.search_create(5, arena_nodes=1 << 14, seed=1)
    stats = e.reanalyse(0, 12, ROLLOUTS)
    assert stats == {**stats, "rows": 12, "updated": 9, "mismatched": 3, "unvisited": 0}
    want = before[3].copy()
    want[good] = root["visits"]
    _assert_window(e, before, 0, 12, want)
    assert (want[good] != before[3][good]).any(axis=1).all()  # every neighbour was rewritten
    e.close()
    ref.close()


def test_roots_without_a_visited_child_stay_byte_identical():
    """Two ways to an all-zero visit sum.  One iteration of one rollout initialises the root and visits no child: every row is
    `unvisited`.  Under proof mode a root that is proven within its first rollouts may stop collecting visits: case 0 of
    tests/golden/solve_cases.json (the mover wins at once) is searched on the parent's path first, and the row is expected
    `unvisited` only if that path leaves its children's visit sum at 0 — otherwise `unvisited == 0` is what is asserted there."""
    import tactics_ref

    doc = json.load(open(os.path.join(sh.GOLDEN, "solve_cases.json")))
    case = doc["cases"][0]
    assert case["depth5"]["value"] == 1 and case["index"] == 0
    state = np.array(tactics_ref.positions(doc["set"])[0])
    moves = np.zeros((1, 512), np.uint16)
    moves[0, :case["counts"]] = case["moves"]
    visits = np.zeros((1, 512), np.uint32)
    visits[0, :case["counts"]] = 1
    e, ref = _hash_engine(5), _hash_engine(5)
    e.window_create(4)
    e.window_push(state[None], np.array([case["counts"]], np.int32), moves, visits, np.array([1.0], np.float32))
    before = e.window_read(0, 1)
    e.search_create(3, arena_nodes=1 << 14)
    stats = e.reanalyse(0, 1, 1)
    assert stats == {**stats, "rows": 1, "updated": 0, "mismatched": 0, "unvisited": 1, "expansions": 1}
    _assert_window(e, before, 0, 1, before[3])
    root, _ = _fresh_search(ref, state[None], ROLLOUTS, proof="on")
    _assert_rows_are_the_roots(before, slice(0, 1), root)
    zero = int(root["visits"].sum() == 0)
    print(f"proof mode, an immediate win, {ROLLOUTS} rollouts on the search path: children's visit sum {int(root['visits'].sum())}")
    e.search_create(3, arena_nodes=1 << 14, proof="on")
    stats = e.reanalyse(0, 1, ROLLOUTS)
    assert (stats["updated"], stats["unvisited"], stats["mismatched"]) == (1 - zero, zero, 0)
    _assert_window(e, before, 0, 1, before[3] if zero else root["visits"])
    e.close()
    ref.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_window_and_the_search_untouched():
    import tak_amd
    from tak_amd.engine import TgReanalyseConfig, TgReanalyseStats

    e = _hash_engine(5)
    parts, _ = _rows(5)

    def raw(first, count, cfg):
        return e.lib.tg_reanalyse(e.h, first, count, C.byref(cfg) if cfg is not None else None, C.byref(TgReanalyseStats()))

    def refused(code, word, first, count, cfg):
        assert raw(first, count, cfg) == code, word
        message = e.lib.tg_last_error().decode()
        assert "tg_reanalyse" in message and word in message, message

    good = TgReanalyseConfig(8, 0.0, 0.0, 0)
    refused(STATE, "tg_window_create", 0, 0, good)  # no window
    _fill(e, 5)
    refused(STATE, "tg_search_create", 0, 1, good)  # no search object
    e.selfplay_create(GAMES, arena_nodes=1 << 14, seed=7, max_examples=1 << 12, **SP)
    e.selfplay_step(2)
    kept = e.selfplay_stats()
    refused(STATE, "self-play", 0, 1, good)
    assert e.selfplay_stats() == kept
    e.search_create(GAMES, arena_nodes=1 << 14, slot_base=9)
    e.search_reset(parts[1][:GAMES])
    e.search_run(5)
    dump = e.search_dump(0)

    def untouched(what):
        for a, b in zip(e.window_read(0, CAP), parts):
            assert _same_bytes(a, b), what
        assert _same_bytes(e.search_dump(0), dump), what

    refused(INVALID, "cfg", 0, 1, None)
    for first, count in [(0, CAP + 1), (CAP, 1), (1, CAP), (2**31 - 1, 2**31 - 1)]:
        refused(INVALID, f"[0, {CAP})", first, count, good)
    refused(INVALID, "first", -1, 2, good)
    refused(INVALID, "count", 0, -1, good)
    refused(INVALID, "rollouts", 0, 1, TgReanalyseConfig(0, 0.0, 0.0, 0))
    refused(INVALID, "rollouts", 0, 1, TgReanalyseConfig(-3, 0.0, 0.0, 0))
    refused(INVALID, "noise_alpha", 0, 1, TgReanalyseConfig(8, -0.5, 0.0, 0))
    refused(INVALID, "noise_alpha", 0, 1, TgReanalyseConfig(8, float("nan"), 0.0, 0))
    refused(INVALID, "noise_ratio", 0, 1, TgReanalyseConfig(8, 0.2, 1.5, 0))
    refused(INVALID, "noise_ratio", 0, 1, TgReanalyseConfig(8, 0.2, -0.1, 0))
    refused(INVALID, "flags", 0, 1, TgReanalyseConfig(8, 0.0, 0.0, 1))
    for i in range(4):
        reserved = [0, 0, 0, 0]
        reserved[i] = 1
        refused(INVALID, "reserved", 0, 1, TgReanalyseConfig(8, 0.0, 0.0, 0, (C.c_int32 * 4)(*reserved)))
    untouched("refusals")
    with pytest.raises(tak_amd.TgError) as ei:
        e.reanalyse(0, CAP + 1, 8)
    assert ei.value.code == INVALID
    # the empty range, at either end: nothing happens, zero stats
    zero = {k: 0 for k in ("rows", "updated", "mismatched", "unvisited", "expansions", "evals")}
    assert e.reanalyse(0, 0, 8) == zero and e.reanalyse(CAP, 0, 8) == zero
    untouched("count = 0")
    e.close()


def _nodes(dump):
    """(nodes the tree has allocated, its largest children block)"""
    blocks = dump["n_children"][dump["n_children"] != 0xFFFF].astype(np.int64)
    return 1 + int(blocks.sum()), int(blocks.max())


def test_an_arena_too_small_for_the_second_slice_keeps_the_first(orc):
    """6 slots with 1024 nodes each are a pool of 25 chunks of 1024 nodes, 24 of them to hand out.  Slice 0 holds the six positions
    with the fewest legal moves of 3000 wall-heavy playouts one ply before their boards fill up, slice 1 six middle-game
    positions: the same 100 rollouts grow trees that fit on the first and cannot fit on the second.  Both facts are checked on
    a reference engine with room to spare before the call is made."""
    import tak_amd

    rollouts, chunk, usable = 100, 1024, 24
    full = orc.playouts(5, 3000, seed=7, style=2, half_komi=4, avoid_roads=True)["prev"]
    full = full[orc.result(5, full) == 0]
    small = full[np.argsort(orc.movegen(5, full)[1], kind="stable")[:GAMES]]
    large = sh._roots(orc, 5, GAMES, seed=12, max_plies=30)
    states = np.concatenate([small, large])
    moves, counts = orc.movegen(5, states)
    visits = (np.arange(512)[None, :] < counts[:, None]).astype(np.uint32)
    ref = _hash_engine(5)
    root, _ = _fresh_search(ref, states, rollouts)
    need = [_nodes(ref.search_dump(g)) for g in range(2 * GAMES)]
    most = sum(-(-nodes // (chunk - block)) + 1 for nodes, block in need[:GAMES])  # a block never straddles two chunks
    least = sum(-(-nodes // chunk) for nodes, _ in need[GAMES:])
    print(f"chunks: slice 0 needs at most {most}, slice 1 at least {least}, the pool hands out {usable}")
    assert most <= usable < least
    e = _hash_engine(5)
    e.window_create(16)
    e.window_push(states, counts, moves, visits, np.zeros(2 * GAMES, np.float32))
    before = e.window_read(0, 2 * GAMES)
    e.search_create(GAMES, arena_nodes=1024)
    with pytest.raises(tak_amd.TgError) as ei:
        e.reanalyse(0, 2 * GAMES, rollouts)
    assert ei.value.code == ARENA and "arena_nodes" in str(ei.value)
    want = before[3].copy()
    want[:GAMES] = root["visits"][:GAMES]
    assert (want[:GAMES] != before[3][:GAMES]).any(axis=1).all()
    _assert_window(e, before, 0, 2 * GAMES, want)
    # the error is the search object's: a new call starts from a whole pool
    assert e.reanalyse(0, GAMES, rollouts)["updated"] == GAMES
    _assert_window(e, before, 0, 2 * GAMES, want)
    e.close()
    ref.close()


# ---- 8. downstream ---------------------------------------------------------------------------------------------------------------
def test_window_train_on_a_reanalysed_window_is_tg_train_on_its_copy():
    import tak_amd
    import window_ref as wr

    w, n = _net_engine("net5_fc_2x32")
    t, _ = _net_engine("net5_fc_2x32")
    _, blocks, filters, _, _ = sh._golden_net("net5_fc_2x32")
    shapes = tak_amd.tensor_shapes(n, blocks, filters, w.head)
    for e in (w, t):
        e.train_create(chunk_size=wr.CHUNK, chunks_in_step=wr.CHUNKS_IN_STEP)
    parts, _ = _fill(w, n)
    w.search_create(GAMES, arena_nodes=1 << 14)
    assert w.reanalyse(0, CAP, ROLLOUTS)["updated"] == CAP
    hdr, states, moves, visits = w.window_read(0, CAP)
    assert (visits != parts[3]).any()
    got = w.window_train(0, CAP, seed=wr.SEEDS[0])
    want = t.train(states, hdr["n_moves"], moves, visits, hdr["result"], seed=wr.SEEDS[0])
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32)
    assert want[2] == 2 and got[2] == want[2] and bits(got[0]) == bits(want[0]) and bits(got[1]) == bits(want[1]), (got, want)
    for name, shape in shapes.items():
        assert np.array_equal(bits(w.train_get_tensor(name, shape)), bits(t.train_get_tensor(name, shape))), name
    w.close()
    t.close()
