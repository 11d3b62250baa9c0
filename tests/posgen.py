"""Test-input generators for the rarely reached corners of the rules (test infrastructure).

* tall_stack_states: packed states built directly (not by play) around one very tall stack, so that the high
  half of the u64 colour word, carries from the top of a 33…62-stone stack, the deep `game_repr` planes and the
  TPS / augmentation paths are exercised.  The states satisfy tg_search_reset's host-side check (heights, colour
  bits, reserves) — the format's invariants, which is what both implementations are specified on.
* with_header: copies of states with header bytes (reversible_plies, half_komi, …) overwritten.
* terminal_mix: whole games from oracle.playouts steered towards every ending of Game::result.
* empty_board / full_board: the positions on which the board planes of game_repr are all zero / dense.
* repr_corner_states: a few hundred states per board size that between them set EVERY input plane of game_repr, the board planes on
  every border class (corner, edge, interior) — what positions from random play never do (tests/test_repr_corners.py).
"""
import numpy as np

STONES = {3: (10, 0), 4: (15, 0), 5: (21, 1), 6: (30, 1)}
H_TO_MOVE, H_PLY, H_WS, H_WC, H_BS, H_BC, H_KOMI, H_REV = 1, 2, 4, 5, 6, 7, 8, 9  # byte offsets inside TgHeader


def state_bytes(n):
    return 256 if n <= 5 else 384


def distinct_positions(orc, n, count, seed, max_plies=60, half_komi=4):
    """`count` DIFFERENT ongoing positions (round 6: the full-batch tests used to tile ≈ 2 930 distinct positions to 4096 rows — every
    row was compared, but a quarter of them were repeats): random play-outs are drawn in rounds of 1.5 × what is still missing,
    finished games dropped, duplicates removed by content, until `count` are there."""
    have, seen = [], set()
    rnd = 0
    while len(have) < count:
        batch = orc.random_positions(n, max(256, int(1.5 * (count - len(have))) + 64), seed=seed + 7919 * rnd, max_plies=max_plies, half_komi=half_komi)
        batch = batch[orc.result(n, batch) == 0]
        for st in batch:
            key = st.tobytes()
            if key not in seen:
                seen.add(key)
                have.append(st)
                if len(have) == count:
                    break
        rnd += 1
        assert rnd < 64, "distinct_positions: the generator keeps repeating itself"
    return np.stack(have)


def with_header(states, **fields):
    """copy of `states` with TgHeader fields replaced: to_move, ply, white_stones, …, half_komi, reversible_plies"""
    out = np.array(states, np.uint8, copy=True).reshape(-1, states.shape[-1])
    h = out.shape[1] - 16
    for k, v in fields.items():
        v = np.asarray(v)
        if k == "ply":
            out[:, h + H_PLY] = (v & 0xFF).astype(np.uint8)
            out[:, h + H_PLY + 1] = ((v >> 8) & 0xFF).astype(np.uint8)
        else:
            off = {"to_move": H_TO_MOVE, "white_stones": H_WS, "white_caps": H_WC, "black_stones": H_BS, "black_caps": H_BC,
                   "half_komi": H_KOMI, "reversible_plies": H_REV}[k]
            out[:, h + off] = (v.astype(np.int64) & 0xFF).astype(np.uint8)
    return out


def header(states, field):
    states = np.asarray(states).reshape(-1, states.shape[-1])
    h = states.shape[1] - 16
    if field == "ply":
        return states[:, h + H_PLY].astype(np.int32) | (states[:, h + H_PLY + 1].astype(np.int32) << 8)
    off = {"to_move": H_TO_MOVE, "white_stones": H_WS, "white_caps": H_WC, "black_stones": H_BS, "black_caps": H_BC,
           "half_komi": H_KOMI, "reversible_plies": H_REV}[field]
    v = states[:, h + off]
    return v.astype(np.int8) if field == "half_komi" else v


def heights(states, n):
    slots = 25 if n <= 5 else 36
    return states.reshape(-1, states.shape[-1])[:, 8 * slots: 8 * slots + n * n] & 63


def tall_stack_states(n, count, seed, lo=33, hi=None):
    """`count` packed states, each with one stack of height in [lo, hi] (default hi = every stone of both supplies)
    plus a few small stacks around it; reserves are what is left of the supplies."""
    S, Cc = STONES[n]
    hi = hi or 2 * (S + Cc)
    rng = np.random.default_rng(seed)
    sb, slots, nsq = state_bytes(n), (25 if n <= 5 else 36), n * n
    out = np.zeros((count, sb), np.uint8)
    for i in range(count):
        H = int(rng.integers(lo, hi + 1))
        avail = {0: [S, Cc], 1: [S, Cc]}  # colour → [stones, caps] still in reserve
        st64 = np.zeros(slots, np.uint64)
        meta = np.zeros(slots, np.uint8)

        def build(height, want_top=None):
            """colours bottom→top and the top piece type, drawn from what the supplies still hold"""
            cols = []
            for k in range(height):
                last = k == height - 1
                choices = [c for c in (0, 1) if avail[c][0] > 0 or (last and avail[c][1] > 0)]
                if not choices:
                    break
                c = int(rng.choice(choices))
                top = 0
                if last:
                    kinds = ([0, 1] if avail[c][0] > 0 else []) + ([2] if avail[c][1] > 0 else [])
                    top = int(rng.choice(kinds)) if want_top is None or want_top not in kinds else want_top
                if top == 2:
                    avail[c][1] -= 1
                else:
                    avail[c][0] -= 1
                cols.append(c)
                if last:
                    return cols, top
            return cols, 0

        squares = rng.permutation(nsq)
        cols, top = build(H, want_top=int(rng.integers(0, 3)))
        sq0 = int(squares[0])
        st64[sq0] = sum(np.uint64(c) << np.uint64(k) for k, c in enumerate(cols)) if cols else np.uint64(0)
        meta[sq0] = len(cols) | (top << 6)
        keep_reserves = rng.random() < 0.7  # most states stay Ongoing: both colours keep a few stones in hand
        for sq in squares[1: 1 + int(rng.integers(2, nsq - 1))]:
            if keep_reserves and min(avail[0][0], avail[1][0]) <= 2:
                break
            h = int(rng.integers(0, 5))
            cols, top = build(h)
            if not cols:
                continue
            st64[sq] = sum(np.uint64(c) << np.uint64(k) for k, c in enumerate(cols))
            meta[sq] = len(cols) | (top << 6)
        out[i, : 8 * slots] = st64.view(np.uint8)
        out[i, 8 * slots: 9 * slots] = meta
        to_move = int(rng.integers(0, 2))
        ply = 2 * int(rng.integers(20, 200)) + to_move
        hdr = out[i, sb - 16:]
        hdr[0] = n
        hdr[H_TO_MOVE] = to_move
        hdr[H_PLY], hdr[H_PLY + 1] = ply & 0xFF, ply >> 8
        hdr[H_WS], hdr[H_WC], hdr[H_BS], hdr[H_BC] = avail[0][0], avail[0][1], avail[1][0], avail[1][1]
        hdr[H_KOMI] = np.uint8(int(rng.integers(-5, 7)) & 0xFF)
        hdr[H_REV] = int(rng.integers(0, 50))
    return out


def terminal_mix(orc, n, per_style=3000, seed=1):
    """final states / previous states / last moves / results of whole steered games (every ending of Game::result)"""
    parts = []
    for style in range(5):
        for avoid in (False, True):
            parts.append(orc.playouts(n, per_style, seed=seed * 100 + style * 2 + int(avoid), style=style, avoid_roads=avoid,
                                      max_plies=700))
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def empty_board(n, to_move, half_komi=4):
    S, Cc = STONES[n]
    st = np.zeros(state_bytes(n), np.uint8)
    h = st[-16:]
    h[0] = n
    h[H_TO_MOVE] = to_move
    h[H_PLY] = to_move
    h[H_WS], h[H_WC], h[H_BS], h[H_BC] = S, Cc, S, Cc
    h[H_KOMI] = np.uint8(half_komi & 0xFF)
    return st


def full_board(n, to_move, caps=None, shift=0, half_komi=4):
    """every square holds one piece: colour (sq + shift) & 1, a wall where (sq + shift) % 7 = 3, white's and black's capstone (boards
    that have one) on the squares `caps` (default n + 1 and 3n + 2); reserves = what is left of the supplies"""
    S, Cc = STONES[n]
    slots, nsq = (25 if n <= 5 else 36), n * n
    caps = ((n + 1, 3 * n + 2) if caps is None else tuple(caps)) if Cc else ()
    st = np.zeros(state_bytes(n), np.uint8)
    colours = np.zeros(slots, np.uint64)
    meta = np.zeros(slots, np.uint8)
    used = {0: [0, 0], 1: [0, 0]}
    for sq in range(nsq):
        c = caps.index(sq) if sq in caps else (sq + shift) & 1
        top = 2 if sq in caps else 1 if (sq + shift) % 7 == 3 else 0
        colours[sq] = c
        meta[sq] = 1 | (top << 6)
        used[c][1 if top == 2 else 0] += 1
    assert max(used[0][0], used[1][0]) <= S
    st[: 8 * slots] = colours.view(np.uint8)
    st[8 * slots: 9 * slots] = meta
    h = st[-16:]
    h[0] = n
    h[H_TO_MOVE] = to_move
    h[H_PLY] = 50 + to_move
    h[H_WS], h[H_WC] = S - used[0][0], Cc - used[0][1]
    h[H_BS], h[H_BC] = S - used[1][0], Cc - used[1][1]
    h[H_KOMI] = np.uint8(half_komi & 0xFF)
    return st


def border_class(n):
    """tower_cb_index's class of every square: 3·(y = 0 ? 0 : y = n − 1 ? 2 : 1) + (x = 0 ? 0 : x = n − 1 ? 2 : 1) — which of the 9
    taps of a 3×3 convolution stay on the board"""
    k = np.where(np.arange(n) == 0, 0, np.where(np.arange(n) == n - 1, 2, 1))
    return (3 * k[:, None] + k[None, :]).reshape(-1)


def class_squares(n):
    """one square of every border class, in class order"""
    cls = border_class(n)
    return [int(np.flatnonzero(cls == c)[-1 if c == 4 else 0]) for c in range(9)]


def reserves_consistent(states, n):
    """per state: reserves + pieces on the board = the starting supplies, per colour and piece type"""
    S, Cc = STONES[n]
    states = np.asarray(states).reshape(-1, states.shape[-1])
    slots = 25 if n <= 5 else 36
    hs = heights(states, n).astype(np.uint64)
    words = np.ascontiguousarray(states[:, : 8 * slots]).view(np.uint64)[:, : n * n]
    black = np.zeros(words.shape, np.int64)
    for k in range(62):
        black += ((words >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
    tops = states[:, 8 * slots: 8 * slots + n * n] >> 6
    top_black = ((words >> (np.maximum(hs, 1) - 1)) & np.uint64(1)).astype(bool) & (hs > 0)
    caps_b = ((tops == 2) & top_black).sum(axis=1)
    caps_w = ((tops == 2) & ~top_black & (hs > 0)).sum(axis=1)
    hs = hs.astype(np.int64)
    return ((header(states, "black_stones") + black.sum(axis=1) - caps_b == S) & (header(states, "black_caps") + caps_b == Cc) &
            (header(states, "white_stones") + (hs - black).sum(axis=1) - caps_w == S) & (header(states, "white_caps") + caps_w == Cc))


def is_position(states, n):
    """per state: the rules of the engine's host-side check of packed states (validate_states: board size, to_move, reserves within the
    supplies, nothing beyond the board, empty squares clean, piece type ≤ 2, heights within the supply, no colour bit above the height)"""
    S, Cc = STONES[n]
    states = np.asarray(states).reshape(-1, states.shape[-1])
    slots, nsq = (25 if n <= 5 else 36), n * n
    hdr = states[:, -16:]
    ok = (states.shape[1] == state_bytes(n)) & (hdr[:, 0] == n) & (hdr[:, H_TO_MOVE] <= 1)
    ok &= (hdr[:, H_WS] <= S) & (hdr[:, H_BS] <= S) & (hdr[:, H_WC] <= Cc) & (hdr[:, H_BC] <= Cc)
    words = np.ascontiguousarray(states[:, : 8 * slots]).view(np.uint64)
    meta = states[:, 8 * slots: 9 * slots]
    hs = (meta & 63).astype(np.uint64)
    ok &= ~(meta[:, nsq:].any(axis=1) | words[:, nsq:].any(axis=1))
    ok &= ~(((hs == 0) & ((meta != 0) | (words != 0)))[:, :nsq]).any(axis=1)
    ok &= ((meta >> 6) <= 2).all(axis=1) & (hs <= min(62, 2 * (S + Cc))).all(axis=1) & ~(words >> hs).any(axis=1)
    return ok & (hs.sum(axis=1) <= 2 * (S + Cc))


def _tall_on_classes(n, per_class, seed, lo):
    """tall_stack_states with the tall stack moved (by exchanging two squares) onto every border class in turn"""
    sts = tall_stack_states(n, 9 * per_class, seed, lo=lo)
    slots, sq_of = (25 if n <= 5 else 36), class_squares(n)
    for i, st in enumerate(sts):
        a, b = int(np.argmax(heights(st[None], n)[0])), sq_of[i % 9]
        words, meta = st[: 8 * slots].view(np.uint64), st[8 * slots: 9 * slots]
        words[[a, b]] = words[[b, a]]
        meta[[a, b]] = meta[[b, a]]
    return sts


def _reserve_ladder(n):
    """consistent positions with k stones in white's reserve and S + 1 − k in black's, k = 1 … S: what is missing lies in two
    one-colour stacks on a diagonal (no road), under either colour to move"""
    S, Cc = STONES[n]
    slots = 25 if n <= 5 else 36
    out = []
    for k in range(1, S + 1):
        for to_move in (0, 1):
            st = empty_board(n, to_move, half_komi=(k % 5) - 2)
            words, meta = st[: 8 * slots].view(np.uint64), st[8 * slots: 9 * slots]
            for sq, colour, height in ((0, 0, S - k), (n + 1, 1, k - 1)):
                if height:
                    words[sq] = np.uint64((1 << height) - 1 if colour else 0)
                    meta[sq] = height
            h = st[-16:]
            h[H_PLY] = 40 + to_move
            h[H_WS], h[H_BS] = k, S + 1 - k
            out.append(st)
    return np.stack(out)


def _other_to_move(states):
    return with_header(states, to_move=1 - header(states, "to_move").astype(np.int64), ply=header(states, "ply") ^ 1)


def repr_corner_states(orc, n, seed=0):
    """A few hundred packed states (deterministic) on which every input plane of game_repr is set somewhere and zero somewhere, every
    0/1 board plane on every border class: tall stacks (every depth of the buried-stone planes, the cap at N + 6 included) on a square
    of each class under both colours to move; full boards with the capstones on each class; the empty board; a ladder of positions over
    every reserve count; positions from play; and header sweeps over copies — every own / enemy reserve count 0 … S, caps 0 … C, both
    to_move, half_komi −6 … 6 (−12 … 12 on one of them).  Every state passes tg_search_reset's host-side check.
    → (states, indices of the states that are ongoing with reserves consistent with the board: the only ones for the search / trainer)"""
    S, Cc = STONES[n]
    tall = np.concatenate([_tall_on_classes(n, 2, seed + 11 * n, lo=n + 7), _tall_on_classes(n, 2, seed + 13 * n, lo=33 if n >= 5 else n + 7)])
    tall = np.concatenate([tall, _other_to_move(tall)])
    sq_of = class_squares(n)
    full = np.stack([full_board(n, tm, caps=(sq_of[v], sq_of[(v + 1) % 9]), shift=v) for v in range(9) for tm in (0, 1)])
    empty = np.stack([empty_board(n, 0), empty_board(n, 1)])
    ladder = _reserve_ladder(n)
    play = distinct_positions(orc, n, 32, seed=seed + 5, max_plies={3: 8, 4: 16, 5: 60, 6: 80}[n])
    # header sweeps: the reserve counts on a position from play and on a tall stack, the komi on three positions
    base = np.stack([play[-1], tall[0]])
    base = np.concatenate([base, _other_to_move(base)])
    sweeps = [with_header(base, white_stones=v, black_stones=S - v) for v in range(S + 1)]
    sweeps += [with_header(base, white_caps=a, black_caps=b) for a in range(Cc + 1) for b in range(Cc + 1)]
    sweeps += [with_header(np.stack([play[0], tall[1], ladder[S]]), half_komi=hk) for hk in range(-6, 7)]
    sweeps += [with_header(play[1][None], half_komi=hk) for hk in list(range(-12, -6)) + list(range(7, 13))]  # (flat counts differ little on 3×3)
    sts = np.concatenate([tall, full, empty, ladder, play] + sweeps)
    sts = sts[np.random.default_rng(seed).permutation(len(sts))]  # every kind among the first 64
    ok = (orc.result(n, sts) == 0) & reserves_consistent(sts, n)
    return sts, np.flatnonzero(ok)


def covering_subset(planes, count):
    """indices of `count` rows of `planes` [B, C, n, n] chosen greedily so that every channel that is non-zero anywhere is non-zero in
    one of them (then filled up in order)"""
    on = np.abs(planes).reshape(planes.shape[0], planes.shape[1], -1).max(axis=2) > 0
    need, chosen = on.any(axis=0), []
    while need.any():
        gain = (on & need).sum(axis=1)
        gain[chosen] = -1
        i = int(np.argmax(gain))
        chosen.append(i)
        need &= ~on[i]
    assert len(chosen) <= count, (len(chosen), count)
    chosen += [i for i in range(len(planes)) if i not in set(chosen)][: count - len(chosen)]
    return np.array(chosen)


def from_tps(n, tps, half_komi=4, reversible_plies=0):
    """the packed state of a TPS string ("row n/…/row 1 player move", stacks bottom → top as 1 / 2 with S or C on top); the
    reserves are what the board leaves of the supplies"""
    S, Cc = STONES[n]
    board, player, number = tps.split()
    slots = 25 if n <= 5 else 36
    st = np.zeros(state_bytes(n), np.uint8)
    words, meta = st[: 8 * slots].view(np.uint64), st[8 * slots: 9 * slots]
    left = {0: [S, Cc], 1: [S, Cc]}
    rows = board.split("/")
    assert len(rows) == n
    for r, text in enumerate(rows):
        col = 0
        for cell in text.split(","):
            if cell[0] == "x":
                col += int(cell[1:] or 1)
                continue
            top = {"S": 1, "C": 2}.get(cell[-1], 0)
            stones = cell.rstrip("SC")
            sq = (n - 1 - r) * n + col
            words[sq] = sum((int(ch) - 1) << k for k, ch in enumerate(stones))
            meta[sq] = len(stones) | (top << 6)
            for k, ch in enumerate(stones):
                left[int(ch) - 1][1 if top == 2 and k == len(stones) - 1 else 0] -= 1
            col += 1
        assert col == n, text
    assert min(left[0] + left[1]) >= 0, "more pieces than the supplies hold"
    to_move = int(player) - 1
    ply = 2 * (int(number) - 1) + to_move
    h = st[-16:]
    h[0], h[H_TO_MOVE], h[H_PLY], h[H_PLY + 1] = n, to_move, ply & 0xFF, ply >> 8
    h[H_WS], h[H_WC], h[H_BS], h[H_BC] = left[0][0], left[0][1], left[1][0], left[1][1]
    h[H_KOMI], h[H_REV] = np.uint8(half_komi & 0xFF), reversible_plies
    return st


# ---- positions with more than TG_MAX_MOVES (512) legal moves: tests/test_long_move_lists.py, tests/test_gpu_long_move_lists.py ------
def swap_colours(state, n):
    """the same position with the colours exchanged (stones, reserves, the side to move; the ply moves on by one)"""
    st = np.array(state, np.uint8, copy=True)
    slots = 25 if n <= 5 else 36
    words, meta = st[: 8 * slots].view(np.uint64), st[8 * slots: 9 * slots]
    words ^= (np.uint64(1) << (meta & 63).astype(np.uint64)) - np.uint64(1)
    h = st[-16:]
    h[H_WS], h[H_BS], h[H_WC], h[H_BC] = h[H_BS], h[H_WS], h[H_BC], h[H_WC]
    ply = (int(h[H_PLY]) | int(h[H_PLY + 1]) << 8) + 1
    h[H_TO_MOVE], h[H_PLY], h[H_PLY + 1] = h[H_TO_MOVE] ^ 1, ply & 0xFF, ply >> 8
    return st


def symmetry_image(state, n, s):
    """the image of a position under symmetry s of the square group: s < 4 is rotate^s, s ≥ 4 mirror (col → n − 1 − col) then
    rotate^(s − 4), rotate being (col, row) → (row, n − 1 − col)"""
    st = np.array(state, np.uint8, copy=True)
    slots = 25 if n <= 5 else 36
    words, meta = st[: 8 * slots].view(np.uint64), st[8 * slots: 9 * slots]
    w0, m0 = words.copy(), meta.copy()
    for sq in range(n * n):
        col, row = sq % n, sq // n
        if s >= 4:
            col = n - 1 - col
        for _ in range(s & 3):
            col, row = row, n - 1 - col
        words[row * n + col], meta[row * n + col] = w0[sq], m0[sq]
    return st


def take_back_flat(state, n, sq):
    """the position before the side NOT to move placed the lone flat on `sq`: that flat back in its reserve, that side to move.
    → (state, the move code of the placement: a flat on sq)"""
    st = np.array(state, np.uint8, copy=True)
    slots = 25 if n <= 5 else 36
    words, meta = st[: 8 * slots].view(np.uint64), st[8 * slots: 9 * slots]
    h = st[-16:]
    placer = int(h[H_TO_MOVE]) ^ 1
    assert meta[sq] == 1 and int(words[sq]) == placer, "the square does not hold a lone flat of the side that moved last"
    words[sq], meta[sq] = 0, 0
    h[H_BS if placer else H_WS] += 1
    ply = (int(h[H_PLY]) | int(h[H_PLY + 1]) << 8) - 1
    h[H_TO_MOVE], h[H_PLY], h[H_PLY + 1] = placer, ply & 0xFF, ply >> 8
    return st, sq  # (a placement's code is square | piece << 6, and a flat is piece 0)


def reply_table(orc, n, state, capacity=4096):
    """per move of the position's UNCUT list, in possible_moves order: (moves, result of the child, whether the child is ongoing and
    its mover has a move that wins at once) — by the oracle alone"""
    state = np.ascontiguousarray(state, np.uint8).reshape(1, -1)
    moves, counts = orc.movegen_full(n, state, capacity)
    c = int(counts[0])
    ch, status = orc.play(n, np.repeat(state, c, axis=0), moves[0, :c])
    assert not status.any()
    res = orc.result(n, ch)
    mover = int(state[0, -16 + H_TO_MOVE]) ^ 1  # the side to move in the children
    wins = (3, 4) if mover else (1, 2)
    hit = np.zeros(c, bool)
    for j in np.flatnonzero(res == 0):
        rm, rc = orc.movegen_full(n, ch[j], capacity)
        rch, rst = orc.play(n, np.repeat(ch[j][None], int(rc[0]), axis=0), rm[0, : rc[0]])
        assert not rst.any()
        hit[j] = np.isin(orc.result(n, rch), wins).any()
    return moves[0, :c], res, hit


LONG_LIST_TPS = {
    # eight mover-topped stacks of height 6 in the interior: 1076 moves
    "max": "x,x,x,x,x,x/x,x,221211,221211,x,x/x,x,221211,221211,x,x/x,x,221211,221211,x,x/x,x,221211,221211,x,x/x,x,x,x,x,x 1 51",
    # S: 763 moves; after each of the first 512 black completes the f-file at once; the only defences (f6) lie behind index 512
    "S": "x,x,x,x,2S,x/x,211111,111111,x,2S,2/x,212121,212121,x,2S,2/x,212121,212121,x,2S,2/x,212121,212121,x,2S,2/x,x,x,x,2S,2 1 51",
    # white's c-file lacks only c6 (a placement early in the list): more than 512 moves, an instant road among the first 512; the
    # black flat on a1 is the move that led here
    "W": "x,x,x,x,x,x/x,x,221211,221211,x,x/x,x,221211,221211,x,x/x,x,221211,221211,x,x/x,x,221211,221211,x,x/2,x,1,x,x,x 1 51",
    # exactly 512 / 513 moves (stacks of "max" trimmed until the oracle's count said so); the black flats on a1 (a2) are there to be
    # taken back: "e512" is reached from its root by a2, "e513" by a1
    "e512": "x,x,x,x,x,x/x,x,211,211,x,x/x,x,221211,221211,x,x/x,x,1211,211,x,x/2,x,211,1211,x,x/2,x,x,x,x,x 1 51",
    "e513": "x,x,x,x,x,x/x,x,211,21211,x,x/x,x,1211,1211,x,x/x,x,1211,221211,x,x/x,x,211,1211,x,x/2,x,x,x,x,x 1 51",
    "e512_bare": "x,x,x,x,x,x/x,x,21211,21211,x,x/x,x,1211,211,x,x/x,x,21211,211,x,x/x,x,211,21211,x,x/x,x,x,x,x,x 1 51",
}
# roots (black to move, nothing of black's on top of a square: its moves are placements only) whose children have at most 512 moves, 39
# of them exactly 512 / at most 513, 44 of them exactly 513: the capacity's edge INSIDE the solver's tree
EDGE_ROOT_TPS = {
    "E512": "x,x,x,x,x,1/x,x,21211,21211,x,x/x,x,221211,1211,x,x/x,x,11,11,x,x/x,x,1211,1211,x,x/x,x,x,x,x,x 2 50",
    "E513": "x,x,x,x,x,x/x,x,211,1211,x,x/x,x,21211,1211,x,x/x,x,1211,221211,x,x/x,x,211,1211,x,x/x,x,x,x,x,x 2 50",
}


def long_list_states(orc, n=6):
    """Positions around the move-list capacity TG_MAX_MOVES = 512, built directly (they pass is_position and reserves_consistent and are
    ongoing; whether play reaches them is beside the point: every entry point takes positions from callers).
    → dict(states = name → packed state, roots = name → (root state, move code, name of the child the move leads to),
           edge_roots = "E512" / "E513" → a root whose longest child list is exactly 512 / 513 (EDGE_ROOT_TPS),
           s_images = the symmetries of S (1 … 7) whose image keeps every defence behind index 511).
    states: "max" 1076 moves; "S" 763 moves, every one of the first 512 loses at once, the defences lie behind; "S_swapped" its colour
    twin; "S_sym<k>" the kept images of S; "S_mirror" S mirrored (file a open: the defences come first in the list — the control);
    "W" an instant road among the first 512 of more; "e512" / "e513" / "e512_bare" the edge.
    roots: "R" → S, "R_swapped" → S_swapped, "R_mirror" → S_mirror, "R_W" → W, "R_e512" → e512, "R_e513" → e513: each is the child
    with one flat of the side not to move back in hand, so its own list is short."""
    assert n == 6, "the family is built on 6×6 only"
    states = {k: from_tps(n, t) for k, t in LONG_LIST_TPS.items()}
    states["S_swapped"] = swap_colours(states["S"], n)
    states["S_mirror"] = symmetry_image(states["S"], n, 4)
    s_images = []
    for s in range(1, 8):
        img = symmetry_image(states["S"], n, s)
        _, res, hit = reply_table(orc, n, img)
        if (res[:512] == 0).all() and hit[:512].all():
            s_images.append(s)
            states[f"S_sym{s}"] = img
    f3, a3, a1, a2 = 2 * n + 5, 2 * n, 0, n
    roots = {}
    for name, child, sq in (("R", "S", f3), ("R_swapped", "S_swapped", f3), ("R_mirror", "S_mirror", a3), ("R_W", "W", a1),
                            ("R_e512", "e512", a2), ("R_e513", "e513", a1)):
        root, move = take_back_flat(states[child], n, sq)
        roots[name] = (root, move, child)
    edge_roots = {k: from_tps(n, t) for k, t in EDGE_ROOT_TPS.items()}
    return dict(states=states, roots=roots, edge_roots=edge_roots, s_images=s_images)
