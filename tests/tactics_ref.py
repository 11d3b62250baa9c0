"""Reference for the forced-win solver (tg_solve): the definitions of include/takgpu.h stated in plain Python on the CPU
rules (oracle.movegen / play / result).  Nothing here follows the kernels' structure: W and X are the two recursive
predicates, a move's value is the least level at which one of them holds, and the early stop is a clip of those values.

    W(s, L)  the mover wins within L plies      X(s, L)  the mover loses within L plies

`Ref(n, variant=...)` plants one deliberate mistake (VARIANTS) — the teeth tests check that `compare`, the comparison the
GPU tests use, rejects each of them."""
import functools

import numpy as np

import posgen
from oracle import oracle

TG_MAX_MOVES = 512
VARIANTS = ("no_suicide", "draw_is_loss", "min_at_lost", "last_best", "no_early_stop", "reversible_is_ongoing")
# mistakes about the move-list capacity inside the tree (they show only below a position with more than TG_MAX_MOVES moves):
# the parent's behaviour, which took the first TG_MAX_MOVES of a longer list for the whole list, and a give-up that is not reported
CAPACITY_VARIANTS = ("cut_x_test", "silent_give_up")
TG_DRAW_REVERSIBLE = 6  # the result code of the 50-reversible-plies draw
FIELDS = ("value", "best", "counts", "moves", "move_values")


class Ref:
    """W, X and the move values on arrays of positions: W(S, L)[i] / X(S, L)[i] is the predicate on the ongoing position S[i]."""
    CHUNK = 2048  # positions expanded at once (bounds the memory of one batch of children)

    def __init__(self, n, variant=None, capacity=TG_MAX_MOVES):
        """capacity: the longest move list a position INSIDE the tree may have (include/takgpu.h, "Move-list capacity inside the tree":
        X on a longer list gives up, W searches its first `capacity` moves and gives up if none of them wins); None = no capacity,
        the exact predicates on whole lists"""
        assert variant is None or variant in VARIANTS + CAPACITY_VARIANTS
        self.n = n
        self.capacity = capacity
        self.sb = oracle.state_bytes(n)
        self.variant = variant
        self.nodes = 0  # children generated

    def mover(self, S):
        return S[:, self.sb - 16 + 1].astype(np.int64)

    @staticmethod
    def won(res, color):
        return np.where(color == 0, (res == 1) | (res == 2), (res == 3) | (res == 4))

    def lost_at_once(self, res, m):
        """the move just played by m ends the game against m"""
        lost = self.won(res, m ^ 1)
        if self.variant == "no_suicide":
            lost = np.zeros_like(lost)
        if self.variant == "draw_is_loss":
            lost = lost | (res >= 5)
        return lost

    def play(self, S, moves):
        ch, status = oracle.play(self.n, S, moves)
        assert not status.any()
        self.nodes += len(ch)
        res = oracle.result(self.n, ch)
        if self.variant == "reversible_is_ongoing":  # the wrong result code tested: the draw by the counter is searched on
            res = np.where(res == TG_DRAW_REVERSIBLE, 0, res).astype(res.dtype)
        return ch, res

    def lists(self, S):
        """(moves, counts, cut) as the solver sees them: the whole list up to the capacity; cut = the position has more"""
        if self.capacity is None:
            moves, counts = oracle.movegen_full(self.n, S)
            return moves, counts, np.zeros(len(S), bool)
        moves, counts = oracle.movegen(self.n, S)
        cut = counts > self.capacity
        if self.variant == "cut_x_test":  # the mistake planted: a cut list is taken for the whole list
            cut = np.zeros(len(S), bool)
        return moves, np.minimum(counts, self.capacity), cut

    def W(self, S, L):
        """some move wins at once, or leads to an ongoing position that is X within L - 1.  → (holds, gave up): the moves are tried
        in order up to the first that wins; gave up = a test on a cut list failed on the way (a cut list of S itself without a win
        among its first `capacity` moves included)"""
        k = len(S)
        if L <= 0 or k == 0:
            return np.zeros(k, bool), np.zeros(k, bool)
        if k > self.CHUNK:
            parts = [self.W(S[i:i + self.CHUNK], L) for i in range(0, k, self.CHUNK)]
            return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
        moves, counts, cut = self.lists(S)
        idx = np.repeat(np.arange(k), counts)
        col = np.arange(len(idx)) - np.repeat(np.cumsum(counts) - counts, counts)
        ch, res = self.play(S[idx], moves[idx, col])
        win = self.won(res, self.mover(S)[idx])
        gave_up = np.zeros(len(idx), bool)
        never = np.iinfo(np.int64).max
        first = np.full(k, never)  # the first move that wins: the test does not look behind it
        np.minimum.at(first, idx[win], col[win])
        if L > 1:
            cand = np.nonzero((res == 0) & (col < first[idx]))[0]
            win[cand], gave_up[cand] = self.X(ch[cand], L - 1)
            np.minimum.at(first, idx[win], col[win])
        out = first < never
        over = cut & ~out
        seen = gave_up & (col <= first[idx])
        over[idx[seen]] = True
        return out, over

    def X(self, S, L):
        """every move loses at once, or leads to an ongoing position that is W within L - 1 (move by move: a position leaves
        the test at its first move that does neither).  → (holds, gave up): a position whose list is cut fails before its first
        move and has given up; otherwise gave up = one of the W tests on the way did"""
        k = len(S)
        if L <= 0 or k == 0:
            return np.zeros(k, bool), np.zeros(k, bool)
        moves, counts, cut = self.lists(S)
        out, over = ~cut, cut.copy()
        if self.variant == "silent_give_up":  # the mistake planted: the give-up is not reported
            over = np.zeros(k, bool)
        m = self.mover(S)
        alive, j = np.nonzero(~cut)[0], 0
        while True:
            alive = alive[counts[alive] > j]
            if not len(alive):
                return out, over
            ch, res = self.play(S[alive], moves[alive, j])
            ok = self.lost_at_once(res, m[alive])
            if L > 1:
                cand = np.nonzero((res == 0) & ~ok)[0]
                ok[cand], sub = self.W(ch[cand], L - 1)
                over[alive[cand]] |= sub
            out[alive[~ok]] = False
            alive, j = alive[ok], j + 1

    def fold(self, moves, vals):
        """(value, best) of a position from its move values"""
        pos = [v for v in vals if v > 0]
        if pos:
            value = min(pos)
        elif len(vals) and all(v < 0 for v in vals):
            value = -(min if self.variant == "min_at_lost" else max)(-v for v in vals)
        else:
            return 0, 0
        hits = [a for a, v in enumerate(vals) if v == value]
        return value, int(moves[hits[-1] if self.variant == "last_best" else hits[0]])

    def solve_one(self, s, depth, all_moves):
        """→ (value, best, moves, move_values)"""
        return self.solve_one_full(s, depth, all_moves)[:4]

    def solve_one_full(self, s, depth, all_moves):
        """→ (value, best, moves, move_values, gave up).  Level L gives a still unvalued move a the value +L if X(s_a, L - 1), else
        -L if W(s_a, L - 1): the least k of the definition, found by trying k = 0, 1, … in turn.  gave up = some test of some level
        that ran failed on a cut list."""
        s = np.ascontiguousarray(s, np.uint8).reshape(1, -1)
        if int(oracle.result(self.n, s)[0]) != 0:
            return 0, 0, np.zeros(0, np.uint16), [], False
        moves, counts = oracle.movegen(self.n, s)
        c = int(counts[0])
        if c > TG_MAX_MOVES:  # the root's own list is an output row of TG_MAX_MOVES: the call is refused (TG_ERR_INVALID_ARG)
            raise ValueError(f"the root has {c} moves, more than TG_MAX_MOVES")
        moves = moves[0, :c]
        ch, res = self.play(np.repeat(s, c, axis=0), moves)
        m = self.mover(s).repeat(c)
        vals = np.zeros(c, np.int64)
        vals[self.lost_at_once(res, m)] = -1
        vals[self.won(res, m)] = 1
        stop_early = not (all_moves or self.variant == "no_early_stop")
        gave_up = False
        for level in range(1, depth + 1):  # the levels run: L* is the first that decides the position, or depth
            if level > 1:
                pend = np.nonzero((res == 0) & (vals == 0))[0]
                holds, over = self.X(ch[pend], level - 1)
                vals[pend[holds]] = level
                gave_up |= bool(over.any())
                pend = pend[~holds]
                holds, over = self.W(ch[pend], level - 1)
                vals[pend[holds]] = -level
                gave_up |= bool(over.any())
            value, best = self.fold(moves, [int(v) for v in vals])
            if stop_early and value != 0:
                break
        return value, best, moves, [int(v) for v in vals], gave_up

    def solve(self, states, depth, all_moves=False):
        states = np.ascontiguousarray(states, np.uint8).reshape(-1, self.sb)
        k = len(states)
        out = dict(value=np.zeros(k, np.int8), best=np.zeros(k, np.uint16), counts=np.zeros(k, np.int32),
                   moves=np.zeros((k, TG_MAX_MOVES), np.uint16), move_values=np.zeros((k, TG_MAX_MOVES), np.int8),
                   nodes=np.zeros(k, np.uint64), budget_hit=np.zeros(k, np.uint8))
        for i in range(k):
            before = self.nodes
            value, best, moves, vals, gave_up = self.solve_one_full(states[i], depth, all_moves)
            c = len(moves)
            out["value"][i], out["best"][i], out["counts"][i] = value, best, c
            out["moves"][i, :c] = moves
            out["move_values"][i, :c] = vals
            out["nodes"][i] = self.nodes - before
            out["budget_hit"][i] = gave_up
        return out


def compare(ref, got, budget_free=True):
    """the comparison of the GPU tests: every field of FIELDS equal, row for row; with budget_free also budget_hit == 0.
    Returns the list of differences (empty = equal)."""
    bad = []
    for f in FIELDS:
        a, b = np.asarray(ref[f]), np.asarray(got[f])
        if a.shape != b.shape:
            bad.append(f"{f}: shape {a.shape} != {b.shape}")
            continue
        rows = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        if len(rows):
            bad.append(f"{f}: {len(rows)} rows differ, first {int(rows[0])}: expected {a[rows[0]].ravel()[:12]} got {b[rows[0]].ravel()[:12]}")
    if budget_free and "budget_hit" in got and np.asarray(got["budget_hit"]).any():
        bad.append(f"budget_hit set for {int(np.count_nonzero(got['budget_hit']))} positions")
    return bad


def compare_with_give_up(ref, got):
    """the comparison of the GPU tests on positions above a move list longer than TG_MAX_MOVES: every field of FIELDS and budget_hit
    equal, row for row (the node budget is set so high that only a cut list gives up)"""
    bad = compare(ref, got, budget_free=False)
    a, b = np.asarray(ref["budget_hit"]).astype(bool), np.asarray(got["budget_hit"]).astype(bool)
    if a.shape != b.shape or (a != b).any():
        bad.append(f"budget_hit: expected {a.astype(int)} got {b.astype(int)}")
    return bad


def sound(exact, got, depth):
    """the promise of include/takgpu.h on every row: a non-zero value has the sign of the exact value (the whole lists, no capacity,
    at the same depth) and a distance not below it — per position and per move.  → the list of violations"""
    bad = []
    for f in ("value", "move_values"):
        e, g = np.asarray(exact[f]).astype(np.int64), np.asarray(got[f]).astype(np.int64)
        wrong = (g != 0) & ((np.sign(g) != np.sign(e)) | (np.abs(g) < np.abs(e)))
        if wrong.any():
            r = np.argwhere(wrong)[0]
            bad.append(f"{f}: {int(wrong.sum())} unsound entries, first at {tuple(int(x) for x in r)}: exact {e[tuple(r)]} got {g[tuple(r)]}")
    return bad


def class_counts(values):
    """{proven value: positions}"""
    v, c = np.unique(np.asarray(values), return_counts=True)
    return {int(a): int(b) for a, b in zip(v, c)}


def require_classes(values, classes):
    """the condition of a test's set: at least 2 positions of every class the test claims to cover"""
    cc = class_counts(values)
    missing = {c: cc.get(c, 0) for c in classes if cc.get(c, 0) < 2}
    assert not missing, f"the set holds fewer than 2 positions of {missing}: {cc}"


def clip(out, depth):
    """an ALL_MOVES result at a larger depth cut down to `depth`: what ALL_MOVES at `depth` must give"""
    mv = np.where(np.abs(out["move_values"]) <= depth, out["move_values"], 0).astype(np.int8)
    r = Ref(5)  # (fold needs no board)
    o = dict(out, move_values=mv, value=out["value"].copy(), best=out["best"].copy())
    for i in range(len(mv)):
        c = int(out["counts"][i])
        o["value"][i], o["best"][i] = r.fold(out["moves"][i, :c], [int(x) for x in mv[i, :c]])
    return o


# ---- the position sets of the tests (each computed once per process) --------------------------------------------------
SETS = {
    "p5_400": lambda: oracle.playouts(5, 400, 7)["prev"],
    "r5_400": lambda: oracle.random_positions(5, 400, 3, 40),
    "p5_160": lambda: oracle.playouts(5, 160, 7)["prev"],
    "p6_200": lambda: oracle.playouts(6, 200, 7)["prev"],
    "p6_80": lambda: oracle.playouts(6, 80, 7)["prev"],
    "s5_200": lambda: oracle.playouts(5, 200, 11, style=3)["prev"],
}
BOARD = {"p5_400": 5, "r5_400": 5, "p5_160": 5, "p6_200": 6, "p6_80": 6, "s5_200": 5}

# the same positions one, two and three spreads away from the 50-reversible-plies draw (play-outs keep the counter far from 50):
# "<base>_r<counter>" is a prefix of <base> with the header's reversible_plies overwritten
REVERSIBLE = {"p5_400_r49": ("p5_400", 120, 49), "p5_400_r48": ("p5_400", 120, 48), "s5_200_r49": ("s5_200", 120, 49),
              "s5_200_r48": ("s5_200", 120, 48), "p6_200_r49": ("p6_200", 60, 49), "p6_200_r48": ("p6_200", 60, 48),
              "s5_200_r47": ("s5_200", 200, 47)}
for _name, (_base, _rows, _r) in REVERSIBLE.items():
    SETS[_name] = lambda b=_base, k=_rows, r=_r: posgen.with_header(positions(b)[:k], reversible_plies=r)
    BOARD[_name] = BOARD[_base]


@functools.lru_cache(maxsize=None)
def positions(name):
    a = SETS[name]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def reference(name, depth, all_moves, variant=None):
    out = Ref(BOARD[name], variant).solve(positions(name), depth, all_moves)
    for v in out.values():
        v.setflags(write=False)
    return out
