"""Reference for the road-only forced-win solver (TG_SOLVE_ROAD_ONLY, the tinuë): tactics_ref.Ref with ONE thing changed, the
meaning of "wins" — a road of that colour and nothing else.  W, X, lost_at_once, the move values, the fold and the early stop are
tactics_ref's own and follow from it: a move that ends the game by flats or in a draw is neither a win in W nor a loss in X nor
ongoing, so it proves nothing.  Nothing here follows the kernels' structure.

`Planted(n, variant)` is TinueRef with one deliberate mistake of this mode (VARIANTS); tests/test_tinue_ref.py checks that
tactics_ref.compare, the comparison of the GPU tests, rejects each of them."""
import functools
import json
import os

import numpy as np

import tactics_ref as T
from oracle import oracle

TG_SOLVE_ROAD_ONLY = 4
VARIANTS = ("flats_win_at_last_ply", "flats_lose_in_x", "flat_loss_is_ongoing")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class TinueRef(T.Ref):
    @staticmethod
    def won(res, color):
        return np.where(color == 0, res == 1, res == 3)


class Planted(TinueRef):
    """TinueRef with one deliberate mistake; each leaves `won` alone and bends one place that uses it"""

    def __init__(self, n, variant):
        assert variant in VARIANTS
        super().__init__(n)
        self.mistake = variant

    def W(self, S, L):
        if self.mistake == "flats_win_at_last_ply" and L == 1 and 0 < len(S) <= self.CHUNK:  # the attacker's last ply counts flats again
            self.__dict__["won"] = T.Ref.won
            try:
                return super().W(S, L)
            finally:
                del self.__dict__["won"]
        return super().W(S, L)

    def lost_at_once(self, res, m):
        lost = super().lost_at_once(res, m)
        if self.mistake == "flats_lose_in_x":
            lost = lost | T.Ref.won(res, m ^ 1)
        return lost

    def play(self, S, moves):
        ch, res = super().play(S, moves)
        if self.mistake == "flat_loss_is_ongoing":  # a flat win of the side that did not move is searched on as if the game went on
            res = np.where(res == np.where(self.mover(S) == 0, 4, 2), 0, res).astype(res.dtype)
        return ch, res


# ---- the position sets: tactics_ref's play-out sets (where the two modes disagree) and the committed mined positions ---------------
@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(os.path.join(GOLDEN, "tinue_positions.npz")) as z:
        out = {k: z[k] for k in z.files}
    for a in out.values():
        a.setflags(write=False)
    return out


BOARD = dict(T.BOARD, m5_400=5, m6_200=6)


def positions(name):
    """"m5_400" / "m6_200": the committed mined positions (tests/golden/make_tinue_cases.py); every other name: tactics_ref's"""
    if name in ("m5_400", "m6_200"):
        return _npz()[name]
    return T.positions(name)


@functools.lru_cache(maxsize=None)
def reference(name, depth, all_moves, variant=None, road_only=True):
    ref = (Planted(BOARD[name], variant) if variant else TinueRef(BOARD[name])) if road_only else T.Ref(BOARD[name])
    out = ref.solve(positions(name), depth, all_moves)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def cases():
    with open(os.path.join(GOLDEN, "tinue_cases.json")) as f:
        return json.load(f)


def table(block, depth):
    """→ (states, the committed early-stop road-only table) of the cases of `block` ("five" / "six") that carry `depth`"""
    b = cases()[block]
    cs = [c for c in b["cases"] if f"depth{depth}" in c]
    k = len(cs)
    ref = dict(value=np.zeros(k, np.int8), best=np.zeros(k, np.uint16), counts=np.zeros(k, np.int32),
               moves=np.zeros((k, T.TG_MAX_MOVES), np.uint16), move_values=np.zeros((k, T.TG_MAX_MOVES), np.int8))
    for j, c in enumerate(cs):
        e = c[f"depth{depth}"]
        ref["value"][j], ref["best"][j], ref["counts"][j] = e["value"], e["best"], c["counts"]
        ref["moves"][j, : c["counts"]] = c["moves"]
        ref["move_values"][j, : c["counts"]] = e["move_values"]
    return positions(b["set"])[[c["index"] for c in cs]], ref


class RefSolver:
    """the reference behind the two calls analysis.forced_line makes on an Engine (solve and play), on the oracle's rules"""

    def __init__(self, n):
        self.n = n

    def solve(self, states, depth, node_budget=0, road_only=False):
        return (TinueRef(self.n) if road_only else T.Ref(self.n)).solve(states, depth, False)

    def play(self, states, moves):
        return oracle.play(self.n, states, moves)
