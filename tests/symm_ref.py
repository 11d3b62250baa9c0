"""Independent statements behind the symmetry tests (tg_policy_eval_symm, TG_SYMM_HASHED).  A plain module, like rng_ref.py and
posgen.py.  Nothing here is transcribed from tak_amd/csrc: the permutation tables come out of oracle.augment (Example::to_tensors
over tak/src/symm.rs:11-20), the hashed image out of oracle.state_hash and Philox as rng_ref states it, the fold is f32 numpy.

  perm[s][j]        the policy slot of the image under s of the move whose slot is j
  fold              policy[i][j] = (Σ_s p_s[i][perm[s][j]]) · (1/k), eval[i] = (Σ_s v_s[i]) · (1/k): f32, ascending s, the first
                    selected image starts the sum, the product with the f32 constant 1/k comes last (include/takgpu.h)
  hashed_symmetry   s = philox(seed; hash_lo, hash_hi, "symm", 0)[0] & 7, hash = oracle.state_hash of the packed state
"""
import functools

import numpy as np

import rng_ref

SYMM_TAG = int.from_bytes(b"symm", "big")  # 0x73796d6d: the third counter word of the hashed image
TG_MAX_MOVES = 512


def slot_moves(n, head_fc5, orc):
    """every move code that has a policy slot.  Conv formula (move_map.rs:19-48): placements of the three pieces and, per direction,
    the spread patterns 1 … 2^n − 2 in the top n bits of the pattern byte; the legacy 5×5 table: the codes oracle.move_index knows."""
    codes = []
    for sq in range(n * n):
        codes += [sq | (f << 6) for f in range(3)]
        codes += [sq | (d << 6) | ((v << (8 - n)) << 8) for d in range(4) for v in range(1, (1 << n) - 1)]
    codes = np.array(codes, np.uint16)
    if head_fc5:
        assert n == 5
        codes = codes[orc.move_index(5, codes) >= 0]
    return codes


def _image_slots(orc, n, head, state, moves):
    """slot of every listed move in each of the 8 images → int array [8, len(moves)] (−1: the image has no slot).  Through
    oracle.augment: visits k + 1 on move k, so round(pi · total) − 1 names the move a target entry belongs to."""
    c = len(moves)
    assert 0 < c <= TG_MAX_MOVES
    mv = np.zeros((1, TG_MAX_MOVES), np.uint16)
    vs = np.zeros((1, TG_MAX_MOVES), np.uint32)
    mv[0, :c] = moves
    vs[0, :c] = np.arange(1, c + 1)
    total = float(vs.sum())
    _, pi = orc.augment(n, head, state[None], np.array([c], np.int32), mv, vs)
    out = np.full((8, c), -1, np.int64)
    for s in range(8):
        nz = np.flatnonzero(pi[s])
        k = np.rint(pi[s, nz].astype(np.float64) * total).astype(np.int64) - 1
        assert len(set(k.tolist())) == len(k), "two moves of one list share a slot"
        out[s, k] = nz
    return out


def perm_from_moves(orc, n, head, state, moves, perm=None):
    """enter the moves' images into perm [8, P] (−1 = not seen yet); an entry seen twice must agree"""
    P = orc.policy_size(n, head)
    if perm is None:
        perm = np.full((8, P), -1, np.int64)
    for lo in range(0, len(moves), TG_MAX_MOVES):
        slots = _image_slots(orc, n, head, state, moves[lo: lo + TG_MAX_MOVES])
        j = slots[0]
        assert (j >= 0).all()
        for s in range(8):
            seen = perm[s, j] >= 0
            assert np.array_equal(perm[s, j][seen], slots[s][seen]), s
            perm[s, j] = slots[s]
    return perm


@functools.lru_cache(maxsize=None)
def _perm_tables_cached(n, fc5):
    from oracle import oracle as orc

    head = orc.HEAD_FC5 if fc5 else orc.HEAD_CONV
    return perm_from_moves(orc, n, head, orc.new_game(n), slot_moves(n, fc5, orc))


def perm_tables(n, fc5):
    """[8, P] from the enumeration of all slots (cached: shared by the tests, never modified — callers get a copy)"""
    return _perm_tables_cached(n, bool(fc5)).copy()


def square_map(n, s):
    """square index → square index under symmetry s as symm.rs orders them: s < 4 is rotate^s, s ≥ 4 mirror then rotate^(s − 4);
    rotate (col, row) → (row, n − 1 − col), mirror col → n − 1 − col"""
    out = np.zeros(n * n, np.int64)
    for sq in range(n * n):
        col, row = sq % n, sq // n
        if s >= 4:
            col = n - 1 - col
        for _ in range(s & 3):
            col, row = row, n - 1 - col
        out[sq] = row * n + col
    return out


def composition(n=5):
    """comp[s][t] = the symmetry that is t followed by s, from the square maps (they are faithful: 8 different maps)"""
    maps = [square_map(n, s) for s in range(8)]
    comp = np.zeros((8, 8), np.int64)
    for s in range(8):
        for t in range(8):
            both = maps[s][maps[t]]
            (u,) = [u for u in range(8) if np.array_equal(maps[u], both)]
            comp[s, t] = u
    return comp


def image_states(orc, n, head, states):
    """[k, 8, bytes]: the 8 images of every state, oracle.augment's"""
    states = np.ascontiguousarray(states, np.uint8).reshape(-1, states.shape[-1])
    k = len(states)
    mv = np.zeros((k, TG_MAX_MOVES), np.uint16)
    vs = np.zeros((k, TG_MAX_MOVES), np.uint32)
    vs[:, 0] = 1
    out, _ = orc.augment(n, head, states, np.ones(k, np.int32), mv, vs)
    return out.reshape(k, 8, -1)


def selected(mask):
    return [s for s in range(8) if (mask >> s) & 1]


def fold(p, v, perm, mask, order="ascending", divide="last"):
    """p [k_images, P], v [k_images] of ONE state's selected images in ascending s → (policy [P], eval) in the stated order.
    order = "descending" and divide = "first" are the two wrong folds the tests show the reference to reject."""
    sel = selected(mask)
    k = len(sel)
    inv = np.float32(1.0) / np.float32(k)
    rows = [(p[r][perm[s]].astype(np.float32), np.float32(v[r])) for r, s in enumerate(sel)]
    if order == "descending":
        rows = rows[::-1]
    if divide == "first":
        rows = [(a * inv, b * inv) for a, b in rows]
    acc_p, acc_v = rows[0]
    for a, b in rows[1:]:
        acc_p = (acc_p + a).astype(np.float32)
        acc_v = np.float32(acc_v + b)
    if divide == "last":
        acc_p, acc_v = (acc_p * inv).astype(np.float32), np.float32(acc_v * inv)
    return acc_p, acc_v


def fold_batch(engine_eval, orc, n, head, states, perm, mask, **kw):
    """the ensemble of every state from `engine_eval(states) → (p, v)` (tg_policy_eval) on oracle.augment's images"""
    img = image_states(orc, n, head, states)
    sel = selected(mask)
    p, v = engine_eval(img[:, sel].reshape(-1, img.shape[-1]))
    p = p.reshape(len(img), len(sel), -1)
    v = v.reshape(len(img), len(sel))
    out = [fold(p[i], v[i], perm, mask, **kw) for i in range(len(img))]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out], np.float32)


def hashed_symmetry(orc, n, states, seed):
    """s of every state [k]: Philox (rng_ref's statement) keyed by the seed over (hash_lo, hash_hi, "symm", 0), word 0, low 3 bits"""
    states = np.ascontiguousarray(states, np.uint8).reshape(-1, states.shape[-1])
    h = np.array([orc.state_hash(n, st) for st in states], np.uint64)
    w = rng_ref.philox_np(seed, h & np.uint64(rng_ref.M32), h >> np.uint64(32), SYMM_TAG, 0)
    return (w[:, 0] & np.uint32(7)).astype(np.int64)


class HashedEvaluator:
    """py_eval for oracle.Search / oracle.SelfPlay: the network sees the hashed image of every leaf, the policy comes back through
    the permutation.  `transformed` counts the states evaluated under s ≠ 0."""

    def __init__(self, orc, n, head, engine_eval, perm, seed):
        self.orc, self.n, self.head, self.eval, self.perm, self.seed = orc, n, head, engine_eval, perm, seed
        self.transformed = 0

    def __call__(self, states):
        s = hashed_symmetry(self.orc, self.n, states, self.seed)
        self.transformed += int((s != 0).sum())
        img = image_states(self.orc, self.n, self.head, states)
        p, v = self.eval(img[np.arange(len(s)), s])
        return np.stack([p[i][self.perm[s[i]]] for i in range(len(s))]), v
