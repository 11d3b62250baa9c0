"""Reference for tg_eval_examples (shared by tests/test_eval_examples_cpu.py and tests/test_gpu_eval_examples.py): seeded examples
with the forced edge cases, and the row values of the eval-mode network in a chosen precision — PyTorch on the CPU, log_softmax over
all P outputs, π = visits / Σ visits at oracle.move_index of the (transformed) move, images from oracle.augment.

Gates (the repository's rule for value gates: the larger of a floor and 3 × PyTorch f32's own worst distance to fp64 on the same
rows).  The floors are a few dozen f32 roundings at the magnitude of the quantity, not a fit to any engine result:
  loss_p  is ≈ log P (7.4 on 5×5, 9.1 on 6×6) on these flat networks: ulp 4.8e-7 … 9.5e-7; 2e-5 ≈ 20 … 40 ulps
  v       |v| < 1: ulp ≤ 6e-8; 2e-6 ≈ 32 ulps of a tanh whose pre-activation is a dot product of 800 … 4608 terms
  loss_z  (z − v)² ≤ 4 with derivative 2 |z − v| ≤ 4: four times v's floor, 8e-6
"""
import os

import numpy as np
import torch

import torch_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLOORS = {"loss_p": 2e-5, "loss_z": 8e-6, "v": 2e-6}
MARGIN = 1e-4        # top-1 / sign are compared only where the fp64 margin clears this
MAX_LEFT_OUT = 0.05  # … and at most this share of the rows may be left out
TG_MAX_MOVES = 512
UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3


def golden_net(name):
    """(net, n, blocks, filters, head) of tests/golden/<name>.npz, built as tests/test_gpu_net.py builds it"""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    n, blocks, filters, head_i, seed = [int(v) for v in z["meta"]]
    head = "fc5" if head_i == 0 else "conv"
    return torch_ref.make_net(n, blocks, filters, head, seed=seed), n, blocks, filters, head


def make_examples(orc, n, count, seed):
    """`count` examples on ongoing positions of oracle.random_positions (plies 0 … 60), oracle.movegen lists, seeded visits.
    Forced: example 0 has ONE visited move (one-hot); example 1 every move visited once (an exact tie: the first one wins);
    example 2 sits on the position with the fewest moves of the sample, example 3 on the one with the most; results cycle
    +1, −1, 0.  → dict(states, n_moves, moves, visits, results)."""
    rng = np.random.default_rng(seed)
    pool = orc.random_positions(n, 4 * count + 64, seed=seed, max_plies=60, half_komi=4)
    pool = pool[orc.result(n, pool) == 0]
    moves, counts = orc.movegen(n, pool)
    assert len(pool) >= count and counts.min() >= 1
    order = list(range(len(pool)))
    lo, hi = int(np.argmin(counts)), int(np.argmax(counts))
    rest = [i for i in order if i not in (lo, hi)]
    pick = (rest[:2] + [lo, hi] + rest[2:])[:count] if count >= 4 else rest[:count]
    states, moves, counts = pool[pick], moves[pick], counts[pick].astype(np.int32)
    visits = np.zeros((count, TG_MAX_MOVES), np.uint32)
    for i in range(count):
        c = int(counts[i])
        v = rng.integers(0, 40, c) * (rng.random(c) < 0.6)  # sparse, with repeated counts
        if v.sum() == 0:
            v[rng.integers(0, c)] = 7
        visits[i, :c] = v
    c0 = int(counts[0])
    visits[0, :] = 0
    visits[0, c0 // 2] = 11
    if count > 1:
        visits[1, :] = 0
        visits[1, : counts[1]] = 1
    results = np.array([(1.0, -1.0, 0.0)[i % 3] for i in range(count)], np.float32)
    return dict(states=states, n_moves=counts, moves=moves, visits=visits, results=results)


def take(ex, sel):
    return {k: v[sel] for k, v in ex.items()}


def args(ex):
    return ex["states"], ex["n_moves"], ex["moves"], ex["visits"], ex["results"]


def sym_move(n, s, mv):
    """move code under symmetry s of tak/src/symm.rs: rotate (col, row) → (row, n−1−col), mirror col → n−1−col; s < 4 is
    rotate^s, s ≥ 4 mirror then rotate^(s−4); spread directions follow the squares"""
    sq, f, pat = mv & 63, (mv >> 6) & 3, mv >> 8
    col, row = sq % n, sq // n
    if s >= 4:
        col = n - 1 - col
    for _ in range(s & 3):
        col, row = row, n - 1 - col
    if pat:
        if s >= 4:
            f = {LEFT: RIGHT, RIGHT: LEFT}.get(f, f)
        for _ in range(s & 3):
            f = {UP: RIGHT, RIGHT: DOWN, DOWN: LEFT, LEFT: UP}[f]
    return (row * n + col) | (f << 6) | (pat << 8)


def positions(orc, n, head, ex, symmetries):
    """(states, idx [positions × TG_MAX_MOVES] policy index of every listed move, example of every position) — with symmetries
    the 8 images of oracle.augment, position 8 i + s; the python move transform is checked against the oracle's dense targets"""
    k = len(ex["n_moves"])
    if not symmetries:
        idx = orc.move_index(n, ex["moves"]).reshape(k, TG_MAX_MOVES)
        return ex["states"], idx, np.arange(k)
    states8, pi8 = orc.augment(n, orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV, ex["states"], ex["n_moves"], ex["moves"], ex["visits"])
    tm = np.zeros((8 * k, TG_MAX_MOVES), np.uint16)
    for i in range(k):
        for s in range(8):
            tm[8 * i + s, : ex["n_moves"][i]] = [sym_move(n, s, int(m)) for m in ex["moves"][i, : ex["n_moves"][i]]]
    idx = orc.move_index(n, tm).reshape(8 * k, TG_MAX_MOVES)
    owner = np.repeat(np.arange(k), 8)
    for p in range(8 * k):
        c = ex["n_moves"][owner[p]]
        v = ex["visits"][owner[p], :c]
        dense = np.zeros(pi8.shape[1], np.float32)
        dense[idx[p, :c]] = v.astype(np.float32) / np.float32(v.sum())
        assert np.array_equal(dense, pi8[p]), f"move transform disagrees with oracle.augment at position {p}"
    return states8, idx, owner


@torch.no_grad()
def reference_rows(orc, net, n, head, ex, symmetries, dtype=torch.float64):
    """Row values of the eval-mode network (running statistics) in `dtype` → dict of float64 arrays over positions:
    loss_p, loss_z, v, entropy, top1 (0 / 1), z, and the margins logit_margin (best − second best LISTED logit; inf with one
    move) and |v|.  Arg-maxes over the listed moves in list order, the first maximum wins."""
    states, idx, owner = positions(orc, n, head, ex, symmetries)
    planes = orc.encode(n, states)
    m = __import__("copy").deepcopy(net).to(dtype).eval()
    logp, v = m.forward_training(torch.from_numpy(np.ascontiguousarray(planes)).to(dtype))
    logp, v = logp.double().numpy(), v[:, 0].double().numpy()
    out = {k: np.zeros(len(states)) for k in ("loss_p", "loss_z", "v", "entropy", "top1", "z", "logit_margin")}
    for p in range(len(states)):
        i = owner[p]
        c = int(ex["n_moves"][i])
        vis = ex["visits"][i, :c].astype(np.float64)
        pi = vis / vis.sum()
        l = logp[p, idx[p, :c]]
        nz = pi > 0
        out["loss_p"][p] = -(pi[nz] * l[nz]).sum()
        out["entropy"][p] = -(pi[nz] * np.log(pi[nz])).sum()
        out["top1"][p] = float(int(np.argmax(l)) == int(np.argmax(vis)))
        srt = np.sort(l)
        out["logit_margin"][p] = srt[-1] - srt[-2] if c > 1 else np.inf
        out["z"][p] = ex["results"][i]
    out["v"] = v
    out["loss_z"] = (out["z"] - v) ** 2
    return out


def distances(rows, ref):
    """worst |Δ| per gated quantity of `rows` (dict or [positions × 4] engine rows) against the fp64 `ref`"""
    if not isinstance(rows, dict):
        rows = {"loss_p": rows[:, 0], "loss_z": rows[:, 1], "v": rows[:, 3]}
    return {k: float(np.abs(np.asarray(rows[k], np.float64) - ref[k]).max()) for k in ("loss_p", "loss_z", "v")}


def bounds(d32):
    return {k: max(FLOORS[k], 3.0 * d32[k]) for k in FLOORS}


def clear_rows(ref):
    """rows whose fp64 margins clear MARGIN: (top-1 comparable, sign comparable)"""
    return ref["logit_margin"] > MARGIN, np.abs(ref["v"]) > MARGIN


def f64_sums(rows):
    """the f64 sums of [positions × 4] float32 rows, one after the other in position order"""
    s = [0.0, 0.0]
    for r in rows:
        s[0] += float(r[0])
        s[1] += float(r[1])
    return s
