"""The network forward on positions that set every input plane (tests/posgen.py: repr_corner_states; tests/test_repr_corners.py shows
on the CPU what they cover and that the gates see a mistake in any plane).  Positions from random play leave the deep buried-stone
planes, the low reserve counts and a negative or odd komi unset, so the fused towers' own statement of game_repr — ws_row_mask +
tower_cb_board_quads for the board planes, tower_cb_table for the reserve / colour / fcd planes as a per-position bias per border
class — and layer 0's packed weight rows of those channels were reached by no gate.

Every row of every batch goes through check_forward against the float64 forward of oracle.encode's planes, and through the 1e-4 gate
against PyTorch fp32.  One batch size per kernel that stages packed states (the bracket edges are those of launch_tower_split:
TOWER_SPLIT_MAX_BATCH = 128 positions, half of it on 6×6; launch_tower_halo: above 1024 / 512 positions at 128 filters, k_tower_sq
above 2048 at 5×5×64; launch_s3: the halo image from 256 positions), the corner positions in the first workgroups and in the ragged
last one.  Then the corner positions past the forward: the search's root priors and the training step's gradients."""
import os
import re

import numpy as np
import pytest

import posgen
import torch_ref

pytestmark = pytest.mark.gpu

# (name, n, filters, head, precision, batch sizes — None = the corner set alone)
ROWS = [
    ("5x5x64_fc", 5, 64, "fc5", "f32", (96, 160, 2049)),        # k_tower_split (4 workgroups per position), k_tower, k_tower_sq
    ("5x5x128_fc", 5, 128, "fc5", "f32", (128, 129, 1025)),     # k_tower_split (8 per position), k_tower, k_tower_halo
    ("6x6x128_conv", 6, 128, "conv", "f32", (64, 65, 513)),     # k_tower_split, k_tower, k_tower_halo
    ("5x5x64_conv", 5, 64, "conv", "f32", (None,)),
    ("5x5x64_fc", 5, 64, "fc5", "bf16x3", (255, 256)),          # k_tower_s3, k_tower_s3_halo
    ("6x6x128_conv", 6, 128, "conv", "bf16x3", (255, 256)),
    ("3x3x32_conv", 3, 32, "conv", "f32", (None,)),             # the unfused path: k_encode (repr_value) + the conv kernels
    ("4x4x32_conv", 4, 32, "conv", "f32", (None,)),
    ("5x5x96_fc", 5, 96, "fc5", "f32", (None,)),
    ("6x6x32_conv", 6, 32, "conv", "f32", (None,)),
]
TAIL = 64
_corner_cache = {}


def _corners(orc, n):
    if n not in _corner_cache:
        _corner_cache[n] = posgen.repr_corner_states(orc, n)
    return _corner_cache[n]


def _engine(n, blocks, filters, head, max_batch, precision="f32"):
    import tak_amd

    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                       evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch)
    if precision != "f32":
        e.set_precision(precision)
    return e


def corner_batches(ncorner, B):
    """Index arrays into the pool (corner set first, positions from play behind it), each of exactly B rows.  B ≥ the corner set: ONE
    batch — the corner set, positions from play, and the corner set's first 64 again as the last rows, so that the ragged last workgroup
    holds corner positions.  A smaller B: the whole corner set in consecutive batches of B, the last one wrapping round to the first
    positions — every corner position passes through the kernel of that batch size, and every batch ends on corner positions."""
    if B >= ncorner:
        tail = min(TAIL, B - ncorner)
        return [np.concatenate([np.arange(ncorner), ncorner + np.arange(B - ncorner - tail), np.arange(tail)])]
    return [(a + np.arange(B)) % ncorner for a in range(0, ncorner, B)]


def gate_every_row(e, net, pool, ref, f32_ref, idx, precision, what, planes=None):
    """check_forward on EVERY row of the batch pool[idx] (tg_policy_eval on packed states; with `planes`, tg_forward_mcts on them) and
    the 1e-4 gate against PyTorch fp32 (tests/test_gpu_net.py).  → (probabilities, values, check_forward's metrics)"""
    p, v = e.policy_eval(pool[idx]) if planes is None else e.forward_mcts(planes[idx])
    p, v = np.ascontiguousarray(p, np.float32), np.asarray(v, np.float32).reshape(-1)
    assert p.shape[0] == len(idx) and np.isfinite(p).all() and np.isfinite(v).all()
    m = torch_ref.check_forward(p, v, torch_ref.slice_ref(ref, idx), precision, what)
    dp, dv = np.abs(p - f32_ref[0][idx]).max(), np.abs(v - f32_ref[1][idx]).max()
    assert dp <= 1e-4 and dv <= 1e-4, (what, "against PyTorch fp32", dp, dv)
    return p, v, m


def _worst(a, b):
    return b if a is None else {k: (max(a[k], b[k]) if isinstance(b[k], float) else b[k]) for k in b}


def test_split_tower_bracket_is_where_the_batch_sizes_assume_it():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tak_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"TOWER_SPLIT_MAX_BATCH\s*=\s*(\d+)", src).group(1)) == 128


@pytest.mark.parametrize("name,n,filters,head,precision,sizes", ROWS, ids=[f"{r[0]}_{r[4]}" for r in ROWS])
def test_forward_on_corner_positions_against_fp64(orc, name, n, filters, head, precision, sizes):
    corner, _ = _corners(orc, n)
    nc = len(corner)
    sizes = [nc if b is None else b for b in sizes]
    total = max(max(sizes), nc)
    pool = corner if total == nc else np.concatenate([corner, posgen.distinct_positions(orc, n, total - nc, seed=37)])
    planes = orc.encode(n, pool)
    net = torch_ref.make_net(n, 1, filters, head, seed=70 + n)  # BatchNorm folds randomised
    ref = torch_ref.forward64(net, planes)
    f32_ref = torch_ref.forward(net, planes)
    tag = f"corner set {name} {precision}"
    torch_ref.report(f"{tag} pytorch-f32, the {nc} corner rows", torch_ref.check_forward(f32_ref[0][:nc], f32_ref[1][:nc], torch_ref.slice_ref(ref, slice(0, nc)), "f32", "PyTorch fp32"))
    e = _engine(n, 1, filters, head, max(sizes), precision)
    e.load_state_dict(torch_ref.abi_tensors(net))
    bits_p, bits_v, fresh = None, None, np.zeros(nc, bool)  # a corner position's bits where it was first evaluated
    for B in sizes:
        seen = np.zeros(nc, bool)
        worst, worst_planes = None, None
        for idx in corner_batches(nc, B):
            assert len(idx) == B and (idx[-min(TAIL, B):] < nc).all()
            p, v, m = gate_every_row(e, net, pool, ref, f32_ref, idx, precision, f"{tag} states B={B}")
            worst = _worst(worst, m)
            if precision == "f32":  # a corner position's output does not depend on the batch, its row or the kernel
                c = idx < nc
                if bits_p is None:
                    bits_p, bits_v = np.zeros((nc, p.shape[1]), np.uint32), np.zeros(nc, np.uint32)
                first = c.copy()
                first[c] = ~fresh[idx[c]]
                bits_p[idx[first]], bits_v[idx[first]] = p.view(np.uint32)[first], v.view(np.uint32)[first]
                fresh[idx[first]] = True
                bad = np.flatnonzero(c)[(p.view(np.uint32)[c] != bits_p[idx[c]]).any(axis=1) | (v.view(np.uint32)[c] != bits_v[idx[c]])]
                assert not len(bad), (f"{tag} B={B}: corner positions whose bits depend on the batch", idx[bad][:8])
            seen[idx[idx < nc]] = True
            if B == min(sizes):  # the planes entry: layer 0 over all channels, no bias table
                worst_planes = _worst(worst_planes, gate_every_row(e, net, pool, ref, f32_ref, idx, precision, f"{tag} planes B={B}", planes=planes)[2])
        assert seen.all()
        torch_ref.report(f"{tag} policy_eval B={B}", worst)
        if worst_planes is not None:
            torch_ref.report(f"{tag} forward_mcts B={B}", worst_planes)
    e.close()


def test_search_root_priors_on_corner_positions(orc):
    """tg_search_reset + one iteration on the ongoing, consistent corner states: the states entry with the FC's gather epilogue"""
    import test_gpu_fp64

    n, filters, head = 5, 64, "fc5"
    corner, ok = _corners(orc, n)
    sts = corner[ok]
    net = torch_ref.make_net(n, 1, filters, head, seed=70 + n)
    ref = torch_ref.forward64(net, orc.encode(n, sts))
    e = _engine(n, 1, filters, head, len(sts))
    e.load_state_dict(torch_ref.abi_tensors(net))
    m = test_gpu_fp64.root_priors_against_fp64(orc, e, n, sts, ref, "f32", f"corner set priors, {len(sts)} roots")
    torch_ref.report(f"corner set 5x5x64_fc f32 search priors G={len(sts)}", m)
    e.close()


def corner_examples(orc, n, count, chunks=2, seed=5):
    """`chunks` chunks of `count` examples on ongoing, consistent corner states chosen so that every input plane is set in one of
    them (posgen.covering_subset), spread over the chunks in turn; move lists from the oracle, random visits, random results"""
    corner, ok = _corners(orc, n)
    sts = corner[ok]
    sts = sts[posgen.covering_subset(orc.encode(n, sts), chunks * count)]
    rng = np.random.default_rng(seed)
    out = []
    for c in range(chunks):
        part = sts[c::chunks]
        mv, cnt = orc.movegen(n, part)
        visits = np.where(np.arange(mv.shape[1])[None, :] < cnt[:, None], rng.integers(1, 50, mv.shape), 0).astype(np.uint32)
        results = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), len(part))
        out.append((part, cnt.astype(np.int32), mv, visits, results))
    return out


@pytest.mark.parametrize("n,filters,head", [(5, 64, "fc5"), (6, 128, "conv")])
def test_training_gradients_on_corner_positions(orc, n, filters, head):
    """the 2e-5 per-tensor gradient gate on examples whose planes are all set: on positions from play the gradient of conv0.weight is
    zero in the unset input channels on both sides, whatever layer 0's weight gradient does there"""
    import test_gpu_train

    count = 40
    examples = corner_examples(orc, n, count)
    net = torch_ref.make_net(n, 1, filters, head, seed=10 + n)
    g0 = 0.0
    for ex in examples:
        planes, pi, z, _ = test_gpu_train._targets(orc, n, head, ex)
        (g,), _ = torch_ref.fp64_gradients(net, planes, pi, z, [None])
        g0 = g0 + g["conv0.weight"]
    per_channel = np.abs(g0).max(axis=(0, 2, 3))
    assert per_channel.shape == (torch_ref.input_channels(n),) and (per_channel > 0).all(), np.flatnonzero(per_channel == 0)
    worst = test_gpu_train.chunk_gradients_against_fp64(orc, n, 1, filters, head, count, net=net, examples=examples)
    print(f"fp64-gate corner set training {n}x{n} 1x{filters} {head}, 2 x {count} examples: worst tensor {worst[0]} {worst[1]:.3e}; "
          f"smallest per-input-channel max |d conv0.weight| {per_channel.min():.3e}", flush=True)
