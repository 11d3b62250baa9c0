"""Layer 0 of the exact-f32 states-entry towers is a sum of weight rows (tower_stage.cuh tower_cb_layer0): the per-position
constant-plane bias plus the folded conv0 weights of the board planes that are SET on a square's neighbours, no MFMA.  The four
kernels that own a layer 0 — k_tower_split, k_tower, k_tower_halo, k_tower_sq — call that one function, so a position must have the
same BITS in every bracket, row and column, and the sums must agree with the references that know nothing of the trick.

Inputs (tests/posgen.py): the empty board and a board with every square occupied under both sides to move, very tall stacks, the
positions that set every input plane on corner, edge and interior squares (every (plane, tap) row of the weights is read), and a few
hundred distinct positions from play.  They come first in every batch, and their head comes again as the batch's last rows: in the
ragged last workgroup, at a column shifted against the first pass.  A set larger than the bracket goes through it in consecutive
batches, each ending on the set's head.

Per topology one batch inside k_tower_split's range, one mid-size batch on k_tower and the smallest batch of the full-batch kernel
(2049: k_tower_sq; 1025 / 513: k_tower_halo), with 0 and 1 residual blocks.  Every batch: np.array_equal on the uint32 views of policy
and value against the bits of the first bracket; torch_ref.check_forward against the float64 forward with the existing f32 gates and
the 1e-4 gate against PyTorch fp32; and the planes entry (tg_forward_mcts: every plane through the dense MFMA layer 0, an
independent implementation) to ≤ 1e-6, as tests/test_gpu_net.py test_golden_fixture asserts it."""
import numpy as np
import pytest

import posgen
import torch_ref

pytestmark = pytest.mark.gpu

# (name, n, filters, head, batch sizes: k_tower_split, k_tower, the full-batch kernel)
TOPOLOGIES = [
    ("5x5x64_fc", 5, 64, "fc5", (96, 700, 2049)),
    ("5x5x128_fc", 5, 128, "fc5", (100, 600, 1025)),
    ("6x6x128_conv", 6, 128, "conv", (32, 300, 513)),
]
_pools = {}


def _pool(orc, n, total):
    """(positions, planes, size of the special set in front) — computed once per board size"""
    if n not in _pools:
        special = np.stack([posgen.empty_board(n, 0), posgen.empty_board(n, 1), posgen.full_board(n, 0), posgen.full_board(n, 1)])
        tall = posgen.tall_stack_states(n, 24, seed=5)
        corner, _ = posgen.repr_corner_states(orc, n)
        play = posgen.distinct_positions(orc, n, 300, seed=31)
        front = np.concatenate([special, tall, corner, play])
        fill = posgen.distinct_positions(orc, n, max(total - len(front), 64), seed=43)
        sts = np.concatenate([front, fill])
        _pools[n] = (sts, orc.encode(n, sts), len(front))
    sts, planes, k = _pools[n]
    assert len(sts) >= total
    return sts, planes, k


def _tail(B):
    """rows of a batch's end that repeat the set's head: a few dozen, and a start that is no multiple of a workgroup's 4 / 8 / 16 positions"""
    return next(t for t in range(37, 41) if (B - t) % 4 != 0)


def batches(k, B):
    """index arrays of exactly B rows into the pool.  B > k + tail: one batch — the special set, positions from play, the set's head
    again.  Smaller: the set in consecutive runs, each batch ending on the set's head."""
    t = _tail(B) if B > 64 else 5
    if B >= k + t:
        return [np.concatenate([np.arange(k), k + np.arange(B - k - t), np.arange(t)])]
    step = B - t
    return [np.concatenate([(a + np.arange(step)) % k, np.arange(t)]) for a in range(0, k, step)]


def test_batches_cover_the_set_and_end_on_its_head():
    for k, B in ((700, 96), (700, 32), (500, 2049), (500, 513)):
        bs = batches(k, B)
        seen = np.zeros(k, bool)
        for idx in bs:
            t = _tail(B) if B > 64 else 5
            assert len(idx) == B and list(idx[-t:]) == list(range(t)) and (B - t) % 4 != 0
            seen[idx[idx < k]] = True
        assert seen.all()


@pytest.mark.parametrize("blocks", [0, 1])
@pytest.mark.parametrize("name,n,filters,head,sizes", TOPOLOGIES, ids=[t[0] for t in TOPOLOGIES])
def test_same_bits_in_every_bracket_and_the_references_agree(orc, name, n, filters, head, sizes, blocks):
    import tak_amd

    total = max(sizes)
    sts, planes, k = _pool(orc, n, 2049 if n == 5 else 513)
    sts, planes = sts[:total], planes[:total]
    k = min(k, total - 64)
    net = torch_ref.make_net(n, blocks, filters, head, seed=90 + 7 * n + blocks)  # BatchNorm folds randomised
    ref = torch_ref.forward64(net, planes)
    f32_ref = torch_ref.forward(net, planes)
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                       evaluator=tak_amd.EVAL_RESNET, max_batch=total)
    e.load_state_dict(torch_ref.abi_tensors(net))
    bits_p, bits_v, have = None, None, np.zeros(total, bool)
    for B in (sizes[1], sizes[0], sizes[2]):  # the bits of the mid-size k_tower batch first
        for idx in batches(k, B):
            what = f"sparse layer 0 {name} blocks {blocks} B={B}"
            p, v = e.policy_eval(sts[idx])
            p, v = np.ascontiguousarray(p, np.float32), np.asarray(v, np.float32).reshape(-1)
            assert p.shape[0] == B and np.isfinite(p).all() and np.isfinite(v).all()
            # ---- the references ----
            m = torch_ref.check_forward(p, v, torch_ref.slice_ref(ref, idx), "f32", what)
            dp, dv = np.abs(p - f32_ref[0][idx]).max(), np.abs(v - f32_ref[1][idx]).max()
            p2, v2 = e.forward_mcts(planes[idx])
            ep, ev = np.abs(p - p2).max(), np.abs(v - np.asarray(v2, np.float32).reshape(-1)).max()
            print(f"{what}: against PyTorch fp32 {dp:.3g} / {dv:.3g}, against the planes entry {ep:.3g} / {ev:.3g}")
            assert dp <= 1e-4 and dv <= 1e-4, (what, "against PyTorch fp32", dp, dv)
            assert ep <= 1e-6 and ev <= 1e-6, (what, "against the planes entry", ep, ev)
            # ---- the bits: a position's output depends on no batch, row, column or kernel ----
            pu, vu = p.view(np.uint32), v.view(np.uint32)
            if bits_p is None:
                bits_p, bits_v = np.zeros((total, p.shape[1]), np.uint32), np.zeros(total, np.uint32)
            first = np.zeros(B, bool)
            first[np.unique(idx, return_index=True)[1]] = True
            first &= ~have[idx]
            bits_p[idx[first]], bits_v[idx[first]] = pu[first], vu[first]
            have[idx[first]] = True
            bad = np.flatnonzero((pu != bits_p[idx]).any(axis=1) | (vu != bits_v[idx]))
            assert not len(bad), (what, "positions whose bits depend on the batch", idx[bad][:8], bad[:8])
        torch_ref.report(what, m)
    assert have[:k].all()
    e.close()
