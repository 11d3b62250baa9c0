"""Layer 0 of the square-tile tower (k_tower_sq: 5×5, 64 filters, more than 2048 positions) runs on square tiles — the board planes
staged straight into the square-tile image, the MFMAs of on-board taps only, the border class of the per-position bias a constant of
the tile.  Every output keeps its chain over (tap, chunk, k) minus additions of exact zeros, so a position evaluated in a batch of
4096, 4090 (ragged last workgroup) or 2049 (the smallest square-tile batch) must have the BITS it has in a batch of 2048, which runs
k_tower on the plain image with per-tap masks.  Inputs: distinct positions from play, plus the ones on which layer 0's planes are
all zero or dense — the empty board, a board with every square occupied, very tall stacks.  No tolerance."""
import numpy as np
import pytest

import posgen
import torch_ref

pytestmark = pytest.mark.gpu
N = 5
PLAIN = 2048  # largest batch of the plain-image bracket


def _positions(orc, total):
    special = np.stack([posgen.empty_board(N, 0), posgen.empty_board(N, 1), posgen.full_board(N, 0), posgen.full_board(N, 1)])
    tall = posgen.tall_stack_states(N, 60, seed=5)
    play = posgen.distinct_positions(orc, N, total - len(special) - len(tall), seed=31)
    sts = np.concatenate([play, special, tall])
    # the special inputs in the first workgroups, in the middle and in the ragged tail of every batch size used below
    perm = np.random.default_rng(17).permutation(total)
    sts = sts[perm]
    sts[:4], sts[2044:2048], sts[4086:4090] = special, special, special
    return sts


@pytest.mark.parametrize("blocks", [6, 0, 1])
def test_square_tile_layer0_keeps_the_bits_of_the_plain_image_tower(orc, blocks):
    import tak_amd

    total = 4096
    sts = _positions(orc, total)
    net = torch_ref.make_net(N, blocks, 64, "fc5", seed=40 + blocks)  # BatchNorm folds randomised
    e = tak_amd.Engine(N, res_blocks=blocks, filters=64, policy_head=tak_amd.HEAD_FC5, evaluator=tak_amd.EVAL_RESNET, max_batch=total)
    e.load_state_dict(torch_ref.abi_tensors(net))
    # reference: the same positions in batches of 2048 (k_tower, plain image)
    ref = [e.policy_eval(sts[a: a + PLAIN]) for a in range(0, total, PLAIN)]
    p_ref = np.concatenate([r[0] for r in ref]).view(np.uint32)
    v_ref = np.concatenate([np.asarray(r[1], np.float32).reshape(-1) for r in ref]).view(np.uint32)
    assert np.isfinite(p_ref.view(np.float32)).all() and np.isfinite(v_ref.view(np.float32)).all()
    for batch in (4096, 4090, 2049):
        p, v = e.policy_eval(sts[:batch])
        p = np.ascontiguousarray(p, np.float32).view(np.uint32)
        v = np.asarray(v, np.float32).reshape(-1).view(np.uint32)
        bad_p = np.flatnonzero((p != p_ref[:batch]).any(axis=1))
        bad_v = np.flatnonzero(v != v_ref[:batch])
        print(f"blocks {blocks} batch {batch}: {len(bad_p)} policy rows, {len(bad_v)} values differ from the batches of {PLAIN}")
        assert np.array_equal(p, p_ref[:batch]), (batch, bad_p[:8])
        assert np.array_equal(v, v_ref[:batch]), (batch, bad_v[:8])
    # a second full batch whose tail holds the first one's head: a position's bits do not depend on its column either
    p2, v2 = e.policy_eval(np.roll(sts, 5, axis=0))
    assert np.array_equal(np.roll(np.ascontiguousarray(p2, np.float32).view(np.uint32), -5, axis=0), p_ref)
    assert np.array_equal(np.roll(np.asarray(v2, np.float32).reshape(-1).view(np.uint32), -5), v_ref)
    e.close()
