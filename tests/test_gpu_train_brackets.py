"""The training step (tg_train_chunk, tg_train_forward) at the chunk sizes where its launchers change kernels, and at ragged sizes in
between: tests/test_gpu_train.py's gradient gate — fp64 differentiated under the engine's own ReLU decisions, 2e-5 per tensor, 1e-5 on
the losses, no allowance for flipped decisions — swept over the brackets of conv_kernels.hip / fc_kernels.hip / train_kernels.hip.  test_gpu_train.CASES
runs that gate at 80 – 192 positions per chunk and at exactly 1024, with one residual block wherever the chunk is full; a chunk is
8 × examples positions, so an odd example count leaves the last workgroup of every whole-position kernel partly filled.

  topology          examples (positions)       what the size reaches
  5×5, 2 × 64, fc5  33 (264)                   k_conv_pos with 2 positions per workgroup
                    65 (520)                   k_conv_pos with 4 positions per workgroup
                    127 (1016)                 the last size below the halo image
                    129 (1032)                 k_conv_halo with a ragged last workgroup (64.5 × 16 positions): BatchNorm's Σz, Σz² from its
                                               accumulators, Σg, Σg·x̂ from the data gradient's epilogue, the in-place write, gskip across
                                               a block boundary
                    257 (2056)                 the top k_conv_pos bracket for layer 0, ragged; k_fc_ring<0> for the FC forward and
                                               k_fc_ring<1> for its data gradient (below: k_fc_small, k_gemm<2,1>), both with M % 128 = 8
  5×5, 2 × 128, fc5 33, 65, 127, 129, 257      the same thresholds on 128 filters; 129 and 257 leave a short last split to k_wgrad_halo
  6×6, 2 × 128, conv 33, 65, 127, 129          the 6×6 brackets at 256 and 512 positions; the halo 128 → 256 head layer at ≥ 1024; the
                                               wide-input data gradient of the head
  6×6, 1 × 128, conv 8, 16, 17 (64, 128, 136)  k_conv_split<3,8> for the head's forward at and just past its upper bound of 128 positions
  5×5, 1 × 128, conv 16, 17                    k_conv_split<2,8> for the head's forward AND its data gradient (Cpad = 128)

The only tensors outside the 2e-5 gate are the conv biases in front of a BatchNorm (true gradient zero: the absolute bound of
test_gpu_train).  The second test holds tg_train_forward at one size per row group against the fp64 training-mode forward of a
trained-like network, under the log-space gates of test_gpu_fp64.test_training_forward_against_fp64."""
import numpy as np
import pytest

import posgen
import test_gpu_train as T
import torch_ref

pytestmark = pytest.mark.gpu

# (n, blocks, filters, head, examples): positions = 8 × examples
GRADIENT_CASES = (
    [(5, 2, 64, "fc5", k) for k in (33, 65, 127, 129, 257)]
    + [(5, 2, 128, "fc5", k) for k in (33, 65, 127, 129, 257)]
    + [(6, 2, 128, "conv", k) for k in (33, 65, 127, 129)]
    + [(6, 1, 128, "conv", k) for k in (8, 16, 17)]
    + [(5, 1, 128, "conv", k) for k in (16, 17)]
)

FORWARD_CASES = [(5, 2, 64, "fc5", 33), (5, 2, 64, "fc5", 129), (5, 2, 64, "fc5", 257), (6, 1, 128, "conv", 17), (6, 2, 128, "conv", 129)]


def _id(c):
    return f"{c[0]}x{c[0]}_{c[1]}x{c[2]}_{c[3]}_{c[4]}"


@pytest.mark.parametrize("n,blocks,filters,head,count", GRADIENT_CASES, ids=[_id(c) for c in GRADIENT_CASES])
def test_chunk_gradients_at_the_launcher_brackets(orc, n, blocks, filters, head, count):
    name, worst = T.chunk_gradients_against_fp64(orc, n, blocks, filters, head, count)
    print(f"fp64-gate train_chunk {n}x{n} {blocks}x{filters} {head} {count} examples ({8 * count} positions): worst tensor {name} {worst:.3e}",
          flush=True)


@pytest.mark.parametrize("n,blocks,filters,head,count", FORWARD_CASES, ids=[_id(c) for c in FORWARD_CASES])
def test_training_forward_against_fp64_at_the_launcher_brackets(orc, n, blocks, filters, head, count):
    """tg_train_forward on a real chunk's batch — `count` distinct positions, augmented 8-fold as Example::to_tensors does — of a
    trained-like network, against the fp64 training-mode forward: check_logp and the value gate of test_training_forward_against_fp64"""
    sts = posgen.distinct_positions(orc, n, count, seed=31, max_plies=60)
    mv, cnt = orc.movegen(n, sts)
    rng = np.random.default_rng(count)
    visits = np.zeros((count, 512), np.uint32)
    for i in range(count):
        visits[i, : cnt[i]] = rng.integers(1, 50, cnt[i])
    results = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), count)
    planes, _, _, a_states = T._targets(orc, n, head, (sts, cnt.astype(np.int32), mv, visits, results))
    assert len(a_states) == 8 * count
    net = torch_ref.make_trained_net(n, blocks, filters, head, planes[:512], seed=29)
    e = T._engine(n, blocks, filters, head)
    e.load_state_dict(torch_ref.abi_tensors(net))
    e.train_create(chunk_size=count, chunks_in_step=1)
    logp, v = e.train_forward(a_states)
    ref = torch_ref.forward64(net, planes, training=True)
    what = f"train_forward {n}x{n} {blocks}x{filters} {head} B={8 * count}"
    m = torch_ref.check_logp(logp, ref, "f32", what)
    dv = np.abs(v.astype(np.float64) - ref["v"])
    m.update(pre=float((np.maximum(dv - 2.0 ** -23, 0) / (1 - ref["v"] ** 2)).max()), v_abs=float(dv.max()),
             v_max=float(np.abs(ref["v"]).max()), rows=8 * count)
    torch_ref.report(what + " f32", m)
    assert (dv <= torch_ref.GATES["f32"]["c"] * (1 - ref["v"] ** 2) + 2.0 ** -23).all(), m["pre"]
    e.close()
