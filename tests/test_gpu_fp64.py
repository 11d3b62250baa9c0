"""The network forward against float64 on networks that look trained (tests/torch_ref.py: make_trained_net, forward64, check_forward):
peaked policies, |v| up to 0.9999, BatchNorm channels with running variance of the order of eps.  PyTorch fp32 with |Δp| ≤ 1e-4 cannot
see a dropped bias or a per-mille mis-scale on make_net's flat policies; these gates can (tests/test_forward_gates.py shows it on the CPU).

Every topology the engine dispatches on, both precisions where the split-bf16 path exists, both entry points (tg_policy_eval on packed
states, tg_forward_mcts on planes), one batch size per launcher bracket of tower_kernels.hip, conv_kernels.hip and fc_kernels.hip (k_tower_split ≤ 128 / ≤ 64 on 6×6 — the
states entry only —, the k_tower brackets ≤ 256 / 512 / 1024 / 2048, k_tower_halo above, k_fc_small ≤ 2048 rows against k_fc_ring,
k_conv_split against k_conv_pos for the conv head, the k_fc_s3 ring above 512 rows) plus ragged sizes; the priors the search computes
in its tree backup (softmax.cuh's block statistics) against p64[move_index]; the training forward against the fp64 training-mode forward."""
import numpy as np
import pytest

import posgen
import torch_ref

pytestmark = pytest.mark.gpu

# (name, n, blocks, filters, head, precisions, batch sizes): the largest size is the batch the fp64 reference is computed on
SWEEP = [
    ("c2_5x5x64_fc", 5, 2, 64, "fc5", ("f32", "bf16x3"), (1, 37, 64, 128, 129, 256, 257, 512, 1024, 1025, 2048, 2049, 2400)),
    ("c5_5x5x128_fc", 5, 2, 128, "fc5", ("f32", "bf16x3"), (1, 33, 64, 65, 128, 129, 256, 257, 513, 1024, 1025, 1300)),
    ("c3_6x6x128_conv", 6, 2, 128, "conv", ("f32", "bf16x3"), (1, 37, 64, 65, 128, 129, 256, 257, 512, 513, 700)),
    ("4x4x64_conv", 4, 1, 64, "conv", ("f32",), (1, 37, 129, 257, 513, 1025, 2049, 2100)),
]


def _engine(n, blocks, filters, head, max_batch, precision="f32"):
    import tak_amd

    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                       evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch)
    if precision != "f32":
        e.set_precision(precision)
    return e


def _trained(orc, n, blocks, filters, head, count, seed):
    sts = posgen.distinct_positions(orc, n, count, seed=seed, max_plies=60)
    planes = orc.encode(n, sts)
    net = torch_ref.make_trained_net(n, blocks, filters, head, planes[:512], seed=seed)
    return net, sts, planes


@pytest.mark.parametrize("name,n,blocks,filters,head,precisions,sizes", SWEEP, ids=[s[0] for s in SWEEP])
def test_forward_against_fp64_on_trained_like_networks(orc, name, n, blocks, filters, head, precisions, sizes):
    total = max(sizes)
    net, sts, planes = _trained(orc, n, blocks, filters, head, total, seed=17)
    ref = torch_ref.forward64(net, planes)
    tensors = torch_ref.abi_tensors(net)
    for precision in precisions:
        e = _engine(n, blocks, filters, head, total, precision)
        e.load_state_dict(tensors)
        for k in sizes:
            r = torch_ref.slice_ref(ref, slice(0, k))
            p, v = e.policy_eval(sts[:k])
            torch_ref.report(f"{name} {precision} policy_eval B={k}", torch_ref.check_forward(p, v, r, precision, f"{name} {precision} states B={k}"))
            p, v = e.forward_mcts(planes[:k])
            torch_ref.report(f"{name} {precision} forward_mcts B={k}", torch_ref.check_forward(p, v, r, precision, f"{name} {precision} planes B={k}"))
        e.close()


def root_priors_against_fp64(orc, e, n, sts, ref, precision, what):
    """one search iteration from the roots `sts` on engine `e`: every root's children are the oracle's legal moves and carry
    p64[move_index(move)] within check_priors' gates (ref = forward64 of the same rows).  → the measured metrics
    (shared with tests/test_gpu_repr_corners.py)"""
    e.search_create(len(sts), arena_nodes=1 << 11)
    e.search_reset(sts)
    e.search_run(1)
    r = e.search_root()
    c = r["counts"]
    assert np.array_equal(c, orc.movegen(n, sts)[1])
    mask = np.arange(r["moves"].shape[1])[None, :] < c[:, None]
    idx = e.move_index(np.where(mask, r["moves"], 0)).reshape(mask.shape)
    lp = np.take_along_axis(ref["logp"], idx, axis=1)
    return torch_ref.check_priors(r["prior"], lp, mask, precision, what)


@pytest.mark.parametrize("name,n,blocks,filters,head,precision,games", [
    ("c2", 5, 2, 64, "fc5", "f32", 32),       # k_fc_small + k_fc_stats
    ("c2", 5, 2, 64, "fc5", "f32", 1000),
    ("c2", 5, 2, 64, "fc5", "f32", 4096),     # k_fc_ring with the statistics epilogue
    ("c2", 5, 2, 64, "fc5", "bf16x3", 32),
    ("c2", 5, 2, 64, "fc5", "bf16x3", 1000),
    ("c2", 5, 2, 64, "fc5", "bf16x3", 4096),
    ("c3", 6, 2, 128, "conv", "f32", 32),     # conv head: the backup's softmax_stats_wave over the logits row
    ("c3", 6, 2, 128, "conv", "f32", 1000),
])
def test_search_priors_against_fp64(orc, name, n, blocks, filters, head, precision, games):
    """tg_search_reset, one iteration, no noise: the root's children carry p[move_index(move)] as the tree backup computed it (from the
    FC's block statistics or from the logits row, with stat_exp) — against p64 under the same gates"""
    net, sts, planes = _trained(orc, n, blocks, filters, head, games, seed=23)
    ref = torch_ref.forward64(net, planes)
    e = _engine(n, blocks, filters, head, games, precision)
    e.load_state_dict(torch_ref.abi_tensors(net))
    m = root_priors_against_fp64(orc, e, n, sts, ref, precision, f"{name} {precision} priors, {games} games")
    torch_ref.report(f"{name} {precision} search priors G={games}", m)
    e.close()


@pytest.mark.parametrize("n,blocks,filters,head", [(5, 2, 64, "fc5"), (6, 1, 128, "conv")])
def test_training_forward_against_fp64(orc, n, blocks, filters, head):
    """tg_train_forward (BatchNorm on the batch's statistics) on a trained-like network: log_softmax against the fp64 training-mode
    forward, the same log-space gates"""
    net, sts, planes = _trained(orc, n, blocks, filters, head, 128, seed=29)
    e = _engine(n, blocks, filters, head, 64)
    e.load_state_dict(torch_ref.abi_tensors(net))
    e.train_create(chunk_size=16, chunks_in_step=1)
    logp, v = e.train_forward(sts)
    ref = torch_ref.forward64(net, planes, training=True)
    m = torch_ref.check_logp(logp, ref, "f32", f"train_forward {n}x{n} {head}")
    dv = np.abs(v.astype(np.float64) - ref["v"])
    m.update(pre=float((np.maximum(dv - 2.0 ** -23, 0) / (1 - ref["v"] ** 2)).max()), v_abs=float(dv.max()))
    torch_ref.report(f"train_forward {n}x{n} {head} f32", m)
    assert (dv <= torch_ref.GATES["f32"]["c"] * (1 - ref["v"] ** 2) + 2.0 ** -23).all(), m["pre"]
    e.close()
