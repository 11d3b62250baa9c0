"""The per-layer inference forward (net_forward_impl's branch for networks the fused towers do not serve: 3×3 and 4×4 boards, filter
counts other than 64 / 128 on 5×5 and 128 on 6×6, 24 or more residual blocks) against float64 on trained-like networks, in the manner
of tests/test_gpu_fp64.py: make_trained_net, positions from play, forward64, both entry points (tg_policy_eval on packed states —
k_encode in front —, tg_forward_mcts on planes — k_nchw_to_nhwc in front), check_forward under GATES["f32"], one report line per case
and size.  tests/test_topology_forward.py shows on the CPU that these gates reject the mistakes these kernels can make.

Every case also asserts that a position's bits do not depend on the batch: each smaller batch equals the first rows of the largest one
bit for bit, policy and value, on both entry points — across the k_conv_pos tilings, k_conv_halo against k_conv_pos, k_conv_split
against k_conv_pos, k_fc_small against k_fc_ring<0>.

Above REF_ALL positions the float64 reference is computed on a subset of rows (reference_rows): the first REF_ALL (COND_ROWS), both
sides of every batch size of the case and of every multiple of 128 positions (the row tiles of k_gemm and k_fc_ring, a multiple of
every k_conv_pos / k_conv_halo workgroup), and the last 24 positions (the ragged last workgroup of every kernel: at most 16
positions).  The engine evaluates the whole batch; the bit comparison covers every row.

The three 49-layer networks are gated at GATES["f32"] × max(1, depth ratio) (torch_ref.depth_scaled_gates): the ratio is PyTorch
fp32's own distance to float64 on the 24-block network over that on a 2-block network of the same shape, on the same rows, per metric —
nothing in it is measured on the engine."""
import numpy as np
import pytest
import torch

import posgen
import torch_ref

pytestmark = pytest.mark.gpu

SEED = 17
MAX_PLIES = {3: 8, 4: 30, 5: 60, 6: 60}
COND_ROWS = {3: 120, 4: 300, 5: 300, 6: 300}   # rows the trained-like conditions are asserted on (and make_trained_net calibrates on)
REF_ALL = 300                                    # batches up to this size are compared with float64 on every row
DEEP_CALIB = 128                                 # calibration planes of the 49-layer networks
DEEP_FIRST = 37                                  # … whose reference holds the first 37 rows (the smallest batch) and the boundary rows

# (name, n, blocks, filters, head, batch sizes) — what the launchers (launch_conv3x3, launch_gemm, launch_softmax, pos_tiling.h) pick
CASES = [
    # conv0: k_conv_pos on the (5,128) table with Cpad 80, cout_valid 96 of CoutP 128; the block: k_conv_pos with Cpad 96 — the
    # brackets ≤ 256 / ≤ 512 / ≤ 1024 / above; k_gemm<2,1> with K = 2400 (37.5 steps of 64) and NP = 1600; k_softmax (no statistics)
    ("5x5_1x96_fc", 5, 1, 96, "fc5", (1, 37, 127, 128, 129, 256, 257, 513, 1025)),
    # k_conv_pos on the (5,64) table (CoutP 64, Cpad 80 and 32) in all five brackets; k_gemm<2,1> with K = 800 (12.5 steps)
    ("5x5_2x32_fc", 5, 2, 32, "fc5", (1, 256, 257, 512, 513, 1024, 1025, 2048, 2049)),
    # k_conv3x3<2,1> (CoutP 192); the head (CoutP 128) on k_conv3x3<2,2>, Cpad 160 > 128; k_softmax_conv with 123 of 128 channels;
    # 6 positions = 150 rows: a position straddles two 128-row workgroups
    ("5x5_1x160_conv", 5, 1, 160, "conv", (1, 6, 37, 129, 300)),
    # k_conv3x3<2,1> at Cpad 192; k_fc_small and k_fc_ring<0> at K = 4800 (75 steps) with the statistics epilogue, k_softmax_stats
    ("5x5_1x192_fc", 5, 1, 192, "fc5", (37, 2049)),
    # conv0 on k_conv_pos (5,128) with two workgroup columns; the block on k_conv3x3<1,2> (two row tiles of Cpad 256 exceed 160 KB of
    # LDS); the FC at K = 6400 on both sides of FC_SMALL_ROWS = 2048
    ("5x5_1x256_fc", 5, 1, 256, "fc5", (1, 3, 37, 129, 2048, 2049)),
    # conv0 and the block on the (5,64) table (CoutP 64); the head (123 of CoutP 128) on k_conv_pos (5,128) with Cpad 32
    ("5x5_1x32_conv", 5, 1, 32, "conv", (37, 257)),
    # k_conv3x3<2,1> with Cpad 96 and 64 (CoutP 64); the head (CoutP 256) on the (6,128) table with Cpad 64
    ("6x6_1x64_conv", 6, 1, 64, "conv", (1, 4, 37, 257, 513)),
    # the (6,128) table with Cpad 96 (all layers: CoutP 128 and 256) in its three brackets ≤ 256 / ≤ 512 / above
    ("6x6_1x96_conv", 6, 1, 96, "conv", (1, 37, 256, 257, 512, 513)),
    # conv0 (Cpad 96, CoutP 256) on the (6,128) table with two columns; the block and the head (Cpad 256) on k_conv3x3<1,2>
    ("6x6_1x256_conv", 6, 1, 256, "conv", (1, 2, 37, 129)),
    # a board no tiling table knows: k_conv3x3<2,2> (96 and 128 filters: CoutP 128), the head (59 of CoutP 64) on <2,1>; 9 positions =
    # 144 rows cross a 128-row tile
    ("4x4_1x128_conv", 4, 1, 128, "conv", (1, 9, 37, 129)),
    ("4x4_2x96_conv", 4, 2, 96, "conv", (1, 9, 37, 129)),
    # the last generic tile: the block (Cpad 320: two row tiles exceed 160 KB of LDS; CoutP 320) and the head (CoutP 64) on k_conv3x3<1,1>
    ("4x4_1x320_conv", 4, 1, 320, "conv", (1, 9, 37)),
    # 9-row positions straddle every tile; k_softmax_conv with 27 of 64 channels
    ("3x3_1x128_conv", 3, 1, 128, "conv", (1, 15, 37)),
    ("3x3_1x32_conv", 3, 1, 32, "conv", (1, 15, 37)),
    # 49 layers: not fused.  k_conv_pos; from 1024 positions the F → F layers run k_conv_halo, the residual ones with res == out; the
    # FC (k_fc_small + k_fc_stats) reads row-major activations, not the tower's fragment order
    ("5x5_24x64_fc", 5, 24, 64, "fc5", (37, 1023, 1024, 1025)),
    # the same on the 6×6 halo geometry; the head (F → 251 of 256) on k_conv_split (≤ 128), k_conv_pos, then k_conv_halo without a residual
    ("6x6_24x128_conv", 6, 24, 128, "conv", (37, 1023, 1024, 1025)),
    # the third halo geometry (5×5, 128 channels), which no network of the issue's table reaches in inference: the residual layers in
    # place and the head (F → 123 of 128) on k_conv_split<2,8>, k_conv_pos (5,128), then k_conv_halo
    ("5x5_24x128_conv", 5, 24, 128, "conv", (37, 1023, 1024, 1025)),
]
CASE = {c[0]: c for c in CASES}


def engine(n, blocks, filters, head, max_batch):
    import tak_amd

    return tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                          evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch)


def reference_rows(sizes, first):
    """the rows of the largest batch the float64 reference is computed on (module comment), ascending; always the first `first`"""
    total = max(sizes)
    if total <= REF_ALL:
        return np.arange(max(total, first))
    rows = set(range(first)) | set(range(16)) | set(range(total - 24, total))
    for edge in list(sizes) + list(range(128, total, 128)):
        rows |= {r for r in range(edge - 2, edge + 2) if 0 <= r < total}
    return np.array(sorted(rows))


def assert_trained_like(net, ref, what):
    """tests/test_forward_gates.py's conditions on the reference alone: the network is the kind the gates are meant for"""
    pmax = np.exp(ref["logp"].max(1))
    assert np.median(pmax) >= 0.15, (what, "median largest probability", float(np.median(pmax)))
    assert np.abs(ref["v"]).max() >= 0.99, (what, "largest |v64|", float(np.abs(ref["v"]).max()))
    assert ref["logp"].min() < -20, (what, "smallest log p64", float(ref["logp"].min()))
    var = min(float(b.running_var.min()) for b in net.modules() if isinstance(b, torch.nn.BatchNorm2d))
    assert var <= 1e-4, (what, "smallest BatchNorm running variance", var)


def build_case(orc, name):
    """→ dict(net, sts, planes [the largest batch], rows = reference_rows, ref = forward64 on them, gates, ratios).  The trained-like
    conditions are asserted on the first COND_ROWS rows (every reference row of a 49-layer network); gates = GATES["f32"], for a
    49-layer network depth-scaled."""
    _, n, blocks, filters, head, sizes = CASE[name]
    deep = 1 + 2 * blocks > 48
    cond = DEEP_FIRST if deep else COND_ROWS[n]
    count = max(max(sizes), DEEP_CALIB if deep else cond)
    sts = posgen.distinct_positions(orc, n, count, seed=SEED, max_plies=MAX_PLIES[n])
    planes = orc.encode(n, sts)
    calib = planes[:DEEP_CALIB] if deep else planes[:cond]
    net = torch_ref.make_trained_net(n, blocks, filters, head, calib, seed=SEED)
    rows = reference_rows(sizes, cond)
    ref = torch_ref.forward64(net, planes[rows])
    assert_trained_like(net, ref if deep else torch_ref.slice_ref(ref, slice(0, cond)), name)
    gates, ratios = None, None
    if deep:
        shallow = torch_ref.make_trained_net(n, 2, filters, head, calib, seed=SEED)
        gates, ratios, m_deep, m_flat = torch_ref.depth_scaled_gates(net, shallow, planes[rows], ref, torch_ref.forward64(shallow, planes[rows]))
        print(f"depth-ratio {name}: " + ", ".join(f"{k} {m_deep[k]:.3e} / {m_flat[k]:.3e} = {ratios[k]:.2f}" for k in ratios) +
              f" -> gates a {gates['a']:.2e}, t {gates['t']:.2e}, c {gates['c']:.2e} on {len(rows)} rows", flush=True)
    total = max(sizes)
    return dict(net=net, sts=sts[:total], planes=planes[:total], rows=rows[rows < total], ref=torch_ref.slice_ref(ref, rows < total),
                gates=gates, ratios=ratios)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_per_layer_forward_against_fp64(orc, name):
    _, n, blocks, filters, head, sizes = CASE[name]
    c = build_case(orc, name)
    rows, total = c["rows"], max(sizes)
    e = engine(n, blocks, filters, head, total)
    e.load_state_dict(torch_ref.abi_tensors(c["net"]))
    whole = {}
    for k in sorted(sizes, reverse=True):   # the largest batch first: every smaller one is compared with its first rows
        sel = rows < k
        r = torch_ref.slice_ref(c["ref"], sel)
        for entry, run in (("policy_eval", lambda: e.policy_eval(c["sts"][:k])), ("forward_mcts", lambda: e.forward_mcts(c["planes"][:k]))):
            p, v = run()
            p, v = np.asarray(p, np.float32), np.asarray(v, np.float32).reshape(-1)
            assert p.shape[0] == k and v.shape == (k,)
            m = torch_ref.check_forward(p[rows[sel]], v[rows[sel]], r, "f32", f"{name} {entry} B={k}", gates=c["gates"])
            torch_ref.report(f"{name} f32 {entry} B={k}", m)
            if k == total:
                whole[entry] = (_bits(p), _bits(v))
            else:
                bad = np.flatnonzero((_bits(p) != whole[entry][0][:k]).any(axis=1) | (_bits(v) != whole[entry][1][:k]))
                assert not len(bad), (f"{name} {entry}: rows of B={k} whose bits differ from the same rows of B={total}", bad[:8], len(bad))
    e.close()


PRIORS = [
    "5x5_1x96_fc",     # no value column, no block statistics: the backup's softmax_stats_wave over a logits row of stride 1600
    "5x5_1x256_fc",    # k_fc_small + k_fc_stats at K = 6400
    "5x5_1x32_conv",   # P = 3075 > 2048: the probability path
    "6x6_1x64_conv",
    "4x4_1x128_conv",
]


@pytest.mark.parametrize("name", PRIORS)
def test_root_priors_against_fp64(orc, name):
    """tg_search_reset and one iteration at 33 roots: the children carry p64[move_index(move)] (test_gpu_fp64.root_priors_against_fp64)"""
    import test_gpu_fp64

    _, n, blocks, filters, head, _ = CASE[name]
    games, cond = 33, COND_ROWS[n]
    sts = posgen.distinct_positions(orc, n, cond, seed=SEED, max_plies=MAX_PLIES[n])
    planes = orc.encode(n, sts)
    net = torch_ref.make_trained_net(n, blocks, filters, head, planes, seed=SEED)
    ref = torch_ref.forward64(net, planes[:games])
    e = engine(n, blocks, filters, head, games)
    e.load_state_dict(torch_ref.abi_tensors(net))
    m = test_gpu_fp64.root_priors_against_fp64(orc, e, n, sts[:games], ref, "f32", f"{name} priors, {games} games")
    torch_ref.report(f"{name} f32 search priors G={games}", m)
    e.close()


@pytest.mark.parametrize("name,names_layers", [("5x5_24x64_fc", True), ("6x6_24x128_conv", True), ("5x5_1x96_fc", False), ("4x4_1x128_conv", False)])
def test_bf16x3_is_refused_and_f32_still_served(orc, name, names_layers):
    """TG_PRECISION_BF16X3 on a network its towers do not serve: tg_net_finalize fails with TG_ERR_INVALID_ARG (for a 49-layer network
    the message names the 48-layer limit), nothing is served meanwhile, and f32 is served again after set_precision("f32") and a reload"""
    import tak_amd

    _, n, blocks, filters, head, _ = CASE[name]
    sts = posgen.distinct_positions(orc, n, 8, seed=SEED, max_plies=MAX_PLIES[n])
    net = torch_ref.make_net(n, blocks, filters, head, seed=SEED)
    tensors = torch_ref.abi_tensors(net)
    e = engine(n, blocks, filters, head, 8)
    e.load_state_dict(tensors)
    p0, v0 = e.policy_eval(sts)
    e.set_precision("bf16x3")
    with pytest.raises(tak_amd.TgError) as refused:
        e.load_state_dict(tensors)
    assert refused.value.code == -1, str(refused.value)   # TG_ERR_INVALID_ARG
    assert "TG_PRECISION_BF16X3" in str(refused.value)
    if names_layers:
        assert "48" in str(refused.value) and "49 layers" in str(refused.value), str(refused.value)
    with pytest.raises(tak_amd.TgError) as unserved:
        e.policy_eval(sts)
    assert unserved.value.code == -7, str(unserved.value)  # TG_ERR_STATE: not finalized
    e.set_precision("f32")
    e.load_state_dict(tensors)
    p1, v1 = e.policy_eval(sts)
    assert np.array_equal(_bits(p1), _bits(p0)) and np.array_equal(_bits(v1), _bits(v0))
    ref = torch_ref.forward64(net, orc.encode(n, sts))
    if 1 + 2 * blocks <= 48:   # (the deep networks' gate is test_per_layer_forward_against_fp64's business)
        torch_ref.check_forward(p1, np.asarray(v1).reshape(-1), ref, "f32", f"{name} after the refusal")
    e.close()
