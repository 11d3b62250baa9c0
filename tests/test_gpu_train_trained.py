"""The training step's backward on networks that look trained, with the targets a trained network's self-play leaves, gated per tensor
AND per slice.  Every gradient the suite had checked was taken on torch_ref.make_net (flat policy, |v| < 0.4, batch variances O(1))
under diffuse targets and one relative norm per tensor; a real run spends its steps where the policy is peaked and π one-hot
(k_policy_loss: the gradient is the small difference p − 1), the value saturated (k_value_train: 1.0f − v·v at |v| = 0.9999), some
BatchNorm channels nearly constant (invstd ≈ 160 amplifies dz) and the channels of one tensor two orders of magnitude apart.

Network and targets: test_gpu_train.trained_case — torch_ref.make_trained_net calibrated on the chunk's own 8-fold augmented planes
(value_std 2.5, seed 32), targets from _sharp_examples; the premises (two channels of the last conv layer with batch variance ≤ 1e-4, median
largest p ≥ 0.2, ≥ 10 % of the rows at |v| ≥ 0.99) are asserted on the fp64 reference.  Gates, all against torch_ref.fp64_gradients under
the engine's ReLU decisions, two accumulated chunks: losses 1e-5, every tensor 2e-5, and torch_ref.compare_slices: every slice relative
to its own fp64 norm, within max(2e-5, 3 × PyTorch f32's worst distance to fp64 for that class) — torch_ref.TRAIN_SLICE_F32, measured
on the CPU by `python tests/test_train_gates_trained.py` (two accumulated chunks, f32's own decisions on both sides):

  worst per-slice distance of PyTorch f32 to fp64   5×5 2×64 fc5   5×5 2×64 fc5   6×6 1×128 conv   6×6 2×128 conv     worst      gate
                                                    33 examples    129 examples   17 examples      33 examples
  conv weights, per output channel                  2.25e-6        1.57e-6        1.80e-6          1.86e-6            2.25e-6    2e-5
  BatchNorm weights, per element                    4.43e-5        7.00e-5        6.23e-5          1.80e-4            1.80e-4    5.40e-4
  BatchNorm biases, per element                     9.90e-4        4.09e-5        2.18e-4          4.19e-4            9.90e-4    2.97e-3
  policy.weight, per 64 outputs / per channel       7.13e-7        5.27e-7        6.14e-6          5.89e-6            6.14e-6    2e-5
  policy.bias, per 64 outputs / per channel         4.50e-7        1.96e-7        9.25e-5          2.55e-5            9.25e-5    2.78e-4
  value.weight, per input channel                   2.70e-6        3.43e-6        2.52e-6          3.45e-6            3.45e-6    2e-5
  value.bias (one slice)                            1.75e-6        3.77e-6        5.32e-7          7.76e-7            3.77e-6    2e-5
  on the saturated sub-batches: value.weight        3.15e-6 / 5.09e-6 / 1.42e-5 (z = sign(v) / −sign(v) / mixed)       1.42e-5    4.26e-5
                                value.bias          1.24e-6 / 1.23e-6 / 1.71e-6                                        1.71e-6    2e-5
  dz of the last conv layer, per channel            1.49e-6        1.15e-6        1.18e-6          1.48e-6            1.49e-6    2e-5
  dx of the last conv layer, per position           8.73e-6        6.14e-6        4.69e-6          1.07e-5            1.07e-5    3.21e-5
  worst whole tensor                                1.75e-6        3.77e-6        5.71e-6          1.39e-5

(A BatchNorm element's gradient is a sum over all rows that may cancel; trained_case's seed is chosen, on the fp64 reference alone, so
that none is closer to zero than torch_ref.SLICE_CONDITION = 1e-3 of its tensor's RMS element — see there — and the classes' gates
are set by the elements just above it.  The cap of 2 % floored slices per tensor is asserted.)  Every case prints the engine's worst tensor and worst slice
per class (the lines `trained-like …`).  tests/test_train_gates_trained.py shows on the CPU what the gates reject."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_train as T
import torch_ref

pytestmark = pytest.mark.gpu

# 5×5 at 264 positions: k_conv_pos, k_fc_small, k_gemm; at 1032: k_conv_halo with fused Σz, Σz² and fused backward sums, k_wgrad_halo, a
# ragged last workgroup; 6×6 1 × 128 at 136 positions: the k_conv_split head and its data gradient; 6×6 2 × 128 at 264
CASES = [(5, 2, 64, "fc5", 33), (5, 2, 64, "fc5", 129), (6, 1, 128, "conv", 17), (6, 2, 128, "conv", 33)]
HALO = CASES[1]


def _id(c):
    return f"{c[0]}x{c[0]}_{c[1]}x{c[2]}_{c[3]}_{c[4]}"


def run_case(orc, case):
    """the gate on one case; prints the engine's worst tensor and worst slice per class (`trained-like …`)"""
    n, blocks, filters, head, count = case
    net, examples = T.trained_case(orc, n, blocks, filters, head, count)
    tensor, worst, by_class = T.chunk_gradients_against_fp64(orc, n, blocks, filters, head, count, net=net, examples=examples, slices=True)
    print(f"trained-like train_chunk {_id(case)} ({8 * count} positions): worst tensor {tensor} {worst:.3e}", flush=True)
    for cls, (d, name, i) in sorted(by_class.items()):
        print(f"trained-like train_chunk {_id(case)}: {cls:14s} worst slice {d:.3e} ({name}[{i}]), gate {torch_ref.slice_gate(cls):.2e}", flush=True)


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_chunk_gradients_on_trained_like_networks(orc, case):
    run_case(orc, case)


VARIANT = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import torch
torch.set_num_threads(min(16, torch.get_num_threads()))
from oracle import oracle as orc
import test_gpu_train_trained as G
G.run_case(orc, {case!r})
"""


@pytest.mark.parametrize("switch", ["TG_NO_CONV_STATS", "TG_NO_BWD_SUMS_FUSION"])
def test_chunk_gradients_on_trained_like_networks_without_the_fused_sums(switch):
    """the 1032-position case with BatchNorm's Σz, Σz² (Σg, Σg·x̂) from passes over memory instead of the convolutions' accumulators:
    the same gates.  The switches are read once per process, so each variant runs in a child of its own."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if not k.startswith("TG_")}
    env[switch] = "1"
    out = subprocess.run([sys.executable, "-c", VARIANT.format(root=root, case=HALO)], env=env, capture_output=True, text=True, timeout=600)
    print("\n".join(l.replace("trained-like", f"trained-like {switch}=1") for l in out.stdout.splitlines() if l.startswith("trained-like")))
    assert out.returncode == 0, out.stderr[-3000:]


@pytest.fixture(scope="module")
def halo(orc):
    n, blocks, filters, head, count = HALO
    net, examples = T.trained_case(orc, n, blocks, filters, head, count)
    return net, examples


def test_one_quiet_layers_backward_operands(orc, halo):
    """The last conv layer (quiet by make_trained_net's default) of the 1032-position case, through tg_train_debug_capture: dz per
    channel and dx per position against the fp64 gradients of the same tensors under the engine's decisions; the batch mean per channel
    to 2e-5 σ + 2e-7 |mean| and the variance implied by invstd of every quiet channel to 3e-5 relative (the bounds of
    test_batchnorm_statistics_from_the_conv_accumulators_by_value)"""
    n, blocks, filters, head, count = HALO
    net, examples = halo
    last, positions = 2 * blocks, 8 * count
    rows = positions * n * n
    e = T._engine(n, blocks, filters, head)
    e.load_state_dict(torch_ref.abi_tensors(net))
    e.train_create(chunk_size=count, chunks_in_step=1000)
    e.train_debug_capture(last)
    e.train_chunk(*examples[0])
    got = {f"{what}/{last}": e.train_debug_read(what, last, (rows, filters)) for what in ("dz", "dx")}
    mean, invstd = e.train_debug_read("mean", last, (filters,)), e.train_debug_read("invstd", last, (filters,))
    decisions = torch_ref.engine_relu_decisions(e, 1 + 2 * blocks, positions, n, filters)
    e.train_debug_capture(-1)
    e.close()
    planes, pi, z, _ = T._targets(orc, n, head, examples[0])
    (g64,), _ = torch_ref.fp64_gradients(net, planes, pi, z, [decisions], keep_layers=[last])
    ref = {k: g64[k] for k in got}
    by_class, _ = torch_ref.compare_slices(got, ref, head, n, gates=torch_ref.slice_gate, what="operands of the last conv layer")
    mean64, var64 = torch_ref.batch_statistics64(net, planes)[last]
    quiet = var64 <= 1e-4
    assert quiet.sum() >= 2
    sigma = np.sqrt(var64)
    d_mean = np.abs(mean - mean64) / (2e-5 * sigma + 2e-7 * np.abs(mean64))
    var = 1.0 / invstd.astype(np.float64) ** 2 - 1e-5
    d_var = np.abs(var / var64 - 1.0)
    for cls, (d, name, i) in sorted(by_class.items()):
        print(f"trained-like operands {_id(HALO)}: {cls} worst slice {d:.3e} ({name}[{i}]), gate {torch_ref.slice_gate(cls):.2e}")
    print(f"trained-like operands {_id(HALO)}: mean, worst channel {d_mean.max():.3f} × its bound; implied variance of the {int(quiet.sum())} quiet "
          f"channels (var {var64[quiet].min():.2e} … {var64[quiet].max():.2e}) {d_var[quiet].max():.3e} relative, of all channels {d_var.max():.3e}", flush=True)
    assert (d_mean <= 1.0).all(), (int(np.argmax(d_mean)), float(d_mean.max()))
    assert (d_var[quiet] <= 3e-5).all(), (np.nonzero(quiet)[0], d_var[quiet])


def test_head_rows_on_the_trained_like_batch(orc, halo):
    """tg_train_forward's logp and v on the first chunk's batch: check_logp and the value gate of test_gpu_fp64"""
    n, blocks, filters, head, count = HALO
    net, examples = halo
    planes, _, _, a_states = T._targets(orc, n, head, examples[0])
    e = T._engine(n, blocks, filters, head)
    e.load_state_dict(torch_ref.abi_tensors(net))
    e.train_create(chunk_size=count, chunks_in_step=1)
    logp, v = e.train_forward(a_states)
    e.close()
    ref = torch_ref.forward64(net, planes, training=True)
    m = torch_ref.check_logp(logp, ref, "f32", f"train_forward trained-like {_id(HALO)}")
    dv = np.abs(v.astype(np.float64) - ref["v"])
    m.update(pre=float((np.maximum(dv - 2.0 ** -23, 0) / (1 - ref["v"] ** 2)).max()), v_abs=float(dv.max()),
             v_max=float(np.abs(ref["v"]).max()), rows=8 * count)
    torch_ref.report(f"trained-like train_forward {_id(HALO)} f32", m)
    assert (dv <= torch_ref.GATES["f32"]["c"] * (1 - ref["v"] ** 2) + 2.0 ** -23).all(), m["pre"]


def saturated_gate(cls):
    return torch_ref.slice_gate(cls + ".saturated")


def test_value_gradient_where_one_minus_v2_stands_alone(orc, halo):
    """value.bias's gradient is Σ dpre = Σ −2(z − v)(1 − v²)/B.  In a mixed chunk the unsaturated rows carry it; in the three sub-batches
    of test_gpu_train.value_sub_batches EVERY row has |v| ≥ 0.99 — asserted on the fp64 reference of the sub-batch, with z = sign(v) on
    every row, z = −sign(v) on every row, and a third each of sign(v), −sign(v), 0 — so k_value_train's `1.0f − v*v` decides value.bias
    and every channel of value.weight.  One chunk each on a fresh trainer: every tensor to 2e-5, value.bias and value.weight's channels
    at the gates of their `.saturated` classes (PyTorch f32 on the same sub-batches, × 3); the other slices are printed only."""
    n, blocks, filters, head, count = HALO
    net, examples = halo
    shapes = T._shapes(net)
    for name, (sub_net, sub) in T.value_sub_batches(orc, net, n, head, examples[0]).items():
        k = len(sub[0])
        assert k >= 16, (name, k)
        planes, pi, z, _ = T._targets(orc, n, head, sub)
        v64 = torch_ref.forward64(sub_net, planes, training=True)["v"]
        assert (np.abs(v64) >= 0.99).all(), (name, float(np.abs(v64).min()))
        same, opposed = float((z == np.sign(v64)).mean()), float((z == -np.sign(v64)).mean())
        assert (same, opposed) == {"z = sign(v)": (1.0, 0.0), "z = -sign(v)": (0.0, 1.0)}.get(name, (same, opposed)), (name, same, opposed)
        assert name != "mixed z, v < 0" or (min(same, opposed) >= 0.3 and (v64 < 0).all()), (name, same, opposed)
        e = T._engine(n, blocks, filters, head)
        e.load_state_dict(torch_ref.abi_tensors(sub_net))
        e.train_create(chunk_size=k, chunks_in_step=1000)
        e.train_chunk(*sub)
        (g64,), _ = torch_ref.fp64_gradients(sub_net, planes, pi, z, [torch_ref.engine_relu_decisions(e, 1 + 2 * blocks, 8 * k, n, filters)])
        got = {t: e.train_get_grad(t, shapes[t]) for t in shapes}
        e.close()
        by_class, (tensor, whole) = torch_ref.compare_slices(got, g64, head, n, gates=saturated_gate, what=name,
                                                                classes=("value.bias", "value.weight"))
        print(f"trained-like value sub-batch {name:15s} ({k} examples, |v| from {float(np.abs(v64).min()):.4f} to 1 - {1 - float(np.abs(v64).max()):.1e}): "
              f"value.bias {by_class['value.bias'][0]:.3e} (gate {saturated_gate('value.bias'):.2e}), value.weight worst channel "
              f"{by_class['value.weight'][0]:.3e} (gate {saturated_gate('value.weight'):.2e}), worst tensor {tensor} {whole:.3e}", flush=True)
