"""The teeth of the training step's gradient gate (tests/test_gpu_train.py: every tensor within 2e-5 of the fp64 gradients under the
implementation's own ReLU decisions), checked on the CPU in the manner of tests/test_forward_gates.py, at 129 examples = 1032 positions:
a ragged size of the halo kernels (64.5 workgroups of 16 positions), where a mistake about the LAST position is as small as it gets.

(a) PyTorch f32 autograd stays inside the gate against fp64 under PyTorch f32's own decisions: the reference alone does not use the
    gate up (tests/test_torch_ref.py shows 5e-6 at 48 positions).
(b) Each of a list of kernel-sized mistakes, made on the fp64 side (torch_ref.fp64_gradients' hook, autograd functions below) and
    compared with the unmutated fp64 gradients under the same decisions, moves at least one gated tensor by more than 2e-5:
      * BatchNorm's batch mean and variance of one layer divide correct sums by a row count rounded up to 16 positions;
      * one layer's Σz² includes the rows of one extra zero-input position (whose z is the conv bias);
      * the last position's rows are missing from one layer's weight gradient;
      * the last position's rows are missing from one layer's BatchNorm-backward sums Σg, Σg·x̂;
      * the last row is missing from the policy bias gradient (fc5) / from the conv head's bias gradient (conv);
      * one layer's data gradient is scaled by 1.001.

What the gate does NOT see at 1032 positions (measured here; the test prints the figures and asserts both sides of them):
      * an extra zero-input position in one layer's Σz²: with PyTorch's default initialisation a conv bias is ≈ 0.03 against a
        standard deviation of z of ≈ 0.5, so n² rows of bias² among 25 800 (37 152) rows of z² move the variance by a few 1e-6:
        the worst gated tensor moves by 5.5e-6 on 5×5 (0.27 × the gate) and 9.5e-6 on 6×6 (0.48 ×).  The effect grows as 1 / rows:
        on 5×5 1.4e-5 at 65 examples and 2.5e-5 at 33; on 6×6 2.3e-5 at 65.  It is kept at the largest example count of 129, 65,
        33, 17, … at which the gate rejects it (AT_SIZE).  The moments themselves are pinned more tightly than the gradients can pin
        them by test_gpu_train.test_batchnorm_statistics_from_the_conv_accumulators_by_value (variance to 1e-5, with biases of ± 25).
    The smallest mistake the gate does see at 1032 positions is the conv head's bias gradient without its last row of 37 152:
    3.9e-5, 1.9 × the gate."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import torch_ref
from test_torch_ref import _batch, _f32_decisions

GATE = 2e-5
EXAMPLES = 129
LAYER = 1  # res0.conv1 / res0.bn1: a layer with tensors below it (conv0, bn0) that its data gradient reaches
TOPOLOGIES = [(5, 1, 32, "fc5"), (6, 1, 32, "conv")]

# (head, mistake) → the example count at which the mistake is asserted, where the gate cannot see it at EXAMPLES (module docstring)
AT_SIZE = {
    ("fc5", "an extra zero-input position in one layer's Σz²"): 33,
    ("conv", "an extra zero-input position in one layer's Σz²"): 65,
}


class Conv(torch.autograd.Function):
    """3×3 convolution with its three gradients written out; drop_w: the last position is missing from the weight gradient;
    dx_scale: factor on the data gradient; drop_b_row: the last row (last position, last square) is missing from the bias gradient"""

    @staticmethod
    def forward(ctx, x, w, b, drop_w, dx_scale, drop_b_row):
        ctx.save_for_backward(x, w)
        ctx.cfg = (drop_w, dx_scale, drop_b_row)
        return F.conv2d(x, w, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        drop_w, dx_scale, drop_b_row = ctx.cfg
        k = x.shape[0] - 1 if drop_w else x.shape[0]
        gw = torch.nn.grad.conv2d_weight(x[:k], w.shape, g[:k], padding=1)
        gx = torch.nn.grad.conv2d_input(x.shape, w, g, padding=1) * dx_scale
        gb = g.sum((0, 2, 3))
        if drop_b_row:
            gb = gb - g[-1, :, -1, -1]
        return gx, gw, gb, None, None, None


class BatchNorm(torch.autograd.Function):
    """training-mode BatchNorm with the backward pass the engine runs: Σg and Σg·x̂ (= dβ, dγ), then dz = γ·invstd·(g − Σg/M − x̂·Σg·x̂/M);
    drop: the last position's rows are missing from both sums (M stays the true row count)"""

    @staticmethod
    def forward(ctx, z, gamma, beta, eps, drop):
        mean = z.mean((0, 2, 3), keepdim=True)
        invstd = torch.rsqrt(z.var((0, 2, 3), unbiased=False, keepdim=True) + eps)
        xhat = (z - mean) * invstd
        ctx.save_for_backward(xhat, invstd, gamma)
        ctx.drop = drop
        return xhat * gamma[None, :, None, None] + beta[None, :, None, None]

    @staticmethod
    def backward(ctx, g):
        xhat, invstd, gamma = ctx.saved_tensors
        k = g.shape[0] - 1 if ctx.drop else g.shape[0]
        rows = g.shape[0] * g.shape[2] * g.shape[3]
        sg = g[:k].sum((0, 2, 3))
        sgx = (g[:k] * xhat[:k]).sum((0, 2, 3))
        dz = gamma[None, :, None, None] * invstd * (g - sg[None, :, None, None] / rows - xhat * sgx[None, :, None, None] / rows)
        return dz, sgx, sg, None, None


class Linear(torch.autograd.Function):
    """the FC policy head; drop: the last row of dLogits is missing from the bias gradient"""

    @staticmethod
    def forward(ctx, x, w, b, drop):
        ctx.save_for_backward(x, w)
        ctx.drop = drop
        return F.linear(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g @ w, g.t() @ x, (g[:-1] if ctx.drop else g).sum(0), None


def _bn_from_sums(m, z, rows, extra_sq=None):
    """BatchNorm's output from Σz / rows and (Σz² + extra_sq) / rows − mean² (differentiated as written)"""
    mean = z.sum((0, 2, 3)) / rows
    sq = (z * z).sum((0, 2, 3))
    if extra_sq is not None:
        sq = sq + extra_sq
    var = sq / rows - mean * mean
    c = lambda t: t[None, :, None, None]  # noqa: E731
    return (z - c(mean)) * c(torch.rsqrt(var + m.eps)) * c(m.weight) + c(m.bias)


def _written_out():
    """the unmutated network through the autograd functions above: has to reproduce the module path"""
    return dict(conv=lambda l, m, x: Conv.apply(x, m.weight, m.bias, False, 1.0, False),
                bn=lambda l, m, z: BatchNorm.apply(z, m.weight, m.bias, m.eps, False),
                policy=lambda m, x: Linear.apply(x, m.weight, m.bias, False) if x.dim() == 2 else Conv.apply(x, m.weight, m.bias, False, 1.0, False))


def _mistakes(head):
    """name → hook for torch_ref.fp64_gradients"""
    at = lambda f: (lambda l, m, t: f(m, t) if l == LAYER else m(t))  # noqa: E731
    bias = {}

    def conv_keeping_bias(l, m, x):
        bias[l] = m.bias
        return m(x)

    def rows(z):
        return z.shape[0] * z.shape[2] * z.shape[3]

    def padded(m, z):
        positions = -(-z.shape[0] // 16) * 16
        return _bn_from_sums(m, z, positions * z.shape[2] * z.shape[3])

    def extra_position(m, z):  # a zero-input position's z is the conv bias on each of its n² rows
        return _bn_from_sums(m, z, rows(z), extra_sq=z.shape[2] * z.shape[3] * bias[LAYER] ** 2)

    out = {
        "BatchNorm divisor rounded up to 16 positions": dict(bn=at(padded)),
        "an extra zero-input position in one layer's Σz²": dict(conv=conv_keeping_bias, bn=at(extra_position)),
        "last position missing from one weight gradient": dict(conv=at(lambda m, x: Conv.apply(x, m.weight, m.bias, True, 1.0, False))),
        "last position missing from Σg, Σg·x̂": dict(bn=at(lambda m, z: BatchNorm.apply(z, m.weight, m.bias, m.eps, True))),
        "one data gradient × 1.001": dict(conv=at(lambda m, x: Conv.apply(x, m.weight, m.bias, False, 1.001, False))),
    }
    if head == "fc5":
        out["last row missing from the policy bias gradient"] = dict(policy=lambda m, x: Linear.apply(x, m.weight, m.bias, True))
    else:
        out["last row missing from the conv head's bias gradient"] = dict(policy=lambda m, x: Conv.apply(x, m.weight, m.bias, False, 1.0, True))
    return out


def _worst(g, ref):
    """the gate's measure: the largest ‖g − ref‖₂ / ‖ref‖₂ over the gated tensors (all but the conv biases in front of a BatchNorm)"""
    worst = ("", 0.0)
    for k in ref:
        if k.endswith(".bias") and "conv" in k and not k.startswith("policy"):
            continue
        d = float(np.linalg.norm(np.asarray(g[k], np.float64) - ref[k]) / np.linalg.norm(ref[k]))
        worst = max(worst, (k, d), key=lambda t: t[1])
    return worst


def _setup(orc, n, blocks, filters, head, count):
    net = torch_ref.make_net(n, blocks, filters, head, seed=10 + n)
    planes, pi, z = _batch(n, head, count, seed=5, orc=orc)
    assert len(planes) == 8 * count
    decisions = _f32_decisions(net, planes)
    (ref,), _ = torch_ref.fp64_gradients(net, planes, pi, z, [decisions])
    return net, planes, pi, z, decisions, ref


@pytest.mark.parametrize("n,blocks,filters,head", TOPOLOGIES, ids=[f"{t[0]}x{t[0]}_{t[3]}" for t in TOPOLOGIES])
def test_gate_accepts_pytorch_f32_at_1032_positions(orc, n, blocks, filters, head):
    net, planes, pi, z, decisions, ref = _setup(orc, n, blocks, filters, head, EXAMPLES)
    assert len(planes) == 1032
    torch_ref.train_chunk(net, planes, pi, z)
    name, worst = _worst(torch_ref.named_grads(net), ref)
    print(f"fp64-gate pytorch-f32 autograd {n}x{n} {head} 1032 positions: worst tensor {name} {worst:.3e}")
    assert worst <= GATE, (name, worst)
    # the autograd functions the mistakes are made in are the network's own operations when no mistake is switched on
    (same,), _ = torch_ref.fp64_gradients(net, planes, pi, z, [decisions], hook=_written_out())
    name, worst = _worst(same, ref)
    assert worst <= 1e-12, (name, worst)


@pytest.mark.parametrize("n,blocks,filters,head", TOPOLOGIES, ids=[f"{t[0]}x{t[0]}_{t[3]}" for t in TOPOLOGIES])
def test_gate_rejects_every_mistake(orc, n, blocks, filters, head):
    """Every mistake of the module docstring at 129 examples — except the extra zero-input position in Σz², which the gate does not see
    there (0.27 × the gate on 5×5, 0.48 × on 6×6: asserted, so that the statement stays true) and which is held at 33 / 65 examples
    (1.26 × / 1.15 ×)"""
    by_size = {}

    def measure(name, hook, count):
        if count not in by_size:
            by_size[count] = _setup(orc, n, blocks, filters, head, count)
        net, planes, pi, z, decisions, ref = by_size[count]
        (g,), _ = torch_ref.fp64_gradients(net, planes, pi, z, [decisions], hook=hook)
        tensor, worst = _worst(g, ref)
        print(f"{n}x{n} {head}, {count} examples: {name}: worst tensor {tensor} {worst:.3e} ({worst / GATE:.2f} × the gate)")
        return worst

    passed = []
    for name, hook in _mistakes(head).items():
        count = AT_SIZE.get((head, name), EXAMPLES)
        if count != EXAMPLES:  # (the record of what the gate cannot see: the figure at 1032 positions beside the size that is kept)
            assert measure(name, hook, EXAMPLES) <= GATE, f"{name} is seen at {EXAMPLES} examples: take it out of AT_SIZE"
        if measure(name, hook, count) <= GATE:
            passed.append(f"{name} ({count} examples)")
    assert not passed, f"mistakes the gate lets through: {passed}"
