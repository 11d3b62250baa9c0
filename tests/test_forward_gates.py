"""The forward gates of tests/torch_ref.py (check_forward against a float64 forward, on make_trained_net's peaked networks) checked on the
CPU: PyTorch's own fp32 forward passes the f32 gates, and each of a list of small kernel-sized mistakes — a dropped bias, a per-mille
mis-scale, a lost edge tap, another BatchNorm eps, two outputs swapped — is rejected under the f32 AND the looser bf16x3 constants.
The second half is what bounds how loose the constants may be set."""
import copy

import numpy as np
import pytest
import torch

import posgen
import torch_ref

TOPOLOGIES = [(5, 1, 32, "fc5"), (6, 1, 32, "conv"), (4, 1, 32, "conv")]


def _setup(orc, n, blocks, filters, head):
    sts = posgen.distinct_positions(orc, n, 192, seed=3, max_plies=60)
    planes = orc.encode(n, sts)
    net = torch_ref.make_trained_net(n, blocks, filters, head, planes, seed=5)
    return net, planes, torch_ref.forward64(net, planes)


def _mutations(net):
    """name → mutated copy of `net` (or a function of the unmutated fp32 outputs, for a mistake in the output order)"""
    def mut(f):
        m = copy.deepcopy(net)
        with torch.no_grad():
            f(m)
        return m.eval()

    f = net.f
    out = {
        "policy bias zeroed": mut(lambda m: m.policy.bias.zero_()),
        "policy weights x 1.001": mut(lambda m: m.policy.weight.mul_(1.001)),
        "res0.conv1 centre taps x 1.001": mut(lambda m: m.res[0].conv1.weight[:, :, 1, 1].mul_(1.001)),
        "res0.conv1 corner tap of one output channel zeroed": mut(lambda m: m.res[0].conv1.weight[f // 2, :, 0, 0].zero_()),
        "BatchNorm eps 2e-5": mut(lambda m: [setattr(b, "eps", 2e-5) for b in m.modules() if isinstance(b, torch.nn.BatchNorm2d)]),
        "value bias + 1e-3": mut(lambda m: m.value.bias.add_(1e-3)),
    }
    if net.head == "conv":
        n2 = net.n * net.n

        def swap(p, v):  # channel 0 and channel 1 of the same square exchanged: p = ch·N² + sq written with another channel order
            p = p.copy()
            p[:, [0, n2]] = p[:, [n2, 0]]
            return p, v

        out["conv head outputs (ch 0, sq 0) and (ch 1, sq 0) swapped"] = swap
    return out


@pytest.mark.parametrize("n,blocks,filters,head", TOPOLOGIES, ids=[f"{t[0]}x{t[0]}_{t[3]}" for t in TOPOLOGIES])
def test_gates_accept_pytorch_f32_and_reject_every_mutation(orc, n, blocks, filters, head):
    net, planes, ref = _setup(orc, n, blocks, filters, head)
    # the network is what the gates are meant for: peaked policy, saturated values, BatchNorm variances of the order of eps
    pmax = np.exp(ref["logp"].max(1))
    assert np.median(pmax) >= 0.15 and np.abs(ref["v"]).max() >= 0.99 and ref["logp"].min() < -20
    assert min(float(b.running_var.min()) for b in net.modules() if isinstance(b, torch.nn.BatchNorm2d)) <= 1e-4
    p, v = torch_ref.forward(net, planes)
    torch_ref.report(f"pytorch-f32 {n}x{n} {head}", torch_ref.check_forward(p, v, ref, "f32", "unmutated PyTorch fp32"))
    passed = []
    for name, m in _mutations(net).items():
        pm, vm = m(p, v) if callable(m) and not isinstance(m, torch.nn.Module) else torch_ref.forward(m, planes)
        for precision in ("f32", "bf16x3"):
            try:
                torch_ref.check_forward(pm, vm, ref, precision, name)
            except AssertionError as ex:
                print(f"rejected under {precision}: {ex}")
                continue
            passed.append(f"{name} ({precision})")
    assert not passed, f"mutations the gates let through: {passed}"


def test_forward64_training_mode_is_forward_training(orc):
    """forward64(training=True) is PyTorch's forward_training in float64 (BatchNorm on the batch statistics)"""
    n = 5
    net, planes, _ = _setup(orc, n, 1, 32, "fc5")
    ref = torch_ref.forward64(net, planes[:64], training=True)
    n32 = copy.deepcopy(net).train()
    with torch.no_grad():
        logp, v = n32.forward_training(torch.from_numpy(planes[:64]))
    torch_ref.report("pytorch-f32 training forward", torch_ref.check_logp(logp.numpy(), ref, "f32"))
    assert np.abs(v.numpy()[:, 0] - ref["v"]).max() < 1e-5
    # eval mode is another function of the same weights
    assert np.abs(torch_ref.forward64(net, planes[:64])["logp"] - ref["logp"]).max() > 1e-3
