"""The teeth of tests/test_gpu_topology_forward.py, on the CPU, in the manner of tests/test_forward_gates.py: on three of its
topologies — built by its own build_case, the same networks, rows, float64 reference and gates — PyTorch's fp32 forward passes the gate
the GPU test applies (the depth-scaled one on the 49-layer network), and mistakes of the kind the per-layer kernels can make are
rejected under that same gate: the half K-step of the policy FC dropped, the padded column block of a layer zeroed, one position
convolved with another square's tap mask, the last block's residual added twice or not at all, the value head over a part of the
channels.  And the depth ratio the 49-layer gates are scaled by stays between 1 and 10: outside, the reference or the networks changed."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_forward_gates
import test_gpu_topology_forward as topo
import torch_ref

TOPOLOGIES = ["5x5_1x96_fc", "6x6_1x96_conv", "5x5_24x64_fc"]
_built = {}


def _case(orc, name):
    if name not in _built:
        _built[name] = topo.build_case(orc, name)
    return _built[name]


def _mutations(net):
    """name → mutated copy of `net`"""
    def mut(f):
        m = copy.deepcopy(net)
        with torch.no_grad():
            f(m)
        return m.eval()

    f, n = net.f, net.n
    nsq = n * n

    def k_tail(m):
        # the engine's K order is (square, channel): its last 32 are channels f − 32 … f − 1 of the last square (fc5), of every tap (conv)
        if m.head == "fc5":
            m.policy.weight.view(-1, f, nsq)[:, f - 32:, nsq - 1].zero_()
        else:
            m.policy.weight[:, f - 32:].zero_()

    def zero_upper_channels(m):
        m.bn0.register_forward_hook(lambda mod, inp, out: torch.cat([out[:, :64], torch.zeros_like(out[:, 64:])], dim=1))

    def wrong_tap_mask(m):
        def hook(mod, inp, out):  # the last position's square (1, 1) with the mask of the corner (0, 0): the taps of row −1 and column −1 lost
            w = mod.weight.clone()
            w[:, :, 1:, 1:] = 0.0
            out = out.clone()
            out[-1, :, 1, 1] -= F.conv2d(inp[0][-1:], w, padding=1)[0, :, 1, 1]
            return out
        m.res[-1].conv1.register_forward_hook(hook)

    def residual_times(k):
        def apply(m):
            def forward(self, x):
                y = F.relu(self.bn1(self.conv1(x)))
                return F.relu(self.bn2(self.conv2(y)) + k * x)
            m.res[-1].forward = types.MethodType(forward, m.res[-1])
        return apply

    out = {
        "the last 32 of K dropped from the policy head": mut(k_tail),
        "the last position convolved with another square's tap mask": mut(wrong_tap_mask),
        "the last block's residual added twice": mut(residual_times(2.0)),
        "the last block's residual not added": mut(residual_times(0.0)),
    }
    if f > 64:
        out["output channels >= 64 of conv0 zeroed"] = mut(zero_upper_channels)
        out["the value head over the first 64 channels only"] = mut(lambda m: m.value.weight.view(1, f, nsq)[:, 64:].zero_())
    else:  # (one column block, a value head within 128 channels: the small mutations of tests/test_forward_gates.py instead)
        out.update({k: v for k, v in test_forward_gates._mutations(net).items() if isinstance(v, torch.nn.Module)})
    return out


@pytest.mark.parametrize("name", TOPOLOGIES)
def test_gate_accepts_pytorch_f32_and_rejects_every_mutation(orc, name):
    c = _case(orc, name)
    planes = c["planes"][c["rows"]]
    assert (c["gates"] is not None) == (name == "5x5_24x64_fc")
    p, v = torch_ref.forward(c["net"], planes)
    torch_ref.report(f"pytorch-f32 {name}", torch_ref.check_forward(p, v, c["ref"], "f32", "unmutated PyTorch fp32", gates=c["gates"]))
    passed = []
    for what, m in _mutations(c["net"]).items():
        pm, vm = torch_ref.forward(m, planes)
        assert not (np.array_equal(pm, p) and np.array_equal(vm, v)), f"{what}: the mutation changed nothing"
        try:
            torch_ref.check_forward(pm, vm, c["ref"], "f32", what, gates=c["gates"])
        except AssertionError as ex:
            print(f"rejected: {ex}")
            continue
        passed.append(what)
    assert not passed, f"mutations the gate of {name} lets through: {passed}"


@pytest.mark.parametrize("name", ["5x5_24x64_fc", "6x6_24x128_conv"])
def test_depth_ratio_is_the_references_own_growth(orc, name):
    c = _case(orc, name)
    print(f"depth-ratio {name}: {c['ratios']}")
    for metric, r in c["ratios"].items():
        assert 1.0 <= r <= 10.0, (name, metric, r)
    g, g0 = c["gates"], torch_ref.GATES["f32"]
    assert g["b"] == g0["b"] and all(g0[k] <= g[k] <= 10.0 * g0[k] for k in "atc")
