"""Plain PyTorch fp32 statement of the reference's networks (alpha-tak/src/model/{net5,net6,res_block}.rs),
used as the arithmetic oracle for the HIP network kernels: libtorch's conv2d / batch_norm(eval) / relu /
linear / softmax / tanh are the same ATen ops tch-rs calls.  Test infrastructure only."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def input_channels(n):
    stones, caps = {3: (10, 0), 4: (15, 0), 5: (21, 1), 6: (30, 1)}[n]
    return (n + 2 + 6) * 2 + 2 + 2 * stones + 2 * caps


class ResBlock(nn.Module):  # res_block.rs:13-24
    def __init__(self, f):
        super().__init__()
        self.conv1 = nn.Conv2d(f, f, 3, padding=1)
        self.conv2 = nn.Conv2d(f, f, 3, padding=1)
        self.bn1 = nn.BatchNorm2d(f)
        self.bn2 = nn.BatchNorm2d(f)

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)))
        y = self.bn2(self.conv2(y))
        return F.relu(y + x)


class TakNet(nn.Module):
    """head 'fc5' = Net5 (net5.rs:19-131), head 'conv' = Net6 (net6.rs:19-139); blocks/filters runtime."""

    def __init__(self, n, res_blocks, filters, head):
        super().__init__()
        self.n, self.head, self.f = n, head, filters
        self.conv0 = nn.Conv2d(input_channels(n), filters, 3, padding=1)
        self.bn0 = nn.BatchNorm2d(filters)
        self.res = nn.ModuleList([ResBlock(filters) for _ in range(res_blocks)])
        if head == "fc5":
            assert n == 5
            self.policy = nn.Linear(filters * 25, 1575)
        else:
            self.policy = nn.Conv2d(filters, 3 + 4 * (2 ** n - 2), 3, padding=1)
        self.value = nn.Linear(filters * n * n, 1)

    def forward(self, x):  # forward_mcts (eval mode BN)
        s = F.relu(self.bn0(self.conv0(x)))
        for blk in self.res:
            s = blk(s)
        if self.head == "fc5":
            p = self.policy(s.reshape(s.shape[0], -1))
        else:
            p = self.policy(s).reshape(s.shape[0], -1)
        p = torch.softmax(p, dim=1)
        v = torch.tanh(self.value(s.reshape(s.shape[0], -1)))
        return p, v[:, 0]


    def forward_training(self, x):  # forward_training (net5.rs:113-118 / net6.rs:111-122): log_softmax, BN per self.training
        s = F.relu(self.bn0(self.conv0(x)))
        for blk in self.res:
            s = blk(s)
        if self.head == "fc5":
            p = self.policy(s.reshape(s.shape[0], -1))
        else:
            p = self.policy(s).reshape(s.shape[0], -1)
        return torch.log_softmax(p, dim=1), torch.tanh(self.value(s.reshape(s.shape[0], -1)))


def make_net(n, res_blocks, filters, head, seed=0, randomize_bn=True):
    torch.manual_seed(seed)
    net = TakNet(n, res_blocks, filters, head)
    if randomize_bn:  # exercise the BN fold: non-trivial affine + running statistics
        g = torch.Generator().manual_seed(seed + 1)
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.data = torch.rand(m.num_features, generator=g) * 1.0 + 0.5
                m.bias.data = torch.randn(m.num_features, generator=g) * 0.1
                m.running_mean = torch.randn(m.num_features, generator=g) * 0.1
                m.running_var = torch.rand(m.num_features, generator=g) * 1.0 + 0.5
    return net.eval()


def abi_tensors(net):
    """state_dict → {ABI tensor name: float32 array} (names of include/takgpu.h)."""
    out = {}
    for k, v in net.state_dict().items():
        if k.endswith("num_batches_tracked"):
            continue
        parts = k.split(".")
        if parts[0] == "res":
            name = f"res{parts[1]}." + ".".join(parts[2:])
        else:
            name = k
        out[name] = v.detach().cpu().numpy().astype(np.float32)
    return out


def load_abi_tensors(net, tensors):
    """inverse of abi_tensors: {ABI tensor name: array} → the module's parameters and buffers"""
    sd = net.state_dict()
    for k in list(sd.keys()):
        if k.endswith("num_batches_tracked"):
            continue
        sd[k] = torch.from_numpy(np.ascontiguousarray(tensors[abi_name(k)], np.float32)).reshape(sd[k].shape).clone()
    net.load_state_dict(sd)
    return net.eval()


@torch.no_grad()
def forward(net, planes):
    p, v = net(torch.from_numpy(np.ascontiguousarray(planes, np.float32)))
    return p.numpy(), v.numpy()


def abi_name(k):
    parts = k.split(".")
    return f"res{parts[1]}." + ".".join(parts[2:]) if parts[0] == "res" else k


def train_chunk(net, planes, pi, z):
    """train_inner (alpha-tak/src/model/network.rs:58-91): BN in training mode, loss_p = −Σπ·logp / B,
    loss_z = Σ(z − v)² / B, backward (gradients accumulate in .grad).  Returns (loss_p, loss_z)."""
    net.train()
    x = torch.from_numpy(np.ascontiguousarray(planes, np.float32))
    p = torch.from_numpy(np.ascontiguousarray(pi, np.float32))
    zt = torch.from_numpy(np.ascontiguousarray(z, np.float32))[:, None]
    logp, v = net.forward_training(x)
    b = x.shape[0]
    loss_p = -(p * logp).sum() / b
    loss_z = (zt - v).square().sum() / b
    (loss_z + loss_p).backward()
    return float(loss_p.detach()), float(loss_z.detach())


def make_adam(net, lr=1e-4, wd=1e-4):
    """Adam { wd, ..Default::default() }.build(vs, lr) (network.rs:40-45): torch::optim::Adam with L2 weight decay"""
    return torch.optim.Adam(net.parameters(), lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)


def named_grads(net):
    return {abi_name(k): v.grad.detach().numpy().copy() for k, v in net.named_parameters()}


def fp64_gradients(net, planes, pi, z, mask_sets, verbose=False, hook=None, dtype=torch.float64, keep_layers=None):
    """fp64 forward of train_inner's loss (network.rs:58-91) on a copy of `net`, then one backward pass per entry of mask_sets:
    None = the fp64 network's own ReLU decisions, a float t = the decisions taken at y > t, a list of 1 + 2·blocks bool tensors
    [B, F, n, n] = THOSE decisions (layer order conv0, res0.conv1, res0.conv2, …).  The backward pass of a ReLU network is the exact
    derivative of a piecewise-linear function once the decisions are fixed, and the forward pass takes them: with an
    implementation's own decisions on the reference side its gradients have to agree to rounding, with no allowance for "flips".
    hook (tests/test_train_gates.py: how a deliberately wrong operation is put on the reference side) may replace operations of the
    fp64 network: {"conv": f(layer, module, x) → z, "bn": f(layer, module, z) → BatchNorm output, "policy": f(module, x) → logits}
    with layer = 0 for conv0 / bn0, 1 + 2·i and 2 + 2·i for block i; an absent entry is the module itself.  Two more entries replace the
    losses' sums (tests/test_train_gates_trained.py): "policy_loss": f(logits, π) → −Σ π·log_softmax(logits), "value_loss": f(pre, z) →
    Σ (z − tanh(pre))², both before the division by the batch size.
    dtype = torch.float32 runs the same graph in PyTorch f32 under the same decisions: the yardstick a per-slice gate is derived from.
    keep_layers: conv layers whose output z and input x keep their gradients; every result dict then also holds "dz/<layer>" and
    "dx/<layer>" as [rows][channels] arrays in tg_train_debug_read's NHWC order (dx of conv1 of a block includes the skip path's gradient).
    → ([{ABI name: gradient}], [pre-activation of every ReLU, tensors of `dtype`])"""
    import copy

    class Relu(torch.autograd.Function):
        mode = None

        @staticmethod
        def forward(ctx, x, layer):
            ctx.save_for_backward(x)
            ctx.layer = layer
            return x.clamp_min(0.0)

        @staticmethod
        def backward(ctx, g):
            (x,) = ctx.saved_tensors
            m = Relu.mode
            if m is None:
                return g * (x > 0.0), None
            if isinstance(m, float):
                return g * (x > m), None
            return g * m[ctx.layer], None

    n64 = copy.deepcopy(net).to(dtype).train()
    for p in n64.parameters():
        p.grad = None
    keep_layers = sorted(keep_layers or [])
    x = torch.from_numpy(np.ascontiguousarray(planes, np.float64)).to(dtype)
    if 0 in keep_layers:
        x.requires_grad_(True)
    pres, kept = [], {}

    def relu(t):
        pres.append(t.detach())
        return Relu.apply(t, len(pres) - 1)

    hook = hook or {}
    conv_op = hook.get("conv", lambda layer, m, t: m(t))

    def conv(layer, m, t):
        out = conv_op(layer, m, t)
        if layer in keep_layers:
            kept[layer] = (out, t)
        return out

    bn = hook.get("bn", lambda layer, m, t: m(t))
    policy = hook.get("policy", lambda m, t: m(t))
    s = relu(bn(0, n64.bn0, conv(0, n64.conv0, x)))
    for i, blk in enumerate(n64.res):  # res_block.rs:13-24
        y = relu(bn(2 * i + 1, blk.bn1, conv(2 * i + 1, blk.conv1, s)))
        s = relu(bn(2 * i + 2, blk.bn2, conv(2 * i + 2, blk.conv2, y)) + s)
    flat = s.reshape(s.shape[0], -1)
    logits = policy(n64.policy, flat) if n64.head == "fc5" else policy(n64.policy, s).reshape(s.shape[0], -1)
    policy_loss = hook.get("policy_loss", lambda lg, t: -(t * torch.log_softmax(lg, dim=1)).sum())
    value_loss = hook.get("value_loss", lambda pre, t: (t - torch.tanh(pre)).square().sum())
    b = x.shape[0]
    pi_t = torch.from_numpy(np.ascontiguousarray(pi, np.float64)).to(dtype)
    z_t = torch.from_numpy(np.asarray(z, np.float64)).to(dtype)[:, None]
    loss = policy_loss(logits, pi_t) / b + value_loss(n64.value(flat), z_t) / b
    params = list(n64.named_parameters())
    extra = [(f"{what}/{l}", kept[l][i]) for l in keep_layers for i, what in enumerate(("dz", "dx"))]
    out = []
    for i, m in enumerate(mask_sets):
        Relu.mode = m
        gs = torch.autograd.grad(loss, [p for _, p in params] + [t for _, t in extra], retain_graph=i + 1 < len(mask_sets))
        out.append({abi_name(k): g.numpy().copy() for (k, _), g in zip(params, gs)})
        for (k, _), g in zip(extra, gs[len(params):]):
            out[-1][k] = g.permute(0, 2, 3, 1).reshape(-1, g.shape[1]).numpy().copy()
        if verbose:
            print(f"  fp64 backward pass {i + 1} of {len(mask_sets)} done", flush=True)
    return out, pres


def engine_relu_decisions(engine, layers, positions, n, filters):
    """the ReLU decisions an engine took in its last training chunk / forward — y > 0 of every conv layer, read back through
    tg_train_debug_read ([rows][F] NHWC) — as bool tensors [B, F, n, n] for fp64_gradients"""
    rows = positions * n * n
    return [torch.from_numpy(engine.train_debug_read("y", l, (rows, filters)) > 0).reshape(positions, n, n, filters).permute(0, 3, 1, 2)
            for l in range(layers)]


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 reference and the forward gates.  make_net's default-initialised networks have an almost flat policy (largest p ≈ 1e-3, on 6×6
# ≈ 3e-4) and |v| < 0.4, so an absolute 1e-4 gate on p cannot see a dropped bias or a per-mille mis-scale.  The gates below work in log
# space against a float64 forward, and make_trained_net builds networks whose outputs look like a trained one's: peaked policies,
# saturated values, BatchNorm channels whose running variance is of the order of eps.
# ---------------------------------------------------------------------------------------------------------------------------------

LOGP_FLOOR = -30.0   # below it an entry is "tiny": only 0 ≤ p ≤ TINY_P is asked of it
TINY_P = 1e-12

# One set of constants per precision.  For every entry with log p64 ≥ LOGP_FLOOR:  |log p − log p64| ≤ a + b·|log p64|;  per row
# Σ|p − p64| / 2 ≤ t;  |v − v64| ≤ c·(1 − v64²) + 2⁻²³  (c bounds the error of the value's pre-activation, tanh′ = 1 − v²).
# b comes from the arithmetic, not from a fit: the FC path's softmax takes exp(x − M) as v_exp_f32((x − M)·log2 e) (softmax.cuh, stat_exp);
# the rounding of x − M and of the product by log2 e are each ≤ 2⁻²⁴ relative, i.e. ≤ 2⁻²⁴·|x − M| ≤ 2⁻²⁴·|log p| in the natural log:
# b = 2·log2 e·2⁻²⁴ (≈ 1.7e-7) covers both with the log2 e factor of the base-2 form to spare.
# a, t and c sit 2 – 3× above the engine's worst error measured on an MI355X over the whole GPU suite (every case check_forward,
# check_logp or check_priors gates — the trained-like sweeps of tests/test_gpu_fp64.py and, for the two f32 maxima at K = 4800 / 6400 of
# the policy FC, tests/test_gpu_topology_forward.py set every maximum):
#              worst |Δlog p| − b·|log p64|          worst row TV                  worst |Δv| − 2⁻²³ over (1 − v64²)
#   f32        6.5e-5 (5×5×128 FC, planes, B=65)     1.0e-5 (5×5×256 FC, B=2049)   1.1e-5 (5×5×192 FC, B=2049)
#   bf16x3     3.1e-4 (6×6×128 conv, planes, B=700)  3.9e-5 (6×6×128 conv, B=700)  9.8e-5 (5×5×64 FC, B=2400)
# (PyTorch's own fp32 forward on the same kind of networks: ≤ 1.3e-5, 2.1e-6, 5.9e-6.  Networks of 49 layers are gated at these constants
# times the reference's own depth growth, depth_scaled_gates: the engine's worst there 3.5e-5, 4.8e-6, 1.2e-5 under ratios of 2 – 6.)  The teeth test (tests/test_forward_gates.py)
# rejects each of its mutations under both sets; the smallest of them, a value bias off by 1e-3, is 1e-3 of pre-activation error.
_B_EXP = 2.0 * 1.4426950408889634 * 2.0 ** -24
GATES = {
    "f32": dict(a=2e-4, b=_B_EXP, t=2e-5, c=3e-5),
    "bf16x3": dict(a=1e-3, b=_B_EXP, t=1e-4, c=3e-4),
}


def _layers64(net, x, training):
    """shared body of the fp64 forwards: (tower output s, policy logits, value pre-activation), all float64 tensors"""
    import copy

    n64 = copy.deepcopy(net).double()
    n64.train(training)
    s = F.relu(n64.bn0(n64.conv0(x)))
    for blk in n64.res:
        s = blk(s)
    flat = s.reshape(s.shape[0], -1)
    logits = n64.policy(flat) if n64.head == "fc5" else n64.policy(s).reshape(s.shape[0], -1)
    return logits, n64.value(flat)[:, 0]


@torch.no_grad()
def forward64(net, planes, training=False, chunk=512):
    """float64 forward of `net` on `planes`: BatchNorm in eval mode (forward_mcts) or, training=True, on the batch's own statistics
    (forward_training; one batch, not chunked).  → dict(logits, logp = log_softmax over all outputs, pre = the value's pre-activation,
    v = tanh(pre)), float64 numpy arrays."""
    planes = np.ascontiguousarray(planes, np.float64)
    step = len(planes) if training else chunk
    parts = [_layers64(net, torch.from_numpy(planes[lo: lo + step]), training) for lo in range(0, max(len(planes), 1), step)]
    logits = torch.cat([p[0] for p in parts])
    pre = torch.cat([p[1] for p in parts])
    return dict(logits=logits.numpy(), logp=torch.log_softmax(logits, dim=1).numpy(), pre=pre.numpy(), v=torch.tanh(pre).numpy())


@torch.no_grad()
def batch_statistics64(net, planes):
    """the batch mean and (biased) variance every BatchNorm of `net` normalises `planes` with in training mode, in float64:
    [(mean, var)] in layer order conv0, res0.conv1, res0.conv2, …"""
    import copy

    n64 = copy.deepcopy(net).double().train()
    bns = [n64.bn0] + [b for blk in n64.res for b in (blk.bn1, blk.bn2)]
    for m in bns:
        m.momentum = 1.0
    x = torch.from_numpy(np.ascontiguousarray(planes, np.float64))
    n64.forward_training(x)
    rows = x.shape[0] * x.shape[2] * x.shape[3]
    return [(m.running_mean.numpy().copy(), m.running_var.numpy() * (rows - 1) / rows) for m in bns]


def slice_ref(ref, sel):
    return {k: v[sel] for k, v in ref.items()}


def _policy_metrics(p, logp64, g, mask=None):
    """log-space and tiny-entry metrics of probabilities p against log p64 (same shape; mask = entries that take part)"""
    p = np.asarray(p, np.float64)
    keep = np.ones(p.shape, bool) if mask is None else mask
    big = keep & (logp64 >= LOGP_FLOOR)
    tiny = keep & (logp64 < LOGP_FLOOR)
    with np.errstate(divide="ignore"):
        d = np.abs(np.log(np.where(big, p, 1.0)) - np.where(big, logp64, 0.0))
    excess = np.where(big, d - g["b"] * np.abs(logp64), -np.inf)
    bad = np.argwhere(excess > g["a"])
    tv = 0.5 * np.where(keep, np.abs(p - np.exp(logp64)), 0.0).sum(axis=-1)
    m = dict(logp_abs=float(d[big].max()) if big.any() else 0.0, logp_a=float(max(excess.max(), 0.0)) if big.any() else 0.0,
             tv=float(tv.max()) if tv.size else 0.0, tiny_max=float(p[tiny].max()) if tiny.any() else 0.0,
             tiny_neg=bool((p[tiny] < 0).any()) if tiny.any() else False, entries=int(big.sum()), tiny_entries=int(tiny.sum()),
             first_bad=tuple(int(i) for i in bad[0]) if len(bad) else None)
    return m


def _assert_policy(m, g, what):
    assert m["first_bad"] is None, (f"{what}: |log p − log p64| beyond a + b·|log p64| at {m['first_bad']} "
                                    f"(worst excess {m['logp_a']:.3e} > a = {g['a']:.1e})")
    assert not m["tiny_neg"] and m["tiny_max"] <= TINY_P, f"{what}: an entry with log p64 < {LOGP_FLOOR} has p = {m['tiny_max']:.3e}"
    assert m["tv"] <= g["t"], f"{what}: row total variation {m['tv']:.3e} > t = {g['t']:.1e}"


def _forward_metrics(p, v, ref, g, what):
    p = np.asarray(p)
    assert p.shape == ref["logp"].shape and np.shape(v) == ref["v"].shape, (what, p.shape, ref["logp"].shape)
    m = _policy_metrics(p, ref["logp"], g)
    dv = np.abs(np.asarray(v, np.float64) - ref["v"])
    slope = 1.0 - ref["v"] ** 2
    pre = np.maximum(dv - 2.0 ** -23, 0.0) / np.maximum(slope, 1e-300)
    m.update(v_abs=float(dv.max()) if dv.size else 0.0, pre=float(pre.max()) if pre.size else 0.0,
             v_max=float(np.abs(ref["v"]).max()) if dv.size else 0.0, rows=int(p.shape[0]))
    return m, dv, slope


def measure_forward(p, v, ref, what="forward"):
    """check_forward's metrics (logp_a, tv, pre, …) of p, v against forward64's `ref`, with nothing asserted: what a gate that has to
    follow the reference's own error is derived from (depth_scaled_gates)"""
    return _forward_metrics(p, v, ref, GATES["f32"], what)[0]


def depth_scaled_gates(net, shallow, planes, ref, ref_shallow, precision="f32"):
    """GATES[precision] for a network far deeper than the 5-layer ones its constants were set on.  Rounding error grows with depth; how
    much is read off the REFERENCE, not off the engine: PyTorch fp32's own distance to float64 on `net` over that on `shallow` (the
    same shape with 2 blocks), on the same `planes`, metric by metric.  a, t and c are multiplied by max(1, ratio of logp_a, tv, pre);
    b (the exp's argument rounding) does not depend on depth.  → (gates, ratios, PyTorch fp32's metrics on net, on shallow)"""
    deep = measure_forward(*forward(net, planes), ref, "PyTorch fp32, deep")
    flat = measure_forward(*forward(shallow, planes), ref_shallow, "PyTorch fp32, 2 blocks")
    ratios = {k: deep[k] / flat[k] for k in ("logp_a", "tv", "pre")}
    g = dict(GATES[precision])
    for const, metric in (("a", "logp_a"), ("t", "tv"), ("c", "pre")):
        g[const] *= max(1.0, ratios[metric])
    return g, ratios, deep, flat


def check_forward(p, v, ref, precision, what="forward", gates=None):
    """The forward gates of `precision` (GATES) on an engine's (or any) probabilities p [B, P] and values v [B] against forward64's `ref`
    (the same rows).  Asserts, naming `what` and the gate that failed; returns the measured metrics.
    gates: constants in GATES' form that take the place of GATES[precision] (depth_scaled_gates: networks far deeper than the ones
    the constants were set on)."""
    g = GATES[precision] if gates is None else gates
    p = np.asarray(p)
    m, dv, slope = _forward_metrics(p, v, ref, g, what)
    _assert_policy(m, g, what)
    assert (dv <= g["c"] * slope + 2.0 ** -23).all(), (f"{what}: |v − v64| beyond c·(1 − v64²) + 2⁻²³ "
                                                       f"(implied pre-tanh error {m['pre']:.3e} > c = {g['c']:.1e})")
    return m


def check_logp(logp, ref, precision, what="log_softmax"):
    """check_forward's policy gates on log-probabilities (forward_training's output) instead of probabilities"""
    g = GATES[precision]
    m = _policy_metrics(np.exp(np.asarray(logp, np.float64)), ref["logp"], g)
    _assert_policy(m, g, what)
    return m


def check_priors(prior, logp64, mask, precision, what="priors"):
    """the policy gates on the entries of p64 a tree's children carry (prior[g, i] against logp64[g, i] where mask[g, i])"""
    g = GATES[precision]
    m = _policy_metrics(np.where(mask, prior, 0.0), np.where(mask, logp64, 0.0), g, mask=mask)
    _assert_policy(m, g, what)
    return m


def report(name, m):
    """one line per gated case (the table of DESIGN.md §4 is read off these)"""
    keys = ("logp_a", "logp_abs", "tv", "tiny_max", "pre", "v_abs", "v_max", "rows")
    print("fp64-gate " + name + ": " + ", ".join(f"{k} {m[k]:.3e}" if isinstance(m[k], float) else f"{k} {m[k]}" for k in keys if k in m),
          flush=True)
    return m


@torch.no_grad()
def make_trained_net(n, res_blocks, filters, head, planes, seed=0, logit_std=3.0, value_std=1.5, quiet_layers=None, quiet_channels=2):
    """A network whose outputs look like a trained one's, built around make_net's random weights (make_net itself stays as it is):
      * BatchNorm running statistics are the network's own activations on `planes` (one training-mode pass, momentum 1);
      * in `quiet_layers` (default: conv0, the first block's conv1, the last conv) `quiet_channels` output channels are nearly constant:
        their conv weights are scaled so the running variance lands near 3e-5 (≤ 1e-4, the order of eps = 1e-5), while the normalised
        output stays O(1) — so eps, and the host fold's rounding of var + eps, change the result visibly;
      * the policy logits have a standard deviation of `logit_std` over the batch, widened in steps of 10 % until the median largest
        probability is ≥ 0.2 (a peaked policy), with a bias of its own of the order of 1;
      * the value pre-activation has a standard deviation of `value_std` (some |v| ≥ 0.99).
    Returns the network in eval mode."""
    net = make_net(n, res_blocks, filters, head, seed=seed, randomize_bn=True)
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.from_numpy(np.ascontiguousarray(planes, np.float32))
    convs = [net.conv0] + [c for blk in net.res for c in (blk.conv1, blk.conv2)]
    bns = [net.bn0] + [b for blk in net.res for b in (blk.bn1, blk.bn2)]
    if quiet_layers is None:
        quiet_layers = sorted({0, 1 if res_blocks else 0, len(convs) - 1})

    def calibrate():
        for m in bns:
            m.momentum = 1.0
        net.train()
        net.forward_training(x)
        net.eval()

    for li in quiet_layers:
        calibrate()
        var = bns[li].running_var
        ch = torch.randperm(filters, generator=g)[:quiet_channels]
        for c in ch.tolist():
            s = float(np.sqrt(3e-5 / max(float(var[c]), 1e-12)))
            convs[li].weight[c] *= s
            convs[li].bias[c] *= s
    calibrate()
    for m in bns:
        m.momentum = 0.1
    # heads: scale to the wanted spreads, then give the policy a bias of the order of its logits
    s = F.relu(net.bn0(net.conv0(x)))
    for blk in net.res:
        s = blk(s)
    flat = s.reshape(s.shape[0], -1)
    logits = net.policy(flat) if head == "fc5" else net.policy(s).reshape(s.shape[0], -1)
    bias = torch.randn(net.policy.bias.shape, generator=g) * 0.5 * logit_std / 3.0
    raw = logits - net.policy.bias if head == "fc5" else logits - net.policy.bias.repeat_interleave(n * n)
    full_bias = bias if head == "fc5" else bias.repeat_interleave(n * n)
    k = logit_std / float(raw.std())
    for _ in range(20):  # a little wider where the spread alone leaves the policy flatter than a trained one's
        if float(torch.softmax(k * raw + full_bias, dim=1).max(dim=1).values.median()) >= 0.2:
            break
        k *= 1.1
    net.policy.weight *= k
    net.policy.bias.copy_(bias)
    pre = net.value(flat)[:, 0]
    kv = value_std / float(pre.std())
    net.value.weight *= kv
    net.value.bias.copy_(0.2 - kv * (pre.mean() - net.value.bias))  # centred: the pre-activation spans about ±4
    return net.eval()


# ---------------------------------------------------------------------------------------------------------------------------------
# Per-slice gates of the training step's gradients (tests/test_gpu_train_trained.py, tests/test_train_gates_trained.py).  A relative
# norm over a whole tensor hides an error confined to one output channel, and on a trained-like network (make_trained_net: quiet
# channels) the channels of one tensor differ in scale by two orders of magnitude.  So every tensor is also compared slice by slice —
# conv weights per output channel, BatchNorm weights and biases per element, the FC policy head per group of 64 outputs (the conv head per
# output channel), value.weight per input channel — each slice relative to ITS OWN fp64 norm.  A slice whose fp64 norm is below
# SLICE_FLOOR × the tensor's RMS slice norm is compared absolutely against that floor and counts as left out (at most SLICE_FLOORED_CAP
# of a tensor's slices).
# The tolerances are not chosen: TRAIN_SLICE_F32 is the worst per-slice distance of PyTorch FLOAT32 autograd to fp64 under the same ReLU
# decisions (fp64_gradients(dtype=torch.float32)), per tensor class, over the cases of tests/test_gpu_train_trained.py, two accumulated
# chunks each, measured on the CPU (python tests/test_train_gates_trained.py prints the table); the gate of a class is
# max(2e-5, 3 × that) — 3 for another, equally valid summation order, the margin of GATES above.
# ---------------------------------------------------------------------------------------------------------------------------------
SLICE_FLOOR = 1e-6
SLICE_FLOORED_CAP = 0.02
# A slice of ONE element (a BatchNorm weight's or bias's gradient) is a sum over all rows that can cancel to any degree, and its fp64
# value moves by up to 1e-4 of the tensor's RMS element between equally valid sets of ReLU decisions (8e-5 between PyTorch f32's and
# fp64's own decisions on one element of the 33-example 5×5 case).  An element closer to zero than SLICE_CONDITION × RMS has a relative
# error that is a property of the decision set, not of the arithmetic (PyTorch f32's own error on such an element: 5e-3 under one set,
# 0.34 under the other, at the same absolute error), and no f32-derived gate means anything there.  test_gpu_train.trained_case asserts,
# on the fp64 reference alone, that its seed leaves no such element.
SLICE_CONDITION = 1e-3
TENSOR_GATE = 2e-5
TRAIN_SLICE_F32 = {
    "conv.weight": 2.25e-6, "bn.weight": 1.80e-4, "bn.bias": 9.90e-4, "policy.weight": 6.14e-6, "policy.bias": 9.25e-5,
    "value.weight": 3.45e-6, "value.bias": 3.77e-6, "dz": 1.49e-6, "dx": 1.07e-5,
    # test_gpu_train.value_sub_batches: every row at |v| ≥ 0.99, where PyTorch's own 1 − v² loses its digits too
    "value.weight.saturated": 1.42e-5, "value.bias.saturated": 1.71e-6,
}


def slice_gate(cls):
    return max(TENSOR_GATE, 3.0 * TRAIN_SLICE_F32[cls])


def bias_before_bn(name):
    """a conv bias in front of a BatchNorm: true gradient exactly zero, outside every relative gate"""
    return name.endswith(".bias") and "conv" in name and not name.startswith("policy")


def slice_class(name):
    if name.startswith(("policy.", "value.", "dz", "dx")):
        return name.split("/")[0]
    if "bn" in name.split(".")[-2]:
        return "bn." + name.split(".")[-1]
    return "conv." + name.split(".")[-1]


def slice_view(name, a, head, n):
    """gradient tensor → float64 [slices, elements per slice] (module comment above)"""
    a = np.asarray(a, np.float64)
    if name.startswith(("dz", "dx")):
        return a.T if name.startswith("dz") else a.reshape(-1, n * n * a.shape[1])   # dz per channel, dx per position
    if name == "value.weight":
        return a.reshape(-1, n * n)
    if name.startswith("policy.") and head == "fc5":
        rows = a.reshape(a.shape[0], -1)
        pad = -rows.shape[0] % 64
        return np.concatenate([rows, np.zeros((pad, rows.shape[1]))]).reshape(-1, 64 * rows.shape[1])
    if a.ndim == 4 or name.startswith("policy."):
        return a.reshape(a.shape[0], -1)
    return a.reshape(-1, 1)


def slice_distances(name, g, ref, head, n):
    """→ (per-slice ‖g − ref‖ / max(‖ref‖, floor), which slices are floored)"""
    G, R = slice_view(name, g, head, n), slice_view(name, ref, head, n)
    nr = np.linalg.norm(R, axis=1)
    floor = SLICE_FLOOR * np.sqrt((nr ** 2).mean())
    return np.linalg.norm(G - R, axis=1) / np.maximum(nr, floor), nr < floor


def compare_slices(grads, ref, head, n, gates=None, what="", classes=None):
    """Every gated tensor of `grads` against `ref` ({ABI name: array}, the conv biases in front of a BatchNorm left out): whole-tensor
    relative norm and the per-slice distances.  gates = None measures only; gates = slice_gate asserts tensor ≤ TENSOR_GATE, every
    slice ≤ gates(class) (of `classes` only, where given) and the cap on floored slices.  → {class: (worst slice distance, tensor, slice)}, (worst tensor, its distance)"""
    worst_slice, worst_tensor = {}, ("", 0.0)
    for name in ref:
        if bias_before_bn(name):
            continue
        r64 = np.asarray(ref[name], np.float64)
        whole = float(np.linalg.norm(np.asarray(grads[name], np.float64) - r64) / np.linalg.norm(r64))
        d, floored = slice_distances(name, grads[name], ref[name], head, n)
        cls, i = slice_class(name), int(np.argmax(d))
        if float(d[i]) >= worst_slice.get(cls, (-1.0,))[0]:
            worst_slice[cls] = (float(d[i]), name, i)
        if not name.startswith(("dz", "dx")):
            worst_tensor = max(worst_tensor, (name, whole), key=lambda t: t[1])
        if gates is not None:
            assert floored.mean() <= SLICE_FLOORED_CAP, (what, name, "floored slices", int(floored.sum()), len(floored))
            assert name.startswith(("dz", "dx")) or whole <= TENSOR_GATE, (what, name, "whole tensor against fp64", whole)
            assert (classes is not None and cls not in classes) or d[i] <= gates(cls), (what, name, f"slice {i} against fp64, relative to its own norm", float(d[i]), gates(cls))
    return worst_slice, worst_tensor
