"""The corner positions of tests/posgen.py (repr_corner_states) and what the forward gates see on them, on the CPU.

Positions from random play leave a quarter of game_repr's input planes zero in every position (buried stones six and more below the
top, low reserve counts, a negative or odd komi), so a network whose layer 0 ignores such a channel passes every gate fed by them.  First
half: the corner set sets every plane the board size can set — the 0/1 board planes on every border class of tower_cb_index —, leaves
every plane zero somewhere, and spreads the fcd plane over both signs.  Second half, the gates' teeth on that set: PyTorch fp32 passes
check_forward under "f32", and each mistake of the kind the engine's three statements of game_repr could make (board.cuh's repr_value,
ws_row_mask + tower_cb_board_quads, tower_stage.cuh's tower_cb_table) is rejected under "f32" AND the looser "bf16x3" constants — made
on the reference side: in the planes, in layer 0's weights, or in how conv0 is applied."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import posgen
import torch_ref

NETS = [(5, 64, "fc5"), (6, 128, "conv"), (4, 32, "conv"), (3, 32, "conv")]
_cache = {}


def _corners(orc, n):
    if n not in _cache:
        sts, ok = posgen.repr_corner_states(orc, n)
        _cache[n] = (sts, ok, orc.encode(n, sts))
    return _cache[n]


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_corner_states_are_positions_and_deterministic(orc, n):
    sts, ok, _ = _corners(orc, n)
    again, ok2 = posgen.repr_corner_states(orc, n)
    assert np.array_equal(sts, again) and np.array_equal(ok, ok2)
    assert 200 <= len(sts) <= 500
    assert posgen.is_position(sts, n).all()
    # the index set: ongoing, reserves + board = supplies; enough of them for the search and training cases
    assert len(ok) >= 80 and not orc.result(n, sts[ok]).any() and posgen.reserves_consistent(sts[ok], n).all()
    S, Cc = posgen.STONES[n]
    for colour in ("white", "black"):  # the header sweeps: every count 0 … S / 0 … C under both colours to move
        for tm in (0, 1):
            sel = posgen.header(sts, "to_move") == tm
            assert set(posgen.header(sts[sel], colour + "_stones").tolist()) == set(range(S + 1))
            assert set(posgen.header(sts[sel], colour + "_caps").tolist()) == set(range(Cc + 1))
    hk = set(posgen.header(sts, "half_komi").astype(int).tolist())
    assert hk >= set(range(-6, 7))
    # the oracle plays every legal move of the ongoing, consistent ones
    om, oc = orc.movegen(n, sts[ok])
    assert (oc > 0).all()
    _, status = orc.play(n, sts[ok][np.repeat(np.arange(len(ok)), oc)], np.concatenate([om[i, : oc[i]] for i in range(len(ok))]))
    assert not status.any()


@pytest.mark.parametrize("n", [3, 4, 5, 6])
def test_corner_states_set_every_input_plane(orc, n):
    sts, ok, planes = _corners(orc, n)
    S, Cc = posgen.STONES[n]
    bc, C = 2 * (n + 8), torch_ref.input_channels(n)
    assert planes.shape[1] == C == bc + 2 * S + 2 * Cc + 2
    flat = planes.reshape(len(sts), C, n * n)
    assert set(np.unique(flat[:, : C - 1]).tolist()) == {0.0, 1.0}
    cls = posgen.border_class(n)
    assert sorted(set(cls.tolist())) == list(range(9))
    missing = [(c, k) for c in range(bc) if Cc or c not in (4, 5) for k in range(9) if not flat[:, c][:, cls == k].any()]
    assert not missing, f"(board plane, border class) pairs never set: {missing}"
    if not Cc:
        assert not flat[:, 4:6].any()  # no capstones on 3×3 and 4×4
    assert (np.abs(flat).min(axis=(0, 2)) == 0).all()  # every plane is zero somewhere
    set_in = (flat[:, bc: C - 1].max(axis=2) > 0).sum(axis=0)  # reserve, capstone and colour planes are constant over the board
    assert (flat[:, bc:].min(axis=2) == flat[:, bc:].max(axis=2)).all() and (set_in >= 2).all(), set_in
    fcd = flat[:, C - 1, 0].astype(np.float64) * n * n
    assert np.abs(fcd - np.rint(fcd)).max() < 1e-5
    values = np.unique(np.rint(fcd).astype(int))
    assert len(values) >= 12 and values.min() < 0 < values.max(), values
    # the ongoing, consistent states alone reach every plane too, within the 2 × 40 examples of the training case
    sub = posgen.covering_subset(planes[ok], 80)
    assert (np.abs(planes[ok][sub]).reshape(80, C, -1).max(axis=2) > 0).any(axis=0).sum() == C - (0 if Cc else 2)


class SplitConv0(torch.nn.Module):
    """conv0 as the fused towers apply it: the board planes through the 3×3 convolution, the constant planes (reserves, colour, fcd)
    on their own.  pad = "zeros" is conv0 itself; pad = "replicate" convolves the constant planes as if they went on beyond the
    border — the mistake of a per-position bias that counts an off-board tap, i.e. ignores the border class."""

    def __init__(self, conv, bc, pad):
        super().__init__()
        self.conv, self.bc, self.pad = conv, bc, pad

    def forward(self, x):
        w, bc = self.conv.weight, self.bc
        board = F.conv2d(x[:, :bc], w[:, :bc], self.conv.bias, padding=1)
        const = x[:, bc:]
        const = F.pad(const, (1, 1, 1, 1), mode="replicate") if self.pad == "replicate" else F.pad(const, (1, 1, 1, 1))
        return board + F.conv2d(const, w[:, bc:])


def _plane_mutations(n, sts, planes):
    """name → planes with a mistake of the encoder"""
    S, Cc = posgen.STONES[n]
    bc, nn_ = 2 * (n + 8), n * n
    groups = [(bc, S), (bc + S, S), (bc + 2 * S, Cc), (bc + 2 * S + Cc, Cc)]  # own stones, enemy stones, own caps, enemy caps
    out = {}
    m = planes.copy()
    m[:, bc - 2: bc] = 0.0
    out["deepest buried-stone plane pair dropped (depth cap one short)"] = m
    m = planes.copy()
    for lo, size in groups:
        m[:, lo + 1: lo + size] = planes[:, lo: lo + size - 1]
        m[:, lo] = 0.0
    out["every reserve one-hot shifted up by one"] = m
    m = planes.copy()
    black = planes[:, bc + 2 * S + 2 * Cc, 0, 0] == 0.0
    for (a, size), (b, _) in ((groups[0], groups[1]), (groups[2], groups[3])):
        m[black, a: a + size], m[black, b: b + size] = planes[black, b: b + size], planes[black, a: a + size]
    out["own and enemy reserves exchanged when black is to move"] = m
    m = planes.copy()
    half = np.trunc(posgen.header(sts, "half_komi").astype(np.float64) / 2.0)  # i8 division truncates towards zero
    fcd = np.rint(planes[:, -1, 0, 0].astype(np.float64) * nn_) + 2.0 * half     # flat_diff + half_komi / 2
    m[:, -1] = (fcd / nn_).astype(np.float32)[:, None, None]
    out["half_komi / 2 taken with the sign flipped"] = m
    return out


def _rejected(p, v, ref, name):
    """[precisions under which check_forward lets (p, v) through]"""
    passed = []
    for precision in ("f32", "bf16x3"):
        try:
            torch_ref.check_forward(p, v, ref, precision, name)
        except AssertionError:
            continue
        passed.append(f"{name} ({precision})")
    return passed


@pytest.mark.parametrize("n,filters,head", NETS, ids=[f"{t[0]}x{t[0]}_{t[2]}" for t in NETS])
def test_gates_on_the_corner_set_reject_every_representation_mistake(orc, n, filters, head):
    gates = copy.deepcopy(torch_ref.GATES)
    sts, _, planes = _corners(orc, n)
    net = torch_ref.make_net(n, 1, filters, head, seed=60 + n)
    ref = torch_ref.forward64(net, planes)
    p, v = torch_ref.forward(net, planes)
    torch_ref.report(f"pytorch-f32 corner set {n}x{n} 1x{filters} {head}", torch_ref.check_forward(p, v, ref, "f32", "unmutated PyTorch fp32"))
    bc = 2 * (n + 8)
    # the split form of conv0 is conv0: the zero-padded form passes, so what the replicate form fails on is the padding
    split = copy.deepcopy(net)
    split.conv0 = SplitConv0(split.conv0, bc, "zeros")
    torch_ref.check_forward(*torch_ref.forward(split, planes), ref, "f32", "conv0 split into board and constant planes")
    passed = []
    split.conv0.pad = "replicate"
    passed += _rejected(*torch_ref.forward(split, planes), ref, "constant planes convolved with replicate padding")
    for name, m in _plane_mutations(n, sts, planes).items():
        assert not np.array_equal(m, planes), name
        passed += _rejected(*torch_ref.forward(net, m), ref, name)
    # layer-0 weights of one input channel zeroed, every channel in turn (a weight row packed to the wrong slot reads zeros).  Only rows
    # on which the channel's plane is set can change, and the gates are per entry and per row: 64 such rows stand for the set — a
    # mistake rejected on them is rejected on the whole set
    cannot = (4, 5) if not posgen.STONES[n][1] else ()
    m = copy.deepcopy(net)
    for c in range(planes.shape[1]):
        rows = np.flatnonzero(np.abs(planes[:, c]).max(axis=(1, 2)) > 0)[:64]
        assert (len(rows) == 0) == (c in cannot)  # a plane the board size cannot set: the channel's weights are unreachable
        if c in cannot:
            continue
        with torch.no_grad():
            m.conv0.weight.copy_(net.conv0.weight)
            m.conv0.weight[:, c].zero_()
        passed += _rejected(*torch_ref.forward(m, planes[rows]), torch_ref.slice_ref(ref, rows), f"layer-0 weights of input channel {c} zeroed")
    assert not passed, f"mistakes the gates let through on the corner set: {passed}"
    assert gates == torch_ref.GATES
