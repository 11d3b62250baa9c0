"""tg_policy_eval_symm / tg_policy_eval_symm_dev on the GPU: bit for bit the f32 numpy fold (tests/symm_ref.py, the order
include/takgpu.h states) of tg_policy_eval on oracle.augment's image states through tables built from oracle.augment — in both
precisions, at sizes below, at and across the slicer's cut — plus what follows from it: the device's tables, rows that sum to 1,
equivariance of the full ensemble, the device-pointer variant, independence of the batch."""
import functools

import numpy as np
import pytest

import posgen
import symm_ref
import torch_ref

pytestmark = pytest.mark.gpu

MAX_BATCH = 64  # 65 states × 8 images = 520 rows: the host variant cuts 9 times, the last slice holds one state
MASKS = (0x01, 0x80, 0x24, 0xFF)
U = 2.0 ** -24  # unit roundoff of f32; one "ulp-of-1 step" is 2 U
NETS = {"fc5": (5, 2, 64, "fc5"), "conv6": (6, 1, 32, "conv"), "conv5": (5, 1, 32, "conv")}


@functools.lru_cache(maxsize=None)
def _engine(kind, precision="f32"):
    import tak_amd

    n, blocks, filters, head = NETS[kind]
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, evaluator=tak_amd.EVAL_RESNET, max_batch=MAX_BATCH,
                       policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV)
    if precision != "f32":
        e.set_precision(precision)
    e.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(n, blocks, filters, head, seed=3)))
    return e


@functools.lru_cache(maxsize=None)
def _states(n):
    """65 positions: tall stacks, caps and walls from repr_corner_states (the ongoing, consistent ones) in front, positions from play behind"""
    from oracle import oracle as orc

    corners, ok = posgen.repr_corner_states(orc, n)
    sts = np.concatenate([corners[ok][:40], posgen.distinct_positions(orc, n, 25, seed=90 + n)])
    assert len(sts) == 65
    sts.setflags(write=False)
    return sts


@functools.lru_cache(maxsize=None)
def _reference(kind, precision, mask):
    """the fold of all 65 states, once per (network, precision, mask): shared, never modified"""
    from oracle import oracle as orc

    n, _, _, head = NETS[kind]
    e = _engine(kind, precision)
    p, v = symm_ref.fold_batch(e.policy_eval, orc, n, orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV, _states(n),
                               symm_ref.perm_tables(n, head == "fc5"), mask)
    p.setflags(write=False)
    v.setflags(write=False)
    return p, v


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("kind", ["fc5", "conv6", "conv5"])
def test_device_tables_equal_the_test_built_ones(kind):
    n, _, _, head = NETS[kind]
    got = _engine(kind).symm_perm()
    want = symm_ref.perm_tables(n, head == "fc5")
    assert got.shape == want.shape and (got >= 0).all()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("kind", ["fc5", "conv6"])
@pytest.mark.parametrize("mask", MASKS)
def test_host_variant_equals_the_numpy_fold_bit_for_bit(kind, mask):
    n = NETS[kind][0]
    e, sts = _engine(kind), _states(n)
    want_p, want_v = _reference(kind, "f32", mask)
    for count in (1, 3, 65):  # 65 · k > max_batch for every k > 0: the slicer cuts inside the run (k = 1: 64 + 1)
        p, v = e.policy_eval(sts[:count], symmetries=mask)
        assert _same_bits(p, want_p[:count]), (count, int((p.view(np.uint32) != want_p[:count].view(np.uint32)).sum()))
        assert _same_bits(v, want_v[:count]), count
    if mask == 0x01:
        p0, v0 = e.policy_eval(sts)
        assert _same_bits(p, p0) and _same_bits(v, v0)
    if mask == 0xFF:
        # the gate has teeth on this data: the descending fold differs in bits (dividing first is bit-equal at k = 8, a power of two:
        # invisible by arithmetic, tests/test_symm_tables.py shows it at k = 3)
        from oracle import oracle as orc

        head = orc.HEAD_FC5 if kind == "fc5" else orc.HEAD_CONV
        wrong, _ = symm_ref.fold_batch(e.policy_eval, orc, n, head, sts[:8], symm_ref.perm_tables(n, kind == "fc5"), mask, order="descending")
        differs = int((wrong.view(np.uint32) != want_p[:8].view(np.uint32)).sum())
        print(f"symm-fold teeth on {kind}: descending fold differs in {differs} of {wrong.size} entries")
        assert differs > 0


@pytest.mark.parametrize("mask", MASKS)
def test_bf16x3_precision_equals_the_fold_of_its_own_policy_eval(mask):
    e, sts = _engine("fc5", "bf16x3"), _states(5)
    want_p, want_v = _reference("fc5", "bf16x3", mask)
    p, v = e.policy_eval(sts, symmetries=mask)
    assert _same_bits(p, want_p) and _same_bits(v, want_v)
    f32_p, _ = _reference("fc5", "f32", mask)
    assert not _same_bits(p, f32_p)  # (it is the other arithmetic that was folded)


@pytest.mark.parametrize("kind", ["fc5", "conv6"])
def test_rows_sum_to_one(kind):
    """Every output entry is k − 1 f32 adds of non-negative terms and one multiply by the rounded constant 1/k: at most k + 1 = 9
    roundings, a relative error ≤ 9 U = 4.5 ulp-of-1 steps on each entry and therefore on the row sum.  The rows that go in are
    tg_policy_eval's softmax rows, whose own sums are measured here on the reference side (they are not what is under test): they
    must leave 3.5 of the 8 steps."""
    n = NETS[kind][0]
    e, sts = _engine(kind), _states(n)
    from oracle import oracle as orc

    img = symm_ref.image_states(orc, n, orc.HEAD_FC5 if kind == "fc5" else orc.HEAD_CONV, sts)
    p_in, _ = e.policy_eval(img.reshape(-1, img.shape[-1]))
    d_in = np.abs(p_in.astype(np.float64).sum(1) - 1.0).max()
    p, _ = e.policy_eval(sts, symmetries=0xFF)
    d_out = np.abs(p.astype(np.float64).sum(1) - 1.0).max()
    print(f"symm row sums on {kind}: inputs deviate by {d_in / (2 * U):.2f} steps, ensemble rows by {d_out / (2 * U):.2f} steps (bound 8)")
    assert d_in <= 3.5 * 2 * U
    assert d_out <= 8 * 2 * U
    assert (p >= 0).all()


@pytest.mark.parametrize("kind", ["fc5", "conv6"])
def test_full_ensemble_is_equivariant(kind):
    """The images of t(x) are the images of x in another order (s ∘ t runs over the group with s), and the forward of a packed state
    does not depend on its row, so the two ensembles add the SAME eight f32 numbers per slot in two orders and multiply by 1/8
    exactly.  Bound as the specification states it: 8 · 2⁻²⁴ relative on each probability (one rounding per term of the sum; below
    the smallest normal number the f32 spacing 2⁻¹⁴⁹ replaces it) and the same absolute on the value (|v| ≤ 1)."""
    from oracle import oracle as orc

    n = NETS[kind][0]
    head = orc.HEAD_FC5 if kind == "fc5" else orc.HEAD_CONV
    e, sts = _engine(kind), _states(n)[:24]
    perm = symm_ref.perm_tables(n, kind == "fc5")
    base_p, base_v = e.policy_eval(sts, symmetries=0xFF)
    img = symm_ref.image_states(orc, n, head, sts)
    worst_p = worst_v = 0.0
    for t in (1, 2, 5, 7):
        p, v = e.policy_eval(img[:, t], symmetries=0xFF)
        back = p[:, perm[t]].astype(np.float64)  # slot j of x is slot perm[t][j] of t(x)
        a = base_p.astype(np.float64)
        err = np.abs(back - a) - 8 * 2.0 ** -149
        rel = (err / np.maximum(a, 2.0 ** -126)).max()
        worst_p, worst_v = max(worst_p, rel), max(worst_v, float(np.abs(v.astype(np.float64) - base_v).max()))
    print(f"symm equivariance on {kind}: worst relative policy difference {worst_p / U:.2f} U, worst value difference {worst_v / U:.2f} U (bound 8 U)")
    assert worst_p <= 8 * U
    assert worst_v <= 8 * U


@pytest.mark.parametrize("kind", ["fc5", "conv6"])
def test_dev_variant_equals_the_host_variant(kind):
    import torch

    import tak_amd

    n = NETS[kind][0]
    e, sts = _engine(kind), _states(n)
    for mask, count in ((0xFF, 8), (0x24, 32), (0x80, 64), (0x01, 64)):
        k = bin(mask).count("1")
        assert count * k <= MAX_BATCH
        d_states = torch.from_numpy(np.array(sts[:count])).cuda()
        d_policy = torch.zeros((count, e.psize), dtype=torch.float32, device="cuda")
        d_eval = torch.zeros(count, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        e.policy_eval_symm_dev(count, d_states.data_ptr(), mask, d_policy.data_ptr(), d_eval.data_ptr())
        e.sync()
        want_p, want_v = _reference(kind, "f32", mask)
        assert _same_bits(d_policy.cpu().numpy(), want_p[:count]) and _same_bits(d_eval.cpu().numpy(), want_v[:count]), hex(mask)
    # n · k > max_batch, a bad mask: argument errors, nothing launched
    for args in ((9, 0xFF), (1, 0), (1, 0x100)):
        with pytest.raises(tak_amd.TgError) as ei:
            e.policy_eval_symm_dev(args[0], d_states.data_ptr(), args[1], d_policy.data_ptr(), d_eval.data_ptr())
        assert ei.value.code == -1
    e.policy_eval_symm_dev(0, 0, 0xFF, 0, 0)  # n = 0: TG_OK


def test_outputs_do_not_depend_on_the_batch_and_errors_are_returned():
    import tak_amd

    e, sts = _engine("fc5"), _states(5)
    want_p, want_v = _reference("fc5", "f32", 0xFF)
    for lo, hi in ((7, 8), (3, 20), (60, 65)):  # other cuts, other neighbours: the same rows
        p, v = e.policy_eval(sts[lo:hi], symmetries=0xFF)
        assert _same_bits(p, want_p[lo:hi]) and _same_bits(v, want_v[lo:hi])
    p, v = e.policy_eval(sts[:0], symmetries=0xFF)
    assert p.shape == (0, e.psize) and v.shape == (0,)
    for mask in (0, 0x100, 0x1FF):
        with pytest.raises(tak_amd.TgError) as ei:
            e.policy_eval(sts[:2], symmetries=mask)
        assert ei.value.code == -1 and "mask" in str(ei.value)
    h = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=8)
    with pytest.raises(tak_amd.TgError) as ei:
        h.policy_eval(sts[:2], symmetries=0xFF)
    assert ei.value.code == -7  # TG_ERR_STATE: not a network engine
    h.close()
    raw = tak_amd.Engine(5, res_blocks=1, filters=32, evaluator=tak_amd.EVAL_RESNET, max_batch=8)
    with pytest.raises(tak_amd.TgError) as ei:
        raw.policy_eval(sts[:2], symmetries=0xFF)
    assert ei.value.code == -7  # TG_ERR_STATE: weights not finalized
    raw.close()
