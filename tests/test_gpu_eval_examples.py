"""tg_eval_examples on the GPU: the losses of the deployed (folded-BatchNorm, running statistics) network on examples, against the
fp64 reference of tests/eval_examples_ref.py — PyTorch on the CPU, eval mode, log_softmax over all P outputs, π from the visits at
oracle.move_index, images from oracle.augment.

Row gate (loss_p, loss_z, v per row): the larger of a floor and 3 × PyTorch f32's own worst distance to fp64 on the same rows.
Measured on the CPU before any GPU run (tests/test_eval_examples_cpu.py prints them): f32 is within 7.5e-7 / 1.3e-7 / 5.7e-8 of fp64
on all four networks, so every bound is its floor: 2e-5 / 8e-6 / 2e-6 (derived in eval_examples_ref.py from the f32 format).
The engine's measured distances are recorded in profiles/r12_a_eval_examples_fp64_distance.txt.
Top-1 and sign are compared on rows whose fp64 margin clears 1e-4; at most 5 % of the rows may be left out (asserted; seed 5 was
chosen on the CPU so that the reference alone satisfies it)."""
import numpy as np
import pytest

import eval_examples_ref as ref

pytestmark = pytest.mark.gpu

SEED = 5
NETS = ["net5_fc_2x32", "net5_fc_1x64", "net6_conv_1x32", "net4_conv_1x32"]
TG_ERR_INVALID_ARG, TG_ERR_STATE = -1, -7
_cache = {}


def _setup(orc, name):
    """(net, n, blocks, filters, head, the 65 examples, fp64 rows without symmetries, fp64 rows of the first 23 with) — computed once"""
    if name not in _cache:
        net, n, blocks, filters, head = ref.golden_net(name)
        ex = ref.make_examples(orc, n, 65, SEED)
        r_plain = ref.reference_rows(orc, net, n, head, ex, False)
        r_symm = ref.reference_rows(orc, net, n, head, ref.take(ex, slice(0, 23)), True)
        _cache[name] = (net, n, blocks, filters, head, ex, r_plain, r_symm)
    return _cache[name]


def _engine(orc, name, max_batch=64, precision="f32", evaluator=None, load=True):
    import tak_amd
    import torch_ref

    net, n, blocks, filters, head = _setup(orc, name)[:5]
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV,
                       evaluator=tak_amd.EVAL_RESNET if evaluator is None else evaluator, max_batch=max_batch)
    if precision != "f32":
        e.set_precision(precision)
    if load:
        e.load_state_dict(torch_ref.abi_tensors(net))
    return e


def _check_rows(what, out, r64, k):
    """the value gate, the top-1 / sign comparison and the sums of one call over the first k positions of the reference"""
    rows, sums = out["rows"], out["sums"]
    r = {key: v[:k] for key, v in r64.items()}
    assert rows.shape == (k, 4) and np.isfinite(rows).all()
    d = ref.distances(rows, r)
    print(f"{what}: engine against fp64  " + "  ".join(f"{key} {v:.2e}" for key, v in d.items()))
    for key, bound in ref.FLOORS.items():  # (= ref.bounds(f32's distances): every 3 × distance is below its floor, see the docstring)
        assert d[key] <= bound, f"{what}: {key} is {d[key]:.3e} from fp64, bound {bound:.1e}"
    top_ok, sign_ok = ref.clear_rows(r)
    assert (~top_ok).mean() <= ref.MAX_LEFT_OUT and (~sign_ok).mean() <= ref.MAX_LEFT_OUT
    assert set(np.unique(rows[:, 2])) <= {0.0, 1.0}
    assert np.array_equal(rows[top_ok, 2], r["top1"][top_ok]), f"{what}: top-1 differs from fp64 on a row with a clear margin"
    assert np.array_equal(np.sign(rows[sign_ok, 3]), np.sign(r["v"][sign_ok]))
    # sums: the f64 sum of the returned rows in order, bit for bit; the counts exact
    lp, lz = ref.f64_sums(rows)
    assert sums["loss_p"] == lp and sums["loss_z"] == lz
    assert abs(sums["target_entropy"] - r["entropy"].sum()) <= 1e-5 * max(1.0, r["entropy"].sum())
    z, v = r["z"], rows[:, 3].astype(np.float64)
    assert sums["positions"] == k and sums["decided"] == int((z != 0).sum())
    assert sums["top1"] == int(rows[:, 2].sum()) and sums["sign_ok"] == int(((z != 0) & (v * z > 0)).sum())
    assert out["loss_p"] == lp / k and out["kl"] == (sums["loss_p"] - sums["target_entropy"]) / k
    return d


@pytest.mark.parametrize("name", NETS)
def test_rows_against_fp64(orc, name):
    """n = 1, 8, 9, 23 with symmetries (8·23 = 184 positions = three slices of max_batch 64, the last one ragged) and n = 65
    without (two slices); one-hot, tied, shortest and longest move lists are examples 0 … 3"""
    _, n, _, _, head, ex, r_plain, r_symm = _setup(orc, name)
    e = _engine(orc, name)
    worst = {}
    for k in (1, 8, 9, 23):
        out = e.evaluate_examples(*ref.args(ref.take(ex, slice(0, k))), symmetries=True, rows=True)
        d = _check_rows(f"{name} n={k} symmetries", out, r_symm, 8 * k)
        worst = {key: max(worst.get(key, 0.0), v) for key, v in d.items()}
    out = e.evaluate_examples(*ref.args(ex), rows=True)
    d = _check_rows(f"{name} n=65", out, r_plain, 65)
    worst = {key: max(worst.get(key, 0.0), v) for key, v in d.items()}
    print(f"{name}: worst engine distance to fp64  " + "  ".join(f"{key} {v:.2e}" for key, v in worst.items()))
    # without rows the sums are the same bits
    assert e.evaluate_examples(*ref.args(ex))["sums"] == out["sums"]
    e.close()


@pytest.mark.parametrize("name", ["net5_fc_2x32", "net6_conv_1x32"])
def test_determinism_over_max_batch_and_call_splits(orc, name):
    ex = ref.take(_setup(orc, name)[5], slice(0, 23))
    ints = ("top1", "sign_ok", "decided", "positions")
    outs = []
    for mb in (64, 256):
        e = _engine(orc, name, max_batch=mb)
        for symm in (False, True):
            one = e.evaluate_examples(*ref.args(ex), symmetries=symm, rows=True)
            a = e.evaluate_examples(*ref.args(ref.take(ex, slice(0, 10))), symmetries=symm, rows=True)
            b = e.evaluate_examples(*ref.args(ref.take(ex, slice(10, 23))), symmetries=symm, rows=True)
            both = np.concatenate([a["rows"], b["rows"]])
            assert np.array_equal(one["rows"].view(np.uint32), both.view(np.uint32)), f"{name} max_batch {mb}: rows depend on the call split"
            assert all(one["sums"][k] == a["sums"][k] + b["sums"][k] for k in ints)
            outs.append((symm, one))
        e.close()
    for (s0, o0), (s1, o1) in zip(outs[:2], outs[2:]):
        assert s0 == s1 and np.array_equal(o0["rows"].view(np.uint32), o1["rows"].view(np.uint32)), f"{name}: rows depend on max_batch"
        assert o0["sums"] == o1["sums"], f"{name}: the one-call sums depend on max_batch"


def test_symmetry_bookkeeping(orc):
    import tak_amd

    name = "net5_fc_2x32"
    ex = ref.take(_setup(orc, name)[5], slice(0, 23))
    h = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=64)
    with pytest.raises(tak_amd.TgError) as err:  # the hash evaluator has no network to evaluate
        h.evaluate_examples(*ref.args(ex))
    assert err.value.code == TG_ERR_STATE
    h.close()
    e = _engine(orc, name)
    plain = e.evaluate_examples(*ref.args(ex), rows=True)
    symm = e.evaluate_examples(*ref.args(ex), symmetries=True, rows=True)
    assert np.array_equal(symm["rows"][0::8].view(np.uint32), plain["rows"].view(np.uint32)), "image 0 is not the example itself"
    assert symm["sums"]["positions"] == 8 * 23 and symm["sums"]["decided"] == 8 * plain["sums"]["decided"]
    # loss_z's target and the target entropy are the example's, whatever the image: per example through single-example calls
    for i in (0, 1, 3, 7):
        one = ref.take(ex, slice(i, i + 1))
        p1 = e.evaluate_examples(*ref.args(one))["sums"]
        s1 = e.evaluate_examples(*ref.args(one), symmetries=True, rows=True)
        acc = 0.0
        for _ in range(8):
            acc += p1["target_entropy"]
        assert s1["sums"]["target_entropy"] == acc and s1["sums"]["decided"] == 8 * p1["decided"]
        z = float(ex["results"][i])
        v = s1["rows"][:, 3]
        assert np.array_equal(s1["rows"][:, 1], (np.float32(z) - v) * (np.float32(z) - v))
    e.close()


def test_search_is_left_alone(orc):
    name = "net5_fc_2x32"
    ex = ref.take(_setup(orc, name)[5], slice(0, 23))
    e = _engine(orc, name)
    roots = ex["states"][4:7]
    e.search_create(3, arena_nodes=1 << 12, batch=4)
    e.search_reset(roots)
    e.search_run(12)
    want = [e.search_dump(g) for g in range(3)]
    e.search_reset(roots)
    e.search_run(6)
    counters = e.search_counters()
    a = e.evaluate_examples(*ref.args(ex), symmetries=True)
    assert e.search_counters() == counters
    e.search_run(6)
    for g in range(3):
        got = e.search_dump(g)
        assert len(got) == len(want[g]) and all(np.array_equal(got[f], want[g][f]) for f in got.dtype.names), f"tree {g} differs"
    assert e.evaluate_examples(*ref.args(ex), symmetries=True)["sums"] == a["sums"]
    e.close()


def test_trainer_is_left_alone_and_the_installed_network_is_read(orc):
    import torch_ref

    name = "net5_fc_2x32"
    net, _, _, _, _, ex, _, _ = _setup(orc, name)
    ex8 = ref.take(ex, slice(0, 8))
    e = _engine(orc, name)
    e.train_create(chunk_size=8, chunks_in_step=1)
    shapes = {k: v.shape for k, v in torch_ref.abi_tensors(net).items()}
    before = {k: e.train_get_tensor(k, s) for k, s in shapes.items()}
    first = e.evaluate_examples(*ref.args(ex8), symmetries=True, rows=True)
    for k, s in shapes.items():
        assert np.array_equal(e.train_get_tensor(k, s).view(np.uint32), before[k].view(np.uint32)), f"{k} changed"
    lp, lz, stepped = e.train_chunk(*ref.args(ex8))
    assert stepped
    # not yet committed: still the installed network
    assert np.array_equal(e.evaluate_examples(*ref.args(ex8), symmetries=True, rows=True)["rows"], first["rows"])
    e.train_commit()
    after = e.evaluate_examples(*ref.args(ex8), symmetries=True, rows=True)
    assert not np.array_equal(after["rows"][:, 0], first["rows"][:, 0]) and not np.array_equal(after["rows"][:, 3], first["rows"][:, 3])
    e.close()


def test_split_bf16(orc):
    """TG_OK, finite rows and the f32 call's top-1 on the rows with a clear fp64 margin; no value gate is claimed for this path"""
    name = "net5_fc_1x64"
    ex, r_symm = _setup(orc, name)[5], _setup(orc, name)[7]
    ex = ref.take(ex, slice(0, 23))
    f = _engine(orc, name)
    want = f.evaluate_examples(*ref.args(ex), symmetries=True, rows=True)["rows"]
    f.close()
    e = _engine(orc, name, precision="bf16x3")
    out = e.evaluate_examples(*ref.args(ex), symmetries=True, rows=True)
    e.close()
    assert np.isfinite(out["rows"]).all() and out["sums"]["positions"] == 184
    top_ok, _ = ref.clear_rows(r_symm)
    assert np.array_equal(out["rows"][top_ok, 2], want[top_ok, 2])
    print("net5_fc_1x64 bf16x3 against fp64 (not gated)  " + "  ".join(f"{k} {v:.2e}" for k, v in ref.distances(out["rows"], r_symm).items()))


def test_errors(orc):
    import tak_amd

    name = "net5_fc_2x32"
    ex = ref.take(_setup(orc, name)[5], slice(0, 9))
    e = _engine(orc, name)

    def refused(code, **changes):
        bad = {k: v.copy() for k, v in ex.items()}
        symm = changes.pop("symmetries", False)
        for k, f in changes.items():
            f(bad[k])
        with pytest.raises(tak_amd.TgError) as err:
            e.evaluate_examples(*ref.args(bad), symmetries=symm)
        assert err.value.code == code, str(err.value)
        return str(err.value)

    def corrupt(states):
        states[5, 0:8] = 0xFF  # colour bits far above any stack height

    def no_moves(n_moves):
        n_moves[6] = 0

    def no_visits(visits):
        visits[7, :] = 0

    assert "example 5" in refused(TG_ERR_INVALID_ARG, states=corrupt)
    assert "example 6" in refused(TG_ERR_INVALID_ARG, n_moves=no_moves)
    assert "example 7" in refused(TG_ERR_INVALID_ARG, visits=no_visits)
    refused(TG_ERR_INVALID_ARG, symmetries=2)
    none = e.evaluate_examples(*ref.args(ref.take(ex, slice(0, 0))), symmetries=True, rows=True)
    assert none["rows"].shape == (0, 4) and all(v == 0 for v in none["sums"].values())
    e.close()
    for eng in (_engine(orc, name, evaluator=tak_amd.EVAL_DUMMY, load=False), _engine(orc, name, load=False)):  # dummy; resnet without weights
        with pytest.raises(tak_amd.TgError) as err:
            eng.evaluate_examples(*ref.args(ex))
        assert err.value.code == TG_ERR_STATE
        eng.close()
