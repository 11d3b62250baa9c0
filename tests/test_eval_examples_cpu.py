"""tg_eval_examples without a GPU: the ABI carries the entry point through every surface, the fp64 reference the GPU test gates
against passes its own gates when it is run in f32 (the bounds are not vacuous and not out of f32's reach), and the training loop's
--holdout 0 is the loop as it was.

PyTorch f32 against fp64 on the GPU test's own rows (the 65 examples without symmetries, the first 23 with; seed 5), worst |Δ|:
                    loss_p     loss_z     v
  net5_fc_2x32      3.8e-07    9.0e-08    4.3e-08
  net5_fc_1x64      3.8e-07    9.5e-08    4.9e-08
  net6_conv_1x32    7.5e-07    1.3e-07    5.7e-08
  net4_conv_1x32    4.2e-07    5.2e-08    2.8e-08
so every bound is its floor (tests/eval_examples_ref.py: 2e-5, 8e-6, 2e-6)."""
import fnmatch
import importlib.util
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import eval_examples_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ["net5_fc_2x32", "net5_fc_1x64", "net6_conv_1x32", "net4_conv_1x32"]
SEED = 5


def test_header_declares_the_entry_point_and_the_struct():
    text = open(os.path.join(ROOT, "include", "takgpu.h")).read()
    m = re.search(r"typedef struct TgExampleMetrics \{(.*?)\} TgExampleMetrics;", text, re.S)
    assert m, "struct TgExampleMetrics is missing"
    fields = re.findall(r"^\s*(double|uint64_t)\s+(\w+);", m.group(1), re.M)
    assert fields == [("double", "loss_p"), ("double", "loss_z"), ("double", "target_entropy"), ("uint64_t", "top1"),
                      ("uint64_t", "sign_ok"), ("uint64_t", "decided"), ("uint64_t", "positions")]
    d = re.search(r"TG_API int tg_eval_examples\((.*?)\);", text, re.S)
    assert d, "tg_eval_examples is not declared"
    params = re.sub(r"/\*.*?\*/", "", d.group(1), flags=re.S)
    assert [p.split()[-1].lstrip("*") for p in params.split(",")] == ["e", "n", "states", "n_moves", "moves", "visits", "results",
                                                                       "symmetries", "sums", "rows"]
    assert "#define TG_ABI_VERSION 5" in text  # one added entry point, the version stays


def test_library_exports_the_entry_point():
    import tak_amd

    text = open(os.path.join(ROOT, "tak_amd", "csrc", "exports.map")).read()
    globs = re.search(r"global:(.*?);", text, re.S).group(1).split()
    assert any(fnmatch.fnmatchcase("tg_eval_examples", g) for g in globs), "exports.map does not list tg_eval_examples"
    out = subprocess.run(["nm", "-D", "--defined-only", tak_amd.LIB_PATH], check=True, stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r" T tg_eval_examples$", out, re.M), "libtakgpu.so does not export tg_eval_examples"
    assert "tg_eval_examples" in tak_amd.engine.ABI_SYMBOLS


def test_rust_binding_carries_it():
    sys_rs = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    assert re.search(r"pub fn tg_eval_examples\(e: \*mut TgEngine, n: c_int, .*sums: \*mut TgExampleMetrics, rows: \*mut f32\) -> c_int;", sys_rs)
    assert re.search(r"pub struct TgExampleMetrics \{\s*pub loss_p: f64,\s*pub loss_z: f64,\s*pub target_entropy: f64,\s*pub top1: u64,", sys_rs)
    safe = open(os.path.join(ROOT, "rust", "takgpu", "src", "net.rs")).read()
    assert "pub fn evaluate_examples" in safe and "sys::tg_eval_examples" in safe


@pytest.mark.parametrize("name", NETS)
def test_reference_in_f32_passes_its_own_gates(orc, name):
    """the fp64 helper run in f32 stays inside the floors with room to spare (so 3 × its distance never lifts a bound above its
    floor here), its top-1 and sign agree with fp64 on every row whose margin clears 1e-4, and at most 5 % of the rows are left out
    — on the fp64 reference alone, which is what fixes the seed"""
    net, n, _, _, head = ref.golden_net(name)
    ex = ref.make_examples(orc, n, 65, SEED)
    worst = {k: 0.0 for k in ref.FLOORS}
    for sub, symm in ((ex, False), (ref.take(ex, slice(0, 23)), True)):
        r64 = ref.reference_rows(orc, net, n, head, sub, symm)
        r32 = ref.reference_rows(orc, net, n, head, sub, symm, dtype=torch.float32)
        d = ref.distances(r32, r64)
        worst = {k: max(worst[k], d[k]) for k in worst}
        top_ok, sign_ok = ref.clear_rows(r64)
        assert (~top_ok).mean() <= ref.MAX_LEFT_OUT and (~sign_ok).mean() <= ref.MAX_LEFT_OUT
        assert np.array_equal(r32["top1"][top_ok], r64["top1"][top_ok])
        assert np.array_equal(np.sign(r32["v"][sign_ok]), np.sign(r64["v"][sign_ok]))
        # the forced cases are in the sample: one-hot (entropy 0), the all-ones tie, both results and a draw
        assert r64["entropy"][0] == 0.0 and set(np.unique(r64["z"])) == {-1.0, 0.0, 1.0}
        c1 = int(sub["n_moves"][1])
        assert abs(r64["entropy"][8 if symm else 1] - np.log(c1)) < 1e-12
    print(f"f32 against fp64, {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    b = ref.bounds(worst)
    assert all(worst[k] <= b[k] for k in worst)
    assert all(3.0 * worst[k] <= ref.FLOORS[k] for k in worst), "the floors no longer sit above 3 × f32's own distance: re-derive them"


def test_move_transform_is_the_oracles(orc):
    """positions() checks the python move transform against oracle.augment's dense targets for every image; longest list included"""
    ex = ref.make_examples(orc, 6, 8, SEED)
    assert ex["n_moves"][3] == ex["n_moves"].max() and ex["n_moves"][2] == ex["n_moves"].min()
    states8, idx, owner = ref.positions(orc, 6, "conv", ex, True)
    assert states8.shape[0] == 64 and idx.min() >= 0 and list(owner[:9]) == [0] * 8 + [1]


def _train_loop():
    spec = importlib.util.spec_from_file_location("train_loop", os.path.join(ROOT, "scripts", "train_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_loop_holdout_zero_is_todays_loop():
    tl = _train_loop()
    a = tl.parse_args([])
    assert a.holdout == 0.0 and int(round(a.holdout * a.examples)) == 0
    assert vars(tl.parse_args(["--holdout", "0"])) == vars(a)
    keep, held = tl.holdout_split(10, 0, [0, 0])
    assert list(keep) == list(range(10)) and len(held) == 0
    keep, held = tl.holdout_split(100, 20, [3, 1])
    assert len(held) == 20 and len(keep) == 80 and sorted(set(keep) | set(held)) == list(range(100))
    assert np.array_equal(held, tl.holdout_split(100, 20, [3, 1])[1]) and not np.array_equal(held, tl.holdout_split(100, 20, [3, 2])[1])
    with pytest.raises(SystemExit):
        tl.parse_args(["--holdout", "1.5"])


def test_rank_sums_add():
    from tak_amd import dist, engine

    s = {"loss_p": 3.0, "loss_z": 1.0, "target_entropy": 1.0, "top1": 2, "sign_ok": 1, "decided": 2, "positions": 4}
    assert dist.reduce_example_sums(None, s) == s
    m = engine.example_means(s)
    assert m == {"loss_p": 0.75, "loss_z": 0.25, "kl": 0.5, "top1": 0.5, "value_sign": 0.5}
    assert np.isnan(engine.example_means({**s, "decided": 0, "sign_ok": 0})["value_sign"])
