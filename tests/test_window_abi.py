"""The example window's seven entry points and its structure in every layer — header, version script, library, ctypes binding, Rust
binding, loop script — without touching what was there: entry points are added only, so the ABI keeps its version.  Needs no GPU."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

from abi_helpers import defined_symbols, parsed_header as _parsed_header, rust_fields, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "takgpu.h")
DECLARATIONS = {
    "tg_window_create": [("TgEngine*", "e"), ("int", "capacity")],
    "tg_window_info": [("TgEngine*", "e"), ("TgWindowInfo*", "out")],
    "tg_window_clear": [("TgEngine*", "e")],
    "tg_window_absorb": [("TgEngine*", "e"), ("int32_t*", "n_absorbed")],
    "tg_window_push": [("TgEngine*", "e"), ("int", "n"), ("const void*", "states"), ("const int32_t*", "n_moves"), ("const TgMove*", "moves"),
                       ("const uint32_t*", "visits"), ("const float*", "results"), ("const int32_t*", "game_ids")],
    "tg_window_read": [("TgEngine*", "e"), ("int", "first"), ("int", "n"), ("TgExampleHeader*", "headers"), ("void*", "states"),
                       ("TgMove*", "moves"), ("uint32_t*", "visits")],
    "tg_window_train": [("TgEngine*", "e"), ("int", "first"), ("int", "count"), ("uint64_t", "seed"), ("float*", "mean_loss_p"),
                        ("float*", "mean_loss_z"), ("int32_t*", "steps")],
}
WRAPPERS = ("window_create", "window_info", "window_clear", "window_absorb", "window_push", "window_read", "window_train")


def test_the_seven_entry_points_are_declared_listed_and_exported():
    import tak_amd

    functions = {name: (ret, args) for name, ret, args in _parsed_header()["functions"]}
    for name, args in DECLARATIONS.items():
        assert functions[name] == ("int", args), name
    assert sorted(n for n in functions if n.startswith("tg_window_")) == sorted(DECLARATIONS)
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "tak_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.search(r"global:(.*?)local:", script, flags=re.S).group(1).replace(";", " ").split()
    defined = defined_symbols()
    for name in DECLARATIONS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in defined, name
        assert name in tak_amd.engine.ABI_SYMBOLS


def test_the_header_comments_cite_the_reference_and_state_the_errors():
    text = open(HEADER).read()
    for name in DECLARATIONS:
        comment = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*TG_API int " + name + r"\(", text, flags=re.S)
        assert len(comment) == 1, name
        assert re.search(r"(main|network)\.rs:\d+", comment[0]), name
    block = text[text.index("Example window (the `examples` of training_loop"):text.index("TG_API int tg_window_create")]
    assert "train/src/main.rs:26,56-123" in block and "TG_ERR_STATE" in block and "TG_ERR_INVALID_ARG" in block and "TG_ERR_NO_DEVICE" in block
    train = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*TG_API int tg_window_train\(", text, flags=re.S).group(1)
    assert "same number of chunks" in train and "bit for" in train and "TG_ERR_STATE" in train and "TG_ERR_INVALID_ARG" in train
    create = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*TG_API int tg_window_create\(", text, flags=re.S).group(1)
    assert "TG_ERR_HIP" in create and "tg_pit" in create and "size_t" in create


def test_the_structure_is_the_same_32_bytes_everywhere_and_the_abi_keeps_its_version(tmp_path):
    from tak_amd import engine

    structs = dict(_parsed_header()["structs"])
    assert structs["TgWindowInfo"] == [(f, "uint64_t", None) for f in ("capacity", "count", "entered", "evicted")]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "takgpu.h"\n'
                   "_Static_assert(sizeof(TgWindowInfo) == 32, \"size\");\n"
                   "_Static_assert(offsetof(TgWindowInfo, capacity) == 0, \"offset\");\n"
                   "_Static_assert(offsetof(TgWindowInfo, count) == 8, \"offset\");\n"
                   "_Static_assert(offsetof(TgWindowInfo, entered) == 16, \"offset\");\n"
                   "_Static_assert(offsetof(TgWindowInfo, evicted) == 24, \"offset\");\n"
                   "_Static_assert(sizeof(TgSelfPlayConfig) == 40 && sizeof(TgExampleHeader) == 16, \"size\");\n"
                   "_Static_assert(TG_ABI_VERSION == 5, \"abi\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    S = engine.TgWindowInfo
    assert [(f, t) for f, t in S._fields_] == [(f, C.c_uint64) for f in ("capacity", "count", "entered", "evicted")]
    assert C.sizeof(S) == 32 and engine.TG_ABI_VERSION == 5
    rust = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    assert rust_fields("TgWindowInfo") == [f"pub {f}: u64" for f in ("capacity", "count", "entered", "evicted")]
    assert "pub fn tg_window_absorb(e: *mut TgEngine, n_absorbed: *mut i32) -> c_int;" in rust
    assert ("pub fn tg_window_train(e: *mut TgEngine, first: c_int, count: c_int, seed: u64, mean_loss_p: *mut f32, mean_loss_z: *mut f32, "
            "steps: *mut i32) -> c_int;") in rust
    safe = "".join(open(os.path.join(ROOT, "rust", "takgpu", "src", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "rust", "takgpu", "src"))))
    for name in DECLARATIONS:
        assert f"sys::{name}(" in safe, name
    window = open(os.path.join(ROOT, "rust", "takgpu", "src", "window.rs")).read()
    assert "impl<const N: usize> GpuNet<N>" in window and "impl Drop" not in window and "Drop for" not in window  # the engine owns its window
    for method, receiver in [("window_create", "&mut self"), ("window_absorb", "&mut self"), ("window_push", "&mut self"),
                             ("window_train", "&mut self"), ("window_clear", "&mut self"), ("window_info", "&self"), ("window_read", "&self")]:
        assert re.search(r"pub fn " + method + r"\(" + receiver + r"[,)]", window), method
    assert "self.trainer_handle()?" in window  # window_train creates the trainer on first use, as try_train does


def test_the_python_wrappers_exist():
    from tak_amd import engine

    for name in WRAPPERS:
        assert callable(getattr(engine.Engine, name)), name
    assert list(inspect.signature(engine.Engine.window_push).parameters)[1:] == ["states", "n_moves", "moves", "visits", "results", "game_ids"]
    assert inspect.signature(engine.Engine.window_push).parameters["game_ids"].default is None
    assert list(inspect.signature(engine.Engine.window_train).parameters)[1:] == ["first", "count", "seed"]
    sig = inspect.signature(engine.Engine.write_examples)
    assert sig.parameters["window"].default is None and sig.parameters["cap"].default == 1 << 16  # the drain path is the default


def test_every_entry_point_fails_loudly_without_a_device_or_an_engine():
    """An engine exists only where a device does — without one tg_engine_create answers TG_ERR_NO_DEVICE and there is nothing to
    hand to tg_window_* — and a null engine is an argument error with a message, never a crash or a silent success."""
    import torch

    import tak_amd

    lib = tak_amd.load_library()
    if not torch.cuda.is_available():
        with pytest.raises(tak_amd.TgError) as ei:
            tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH)
        assert ei.value.code == -2 and "no HIP device" in str(ei.value)
    info, k, f = tak_amd.engine.TgWindowInfo(), C.c_int32(0), C.c_float(0)
    null = C.c_void_p(None)
    calls = {
        "tg_window_create": (null, 16),
        "tg_window_info": (null, C.byref(info)),
        "tg_window_clear": (null,),
        "tg_window_absorb": (null, C.byref(k)),
        "tg_window_push": (null, 0, None, None, None, None, None, None),
        "tg_window_read": (null, 0, 0, None, None, None, None),
        "tg_window_train": (null, 0, 0, C.c_uint64(0), C.byref(f), C.byref(f), C.byref(k)),
    }
    assert sorted(calls) == sorted(DECLARATIONS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name  # TG_ERR_INVALID_ARG
        assert "null engine" in lib.tg_last_error().decode() and name in lib.tg_last_error().decode(), name


def test_the_loop_script_takes_the_window_and_defaults_to_the_loop_as_it_was():
    train_loop = script("train_loop")
    assert train_loop.parse_args([]).window == 0
    assert train_loop.parse_args(["--window", "4000"]).window == 4000
    with pytest.raises(SystemExit) as ei:
        train_loop.parse_args(["--window", "-1"])
    assert ei.value.code == 2
