"""tg_reanalyse in every layer — header, version script, library, ctypes binding, Rust binding, loop script — added beside what
was there: one more entry point, the window's seven untouched, the ABI version kept.  Needs no GPU."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

from abi_helpers import defined_symbols, parsed_header as _parsed_header, rust_fields, script as _script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "takgpu.h")
DECLARATION = [("TgEngine*", "e"), ("int", "first"), ("int", "count"), ("const TgReanalyseConfig*", "cfg"), ("TgReanalyseStats*", "out")]
CONFIG = [("rollouts", "int32_t", None), ("noise_alpha", "float", None), ("noise_ratio", "float", None), ("flags", "uint32_t", None),
          ("reserved", "int32_t", 4)]
STATS = [(f, "uint64_t", None) for f in ("rows", "updated", "mismatched", "unvisited", "expansions", "evals")]
WINDOW_SEVEN = ["tg_window_absorb", "tg_window_clear", "tg_window_create", "tg_window_info", "tg_window_push", "tg_window_read", "tg_window_train"]


def test_the_entry_point_is_declared_listed_and_exported_beside_the_windows_seven():
    import tak_amd

    functions = {name: (ret, args) for name, ret, args in _parsed_header()["functions"]}
    assert functions["tg_reanalyse"] == ("int", DECLARATION)
    assert sorted(n for n in functions if n.startswith("tg_reanalyse")) == ["tg_reanalyse"]
    assert sorted(n for n in functions if n.startswith("tg_window_")) == WINDOW_SEVEN
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "tak_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.search(r"global:(.*?)local:", script, flags=re.S).group(1).replace(";", " ").split()
    assert any(fnmatch.fnmatchcase("tg_reanalyse", p) for p in patterns), patterns
    defined = defined_symbols()
    assert "tg_reanalyse" in defined
    assert sorted(n for n in defined if n.startswith("tg_window_")) == WINDOW_SEVEN
    assert "tg_reanalyse" in tak_amd.engine.ABI_SYMBOLS
    assert sorted(n for n in tak_amd.engine.ABI_SYMBOLS if n.startswith("tg_window_")) == WINDOW_SEVEN


def test_the_header_comment_cites_the_reference_and_states_the_rules():
    text = open(HEADER).read()
    start = text.index("Reanalyse: refresh the policy targets")
    block = text[start:text.index("TG_API int tg_reanalyse(")]
    for needle in ("train/src/main.rs:82-95", "alpha-tak/src/search/play.rs:13-21", "TG_ERR_INVALID_ARG", "TG_ERR_STATE", "TG_ERR_ARENA_OVERFLOW",
                   "TG_ERR_LIMIT", "TG_ERR_NAN", "slot_base", "gamma_sample", "mismatched", "unvisited", "tg_search_set_symmetry", "tg_search_set_proof",
                   "self-play", "No counterpart"):
        assert needle in block, needle


def test_the_structures_have_the_same_layout_everywhere_and_the_abi_keeps_its_version(tmp_path):
    from tak_amd import engine

    structs = dict(_parsed_header()["structs"])
    assert structs["TgReanalyseConfig"] == CONFIG and structs["TgReanalyseStats"] == STATS
    offsets = [f"_Static_assert(offsetof(TgReanalyseConfig, {f}) == {o}, \"offset\");\n"
               for f, o in (("rollouts", 0), ("noise_alpha", 4), ("noise_ratio", 8), ("flags", 12), ("reserved", 16))]
    offsets += [f"_Static_assert(offsetof(TgReanalyseStats, {f}) == {8 * i}, \"offset\");\n" for i, (f, _, _) in enumerate(STATS)]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "takgpu.h"\n'
                   "_Static_assert(sizeof(TgReanalyseConfig) == 32, \"size\");\n"
                   "_Static_assert(sizeof(TgReanalyseStats) == 48, \"size\");\n"
                   "_Static_assert(sizeof(TgWindowInfo) == 32 && sizeof(TgSearchConfig) == 40, \"size\");\n"
                   "_Static_assert(TG_ABI_VERSION == 5, \"abi\");\n" + "".join(offsets))
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cfg, stats = engine.TgReanalyseConfig, engine.TgReanalyseStats
    assert [f for f, _ in cfg._fields_] == [f for f, _, _ in CONFIG]
    assert [t for _, t in cfg._fields_] == [C.c_int32, C.c_float, C.c_float, C.c_uint32, C.c_int32 * 4]
    assert [(f, t) for f, t in stats._fields_] == [(f, C.c_uint64) for f, _, _ in STATS]
    assert C.sizeof(cfg) == 32 and C.sizeof(stats) == 48 and engine.TG_ABI_VERSION == 5
    assert [getattr(cfg, f).offset for f, _, _ in CONFIG] == [0, 4, 8, 12, 16]
    rust = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    assert rust_fields("TgReanalyseConfig") == ["pub rollouts: i32", "pub noise_alpha: f32", "pub noise_ratio: f32", "pub flags: u32", "pub reserved: [i32; 4]"]
    assert rust_fields("TgReanalyseStats") == [f"pub {f}: u64" for f, _, _ in STATS]
    assert ("pub fn tg_reanalyse(e: *mut TgEngine, first: c_int, count: c_int, cfg: *const TgReanalyseConfig, out: *mut TgReanalyseStats) "
            "-> c_int;") in rust
    assert "pub const TG_ABI_VERSION: i32 = 5;" in rust
    safe = open(os.path.join(ROOT, "rust", "takgpu", "src", "reanalyse.rs")).read()
    assert "impl<const N: usize> GpuNet<N>" in safe and "sys::tg_reanalyse(" in safe
    assert re.search(r"pub fn reanalyse\(&mut self[,)]", safe)
    assert "pub mod reanalyse;" in open(os.path.join(ROOT, "rust", "takgpu", "src", "lib.rs")).read()


def test_the_python_wrapper_exists():
    from tak_amd import engine

    sig = inspect.signature(engine.Engine.reanalyse)
    assert list(sig.parameters)[1:] == ["first", "count", "rollouts", "noise_alpha", "noise_ratio"]
    assert sig.parameters["noise_alpha"].default == 0.0 and sig.parameters["noise_ratio"].default == 0.0
    assert sig.parameters["rollouts"].default is inspect.Parameter.empty


def test_a_null_engine_is_an_argument_error_with_a_message():
    import tak_amd

    lib = tak_amd.load_library()
    cfg, stats = tak_amd.engine.TgReanalyseConfig(8, 0.0, 0.0, 0), tak_amd.engine.TgReanalyseStats()
    assert lib.tg_reanalyse(C.c_void_p(None), 0, 0, C.byref(cfg), C.byref(stats)) == -1  # TG_ERR_INVALID_ARG
    message = lib.tg_last_error().decode()
    assert "null engine" in message and "tg_reanalyse" in message
    assert lib.tg_reanalyse(C.c_void_p(None), 0, 0, None, None) == -1


def test_the_loop_script_defaults_to_the_loop_as_it_was_and_needs_the_window():
    train_loop = _script("train_loop")
    args = train_loop.parse_args([])
    assert args.reanalyse_rows == 0 and args.reanalyse_rollouts == 0 and args.window == 0
    args = train_loop.parse_args(["--window", "4000", "--reanalyse-rows", "512", "--reanalyse-rollouts", "24"])
    assert (args.window, args.reanalyse_rows, args.reanalyse_rollouts) == (4000, 512, 24)
    for bad in (["--reanalyse-rows", "512"], ["--window", "4000", "--reanalyse-rows", "-1"], ["--window", "4000", "--reanalyse-rollouts", "-2"]):
        with pytest.raises(SystemExit) as ei:
            train_loop.parse_args(bad)
        assert ei.value.code == 2, bad
