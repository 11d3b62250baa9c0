"""The symmetry entry points in every layer — header, version script, library, ctypes binding, Rust sys binding — added without touching
what was there: structures keep their sizes and the ABI its version.  Needs no GPU."""
import ctypes as C
import fnmatch
import inspect
import os
import re
import subprocess

import pytest

from abi_helpers import defined_symbols, parsed_header as _parsed_header, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "takgpu.h")
DECLARATIONS = {
    "tg_policy_eval_symm": [("TgEngine*", "e"), ("int", "n"), ("const void*", "states"), ("uint32_t", "mask"), ("float*", "policy"),
                            ("float*", "eval")],
    "tg_policy_eval_symm_dev": [("TgEngine*", "e"), ("int", "n"), ("const void*", "d_states"), ("uint32_t", "mask"), ("float*", "d_policy"),
                                ("float*", "d_eval")],
    "tg_symm_perm_read": [("TgEngine*", "e"), ("int32_t*", "perm")],
    "tg_search_set_symmetry": [("TgEngine*", "e"), ("int", "mode")],
    "tg_search_get_symmetry": [("TgEngine*", "e"), ("int*", "mode"), ("uint64_t*", "leaves_transformed")],
}


def test_the_entry_points_are_declared_listed_and_exported():
    import tak_amd

    functions = {name: (ret, args) for name, ret, args in _parsed_header()["functions"]}
    for name, args in DECLARATIONS.items():
        assert functions[name] == ("int", args), name
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "tak_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.search(r"global:(.*?)local:", script, flags=re.S).group(1).replace(";", " ").split()
    defined = defined_symbols()
    for name in DECLARATIONS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in defined, name
        assert name in tak_amd.engine.ABI_SYMBOLS


def test_the_header_says_there_is_no_counterpart_and_states_the_fold_order():
    text = open(HEADER).read()
    for name in ("tg_policy_eval_symm", "tg_symm_perm_read", "tg_search_set_symmetry"):
        comment = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*(?:typedef enum TgSearchSymmetry[^\n]*\n)?TG_API int " + name + r"\(", text, flags=re.S)
        assert len(comment) == 1, name
        assert "No counterpart in the reference" in comment[0] and re.search(r"symm\.rs:\d+", comment[0]), name
    fold = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*TG_API int tg_policy_eval_symm\(", text, flags=re.S).group(1)
    for phrase in ("ASCENDING s", "first selected image", "comes last", "1.0f / (float)k", "TG_ERR_INVALID_ARG", "TG_ERR_STATE", "bit for bit"):
        assert phrase in fold, phrase
    mode = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef enum TgSearchSymmetry", text, flags=re.S).group(1)
    for phrase in ("0x73796d6d", "& 7", "tg_pit", "TG_SYMM_OFF", "TG_ERR_STATE", "TG_ERR_INVALID_ARG"):
        assert phrase in mode, phrase
    assert "typedef enum TgSearchSymmetry { TG_SYMM_OFF = 0, TG_SYMM_HASHED = 1 } TgSearchSymmetry;" in text


def test_structures_keep_their_sizes_and_the_abi_its_version(tmp_path):
    from tak_amd import engine

    src = tmp_path / "layout.c"
    src.write_text('#include "takgpu.h"\n'
                   "_Static_assert(sizeof(TgSearchConfig) == 40 && sizeof(TgSelfPlayConfig) == 40, \"size\");\n"
                   "_Static_assert(sizeof(TgPitConfig) == 40, \"size\");\n"
                   "_Static_assert(TG_SYMM_OFF == 0 && TG_SYMM_HASHED == 1, \"enum\");\n"
                   "_Static_assert(TG_ABI_VERSION == 5, \"abi\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert engine.TG_ABI_VERSION == 5 and C.sizeof(engine.TgSearchConfig) == 40 and C.sizeof(engine.TgPitConfig) == 40
    assert (engine.SYMM_OFF, engine.SYMM_HASHED) == (0, 1)
    fields = dict(_parsed_header()["structs"])
    assert "symmetry" not in " ".join(f for f, _, _ in fields["TgPitConfig"] + fields["TgSearchConfig"])


def test_the_rust_sys_binding_agrees_with_the_header():
    rust = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    for line in (
        "pub fn tg_policy_eval_symm(e: *mut TgEngine, n: c_int, states: *const c_void, mask: u32, policy: *mut f32, eval: *mut f32) -> c_int;",
        "pub fn tg_policy_eval_symm_dev(e: *mut TgEngine, n: c_int, d_states: *const c_void, mask: u32, d_policy: *mut f32, d_eval: *mut f32) -> c_int;",
        "pub fn tg_symm_perm_read(e: *mut TgEngine, perm: *mut i32) -> c_int;",
        "pub fn tg_search_set_symmetry(e: *mut TgEngine, mode: c_int) -> c_int;",
        "pub fn tg_search_get_symmetry(e: *mut TgEngine, mode: *mut c_int, leaves_transformed: *mut u64) -> c_int;",
        "pub const TG_SYMM_OFF: TgSearchSymmetry = 0;",
        "pub const TG_SYMM_HASHED: TgSearchSymmetry = 1;",
    ):
        assert line in rust, line
    safe = "".join(open(os.path.join(ROOT, "rust", "takgpu", "src", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "rust", "takgpu", "src"))))
    for name in ("tg_policy_eval_symm", "tg_search_set_symmetry"):
        assert f"sys::{name}(" in safe, name
    assert re.search(r"pub fn policy_eval_symm\(&self", safe) and re.search(r"pub symmetry: ", safe)


def test_the_python_wrappers_exist_and_default_to_off():
    import tak_amd
    from tak_amd import analysis, engine, player

    E = engine.Engine
    assert inspect.signature(E.policy_eval).parameters["symmetries"].default is None
    for f in (E.search_create, E.selfplay_create, engine.pit, player.Player.__init__):
        assert inspect.signature(f).parameters["symmetry"].default is None, f
    for name in ("search_set_symmetry", "search_get_symmetry", "policy_eval_symm_dev", "symm_perm"):
        assert callable(getattr(E, name)), name
    assert engine._symmetry_mode("hashed") == tak_amd.SYMM_HASHED and engine._symmetry_mode("off") == tak_amd.SYMM_OFF
    with pytest.raises(ValueError):
        engine._symmetry_mode("random")
    assert inspect.signature(analysis.root_eval).parameters["ensemble"].default is True
    assert inspect.signature(player.Player.root_eval).parameters["ensemble"].default is True


def test_argument_errors_that_need_no_device():
    """An engine exists only where a device does, so without one the reachable errors are the null engine's: an argument error with
    a message that names the entry point, never a crash or a silent success."""
    import tak_amd

    lib = tak_amd.load_library()
    null, f, m, c = C.c_void_p(None), C.c_float(0), C.c_int(0), C.c_uint64(0)
    calls = {
        "tg_policy_eval_symm": (null, 1, None, C.c_uint32(0xFF), C.byref(f), C.byref(f)),
        "tg_policy_eval_symm_dev": (null, 1, None, C.c_uint32(0xFF), C.byref(f), C.byref(f)),
        "tg_symm_perm_read": (null, None),
        "tg_search_set_symmetry": (null, 1),
        "tg_search_get_symmetry": (null, C.byref(m), C.byref(c)),
    }
    assert sorted(calls) == sorted(DECLARATIONS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name  # TG_ERR_INVALID_ARG
        assert "null engine" in lib.tg_last_error().decode() and name in lib.tg_last_error().decode(), name


def test_the_loop_script_takes_the_symmetry_and_defaults_to_off():
    train_loop = script("train_loop")
    assert train_loop.parse_args([]).symmetry == "off"
    assert train_loop.parse_args(["--symmetry", "hashed"]).symmetry == "hashed"
    with pytest.raises(SystemExit) as ei:
        train_loop.parse_args(["--symmetry", "random"])
    assert ei.value.code == 2
