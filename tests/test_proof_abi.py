"""The proof entry points in every layer — header, version script, library, ctypes binding, Rust sys binding and wrapper, the
loop script — added without touching what was there: structures keep their sizes and the ABI its version.  Needs no GPU."""
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
    "tg_search_set_proof": [("TgEngine*", "e"), ("int", "mode")],
    "tg_search_get_proof": [("TgEngine*", "e"), ("int*", "mode"), ("uint64_t*", "nodes_proven"), ("uint64_t*", "rollouts_ended_on_proven")],
    "tg_search_proof": [("TgEngine*", "e"), ("uint8_t*", "root_status"), ("uint8_t*", "child_status"), ("int32_t*", "counts")],
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


def test_the_header_states_the_rule_the_pick_and_the_life_cycle():
    text = open(HEADER).read()
    comment = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef enum TgProven", text, flags=re.S).group(1)
    for phrase in ("No counterpart in the reference", "mcts.rs:35-38", "TG_PROVEN_DRAW", "no child is unknown", "keeps its child count",
                   "never a game's result", "closed under the rule", "already has visits", "resets it to TG_PROOF_OFF", "would back a proven node up as a", "tg_pit",
                   "the LAST on ties", "real visits", "TG_ERR_STATE", "TG_ERR_INVALID_ARG", "possible_moves order"):
        assert phrase in comment, phrase
    assert "typedef enum TgProven { TG_PROVEN_WHITE = 8, TG_PROVEN_BLACK = 9, TG_PROVEN_DRAW = 10 } TgProven;" in text
    assert "typedef enum TgSearchProof { TG_PROOF_OFF = 0, TG_PROOF_ON = 1 } TgSearchProof;" in text
    record = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*typedef struct TgNodeRecord", text, flags=re.S).group(1)
    assert "TgProven" in record


def test_structures_keep_their_sizes_and_the_abi_its_version(tmp_path):
    from tak_amd import engine

    src = tmp_path / "layout.c"
    src.write_text('#include "takgpu.h"\n'
                   "_Static_assert(sizeof(TgSearchConfig) == 40 && sizeof(TgSelfPlayConfig) == 40, \"size\");\n"
                   "_Static_assert(sizeof(TgNodeRecord) == 24, \"size\");\n"
                   "_Static_assert(TG_PROOF_OFF == 0 && TG_PROOF_ON == 1, \"enum\");\n"
                   "_Static_assert(TG_PROVEN_WHITE == 8 && TG_PROVEN_BLACK == 9 && TG_PROVEN_DRAW == 10, \"enum\");\n"
                   "_Static_assert(TG_DRAW_REVERSIBLE == 6, \"the result codes stay below the proven ones\");\n"
                   "_Static_assert(TG_ABI_VERSION == 5, \"abi\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert engine.TG_ABI_VERSION == 5 and C.sizeof(engine.TgSearchConfig) == 40
    assert (engine.PROOF_OFF, engine.PROOF_ON) == (0, 1)
    assert (engine.PROVEN_WHITE, engine.PROVEN_BLACK, engine.PROVEN_DRAW) == (8, 9, 10)
    fields = dict(_parsed_header()["structs"])
    assert "proof" not in " ".join(f for f, _, _ in fields["TgSelfPlayConfig"] + fields["TgSearchConfig"])


def test_the_rust_binding_agrees_with_the_header():
    rust = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    for line in (
        "pub fn tg_search_set_proof(e: *mut TgEngine, mode: c_int) -> c_int;",
        "pub fn tg_search_get_proof(e: *mut TgEngine, mode: *mut c_int, nodes_proven: *mut u64, rollouts_ended_on_proven: *mut u64) -> c_int;",
        "pub fn tg_search_proof(e: *mut TgEngine, root_status: *mut u8, child_status: *mut u8, counts: *mut i32) -> c_int;",
        "pub const TG_PROOF_OFF: TgSearchProof = 0;",
        "pub const TG_PROOF_ON: TgSearchProof = 1;",
        "pub const TG_PROVEN_WHITE: TgProven = 8;",
        "pub const TG_PROVEN_BLACK: TgProven = 9;",
        "pub const TG_PROVEN_DRAW: TgProven = 10;",
    ):
        assert line in rust, line
    safe = "".join(open(os.path.join(ROOT, "rust", "takgpu", "src", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "rust", "takgpu", "src"))))
    for name in DECLARATIONS:
        assert f"sys::{name}(" in safe, name
    assert re.search(r"pub proof: i32", safe) and re.search(r"proof: sys::TG_PROOF_OFF", safe)
    assert re.search(r"pub fn search_set_proof\(&self", safe) and re.search(r"pub fn search_proof\(&self", safe)


def test_the_python_wrappers_exist_and_default_to_off():
    import tak_amd
    from tak_amd import engine, player

    E = engine.Engine
    for f in (E.search_create, E.selfplay_create, player.Player.__init__):
        assert inspect.signature(f).parameters["proof"].default is None, f
    for name in ("search_set_proof", "search_get_proof", "search_proof"):
        assert callable(getattr(E, name)), name
    assert engine._proof_mode("on") == tak_amd.PROOF_ON and engine._proof_mode("off") == tak_amd.PROOF_OFF
    assert engine._proof_mode(True) == 1 and engine._proof_mode(False) == 0
    with pytest.raises(ValueError):
        engine._proof_mode("maybe")
    codes = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10]
    assert tak_amd.node_status(codes).tolist() == [3, 0, 0, 1, 1, 2, 2, 3, 0, 1, 2]


def test_argument_errors_that_need_no_device():
    """without a device the reachable errors are the null engine's: an argument error whose message names the entry point"""
    import tak_amd

    lib = tak_amd.load_library()
    null, m, a, b = C.c_void_p(None), C.c_int(0), C.c_uint64(0), C.c_uint64(0)
    calls = {
        "tg_search_set_proof": (null, 1),
        "tg_search_get_proof": (null, C.byref(m), C.byref(a), C.byref(b)),
        "tg_search_proof": (null, None, None, None),
    }
    assert sorted(calls) == sorted(DECLARATIONS)
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name  # TG_ERR_INVALID_ARG
        assert "null engine" in lib.tg_last_error().decode() and name in lib.tg_last_error().decode(), name


def test_the_loop_script_takes_the_mode_and_defaults_to_off():
    train_loop = script("train_loop")
    assert train_loop.parse_args([]).proof == "off"
    assert train_loop.parse_args(["--proof", "on"]).proof == "on"
    with pytest.raises(SystemExit) as ei:
        train_loop.parse_args(["--proof", "maybe"])
    assert ei.value.code == 2
