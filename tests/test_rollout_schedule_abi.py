"""The rollout schedule's two entry points and its structure in every layer — header, version script, library, ctypes binding, Rust
binding, loop script — without touching what was there: TgSelfPlayConfig keeps its 40 bytes and the ABI its version.  Needs no GPU."""
import ctypes as C
import fnmatch
import os
import re
import subprocess

import pytest

from abi_helpers import defined_symbols, parsed_header as _parsed_header, rust_fields, script

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "takgpu.h")
ENTRY_POINTS = ("tg_selfplay_set_schedule", "tg_selfplay_schedule_stats")
FIELDS = [("boost_plies", "int32_t", None), ("boost_factor", "int32_t", None), ("reserved", "int32_t", 2)]


def test_both_entry_points_are_declared_listed_and_exported():
    import tak_amd

    functions = {name: (ret, args) for name, ret, args in _parsed_header()["functions"]}
    assert functions["tg_selfplay_set_schedule"] == ("int", [("TgEngine*", "e"), ("const TgRolloutSchedule*", "s")])
    assert functions["tg_selfplay_schedule_stats"] == ("int", [("TgEngine*", "e"), ("uint64_t*", "boosted_moves"),
                                                               ("uint64_t*", "compact_iterations"), ("uint64_t*", "compact_leaves")])
    # the version script exports by pattern: the globals' patterns cover both names, and no local pattern comes first
    script = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "tak_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.search(r"global:(.*?)local:", script, flags=re.S).group(1).replace(";", " ").split()
    defined = defined_symbols()
    for name in ENTRY_POINTS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, patterns)
        assert name in defined, name
        assert name in tak_amd.engine.ABI_SYMBOLS


def test_the_header_comments_cite_the_reference_the_ply_rule_and_the_wait():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        comment = re.findall(r"/\*((?:(?!\*/).)*?)\*/\s*TG_API int " + name + r"\(", text, flags=re.S)
        assert len(comment) == 1, name
        assert "train/src/self_play.rs:19,63" in comment[0], name
        assert "ply" in comment[0] and "wait" in comment[0], name
    block = text[text.index("Rollout schedule of the self-play driver"):text.index("TG_API int tg_selfplay_set_schedule")]
    assert "header" in block and "ply 2" in block  # Game::ply is the header's ply: the first searched move is ply 2
    step = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*TG_API int tg_selfplay_step\(", text, flags=re.S).group(1)
    assert "QUAD_ROLLOUT_PLIES" not in step and "waits once per ply" in step


def test_the_structure_is_the_same_16_bytes_in_header_ctypes_and_rust(tmp_path):
    from tak_amd import engine

    structs = dict(_parsed_header()["structs"])
    assert structs["TgRolloutSchedule"] == FIELDS
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "takgpu.h"\n'
                   "_Static_assert(sizeof(TgRolloutSchedule) == 16, \"size\");\n"
                   "_Static_assert(offsetof(TgRolloutSchedule, boost_plies) == 0, \"offset\");\n"
                   "_Static_assert(offsetof(TgRolloutSchedule, boost_factor) == 4, \"offset\");\n"
                   "_Static_assert(offsetof(TgRolloutSchedule, reserved) == 8, \"offset\");\n"
                   "_Static_assert(sizeof(TgSelfPlayConfig) == 40, \"size\");\n"
                   "_Static_assert(TG_ABI_VERSION == 5, \"abi\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # ctypes
    S = engine.TgRolloutSchedule
    assert [(f, t) for f, t in S._fields_] == [("boost_plies", C.c_int32), ("boost_factor", C.c_int32), ("reserved", C.c_int32 * 2)]
    assert C.sizeof(S) == 16 and S.boost_factor.offset == 4 and S.reserved.offset == 8
    assert C.sizeof(engine.TgSelfPlayConfig) == 40 and engine.TG_ABI_VERSION == 5
    # Rust: the raw binding's struct and functions, and the safe wrapper's settings
    rust = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    assert rust_fields("TgRolloutSchedule") == ["pub boost_plies: i32", "pub boost_factor: i32", "pub reserved: [i32; 2]"]
    assert "pub fn tg_selfplay_set_schedule(e: *mut TgEngine, s: *const TgRolloutSchedule) -> c_int;" in rust
    assert ("pub fn tg_selfplay_schedule_stats(e: *mut TgEngine, boosted_moves: *mut u64, compact_iterations: *mut u64, "
            "compact_leaves: *mut u64) -> c_int;") in rust
    safe = open(os.path.join(ROOT, "rust", "takgpu", "src", "selfplay.rs")).read()
    settings = re.search(r"pub struct SelfPlaySettings \{(.*?)\n\}", safe, flags=re.S).group(1)
    assert re.search(r"pub boost_plies: i32,", settings) and re.search(r"pub boost_factor: i32,", settings)
    defaults = re.search(r"impl Default for SelfPlaySettings \{(.*?)\n\}", safe, flags=re.S).group(1)
    assert "boost_plies: 0," in defaults and "boost_factor: 1," in defaults  # off
    assert "sys::tg_selfplay_set_schedule(network.e, &schedule)" in safe


def test_the_python_keywords_default_to_off():
    import inspect

    from tak_amd import engine

    sig = inspect.signature(engine.Engine.selfplay_create)
    assert sig.parameters["boost_plies"].default == 0 and sig.parameters["boost_factor"].default == 1
    assert hasattr(engine.Engine, "selfplay_schedule_stats") and hasattr(engine.Engine, "selfplay_set_schedule")


def _train_loop():
    train_loop = script("train_loop")
    return train_loop


def test_the_loop_script_takes_the_flags_and_leaves_the_defaults_off():
    tl = _train_loop()
    args = tl.parse_args([])
    assert (args.boost_plies, args.boost_factor) == (0, 1)
    args = tl.parse_args(["--boost-plies", "10", "--boost-factor", "4"])
    assert (args.boost_plies, args.boost_factor) == (10, 4)
    args = tl.parse_args(["--boost-plies", "512", "--boost-factor", "64"])
    assert (args.boost_plies, args.boost_factor) == (512, 64)


@pytest.mark.parametrize("argv", [["--boost-plies", "-1"], ["--boost-plies", "513"], ["--boost-factor", "0"], ["--boost-factor", "65"],
                                  ["--boost-factor", "-4"], ["--boost-plies", "ten"], ["--rollouts", str(1 << 26), "--boost-factor", "64"]])
def test_the_loop_script_rejects_bad_values(argv, capsys):
    tl = _train_loop()
    with pytest.raises(SystemExit) as ei:
        tl.parse_args(argv)
    assert ei.value.code == 2
    assert "--boost-" in capsys.readouterr().err
