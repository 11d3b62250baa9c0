"""CPU checks of the forced-win solver's boundary: the two exports and TgSolveConfig in the header, the generated Rust binding and
the ctypes table; and the opt-in tactical annotation of Analysis with a solver stub (no GPU: the text alone)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from abi_helpers import defined_symbols, parsed_header as _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ("tg_solve", "tg_search_solve")


def test_the_two_exports_are_in_header_rust_binding_python_table_and_library():
    import tak_amd
    from tak_amd.engine import ABI_SYMBOLS

    h = _header()
    fns = {name: args for name, _, args in h["functions"]}
    rs = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    lib = tak_amd.load_library()
    for name in NEW:
        assert name in fns and name in ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(rf"pub fn {name}\(", rs)
    assert [a for _, a in fns["tg_solve"]] == ["e", "n", "states", "cfg", "value", "best", "counts", "moves", "move_values", "budget_hit", "nodes"]
    assert [a for _, a in fns["tg_search_solve"]] == ["e", "cfg", "active", "value", "best", "counts", "moves", "move_values", "budget_hit", "nodes"]
    assert [t for t, _ in fns["tg_solve"]][4:] == ["int8_t*", "TgMove*", "int32_t*", "TgMove*", "int8_t*", "uint8_t*", "uint64_t*"]
    defined = defined_symbols()
    assert defined == {name for name, _, _ in h["functions"]}  # `nm -D` is still the header, no more and no less
    assert dict(h["defines"])["TG_ABI_VERSION"] == 5 and dict(h["defines"])["TG_SOLVE_MAX_DEPTH"] == 6


def test_solve_config_layout_header_rust_ctypes(tmp_path):
    from tak_amd.engine import TG_SOLVE_ALL_MOVES, TG_SOLVE_MAX_DEPTH, TgSolveConfig

    fields = dict(_header()["structs"])["TgSolveConfig"]
    assert fields == [("depth", "int32_t", None), ("flags", "uint32_t", None), ("node_budget", "uint64_t", None), ("reserved", "int32_t", 4)]
    assert [f for f, _ in TgSolveConfig._fields_] == [f for f, _, _ in fields]
    # the C compiler's own layout
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "takgpu.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %u %d\\n", '
                   "sizeof(TgSolveConfig), offsetof(TgSolveConfig, depth), offsetof(TgSolveConfig, flags), offsetof(TgSolveConfig, node_budget), "
                   "offsetof(TgSolveConfig, reserved), TG_SOLVE_ALL_MOVES, TG_SOLVE_MAX_DEPTH); return 0; }\n")
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 0, 4, 8, 16, 1, 6]
    assert [C.sizeof(TgSolveConfig)] + [getattr(TgSolveConfig, f).offset for f in ("depth", "flags", "node_budget", "reserved")] == got[:5]
    assert (TG_SOLVE_ALL_MOVES, TG_SOLVE_MAX_DEPTH) == (1, 6)
    rs = open(os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")).read()
    body = re.search(r"pub struct TgSolveConfig \{(.*?)\}", rs, flags=re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("depth", "i32"), ("flags", "u32"), ("node_budget", "u64"), ("reserved", "[i32; 4]")]
    wrapper = open(os.path.join(ROOT, "rust", "takgpu", "src", "solve.rs")).read()
    assert "sys::tg_solve(" in wrapper and "sys::tg_search_solve(" in wrapper and "SOLVE_ALL_MOVES: u32 = 1" in wrapper


# ---- the analysis text ------------------------------------------------------------------------------------------------------
class _Stub:
    """stands in for the Engine: play returns a state whose first byte is the played move's low byte, solve answers from a table
    keyed by (that byte, depth, to_move byte of the state)"""

    def __init__(self, table):
        self.table, self.calls = table, []

    def play(self, states, moves):
        out = np.zeros((1, 256), np.uint8)
        out[0, 0] = int(moves[0]) & 0xFF
        return out, np.zeros(1, np.uint8)

    def solve(self, states, depth, **kw):
        key = (int(states[0, 0]), int(depth), int(states[0, 256 - 15]))
        self.calls.append(key)
        return {"value": np.array([self.table.get(key, 0)], np.int8)}


def _analysis(tactics):
    import tak_amd
    from tak_amd.analysis import Analysis, MoveInfo, NodeDebugInfo

    mv = [tak_amd.parse_move(5, t) for t in ("a1", "e5", "c3", "c4", "d3", "b3")]
    evals = [0.0, 0.0, 0.0, 0.5, -0.5, 0.5]  # the swing of the evaluation marks ply 2 (c3) as a blunder, "??"
    # position after the move: c3 (marked) → opponent lost in 4; c4 → opponent lost in 2; d3 → the mover's move loses in 3;
    # b3 → nothing proven, Tak by the flipped depth-1 solve; a1 (ply 0) would be Tak too but is before ply 2
    table = {(mv[2] & 0xFF, 3, 0): -4, (mv[3] & 0xFF, 3, 0): -2, (mv[4] & 0xFF, 3, 0): 3, (mv[5] & 0xFF, 1, 1): 1, (mv[0] & 0xFF, 1, 1): 1}
    stub = _Stub(table)
    a = Analysis(5, 4, 0)
    for m, ev in zip(mv, evals):
        info = MoveInfo(5, m, 100, np.float32(ev), np.float32(0.5))
        other = MoveInfo(5, mv[0] ^ 1, 10, np.float32(ev), np.float32(0.1))
        a.update(NodeDebugInfo([info, other]), m)
        if tactics:
            a.annotate_tactics(stub, np.zeros(256, np.uint8), m, 3)
    return a, stub


def test_annotation_is_off_by_default_and_changes_nothing():
    plain, _ = _analysis(False)
    assert plain.tactics == {} and '"' not in str(plain).split("\n", 2)[2] and "forced" not in str(plain)
    noted, _ = _analysis(True)
    strip = str(noted).replace(' {forced win in 4}', "").replace(' {forced win in 2}', "").replace(" {loses in 3}", "")
    strip = strip.replace('c3"', "c3").replace('c4"', "c4").replace("b3'", "b3")
    assert strip == str(plain)


def test_annotation_marks_and_comments():
    a, stub = _analysis(True)
    text = str(a)
    assert 'c3"??{evaluation:' in text and "{forced win in 4}" in text  # `"` right behind the move, before the ?? mark
    assert 'c4"{evaluation:' in text and "{forced win in 2}" in text    # … and behind an unmarked move
    assert "d3{evaluation:" in text and "{loses in 3}" in text          # a losing move gets the comment alone
    assert "b3' {r:" in text                                            # Tak: no comment of its own (the last move has no evaluation)
    assert "a1'" not in text                                            # plies 0 and 1 place the opponent's stone: no Tak mark
    line = [ln for ln in text.splitlines() if ln.startswith("2. ")][0]
    assert line.index('c3"??') < line.index("{r:") < line.index("{forced win in 4}") < line.index('c4"') < line.index("{forced win in 2}")
    assert a.tactics == {2: ('"', " {forced win in 4}"), 3: ('"', " {forced win in 2}"), 4: ("", " {loses in 3}"), 5: ("'", "")}
    # the flipped depth-1 solve runs only where the depth-3 solve proved nothing and the ply is 2 or later
    assert [c for c in stub.calls if c[1] == 1] == [(stub.calls[-1][0], 1, 1)]
