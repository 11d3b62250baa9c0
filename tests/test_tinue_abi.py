"""CPU checks of the road-only solver's boundary: TG_SOLVE_ROAD_ONLY in the header, the Rust binding and the ctypes table, the
library's exports unchanged, and the road-only tactical annotation of Analysis with a solver stub (no GPU: the text alone)."""
import inspect
import os
import subprocess

import numpy as np

from abi_helpers import LIB_RS, ROOT, defined_symbols, parsed_header as _header


def test_the_flag_is_in_header_rust_binding_and_ctypes(tmp_path):
    import tak_amd
    from tak_amd import abi
    from tak_amd.engine import TG_SOLVE_ALL_MOVES, TG_SOLVE_ROAD_ONLY, Engine

    h = _header()
    defines = dict(h["defines"])
    assert (defines["TG_SOLVE_ALL_MOVES"], defines["TG_SOLVE_ROAD_ONLY"], defines["TG_SOLVE_MAX_DEPTH"], defines["TG_ABI_VERSION"]) == (1, 4, 6, 5)
    assert (TG_SOLVE_ALL_MOVES, TG_SOLVE_ROAD_ONLY) == (1, 4) and abi.TG_SOLVE_ROAD_ONLY == 4 and tak_amd.engine.TG_SOLVE_ROAD_ONLY == 4
    # the C compiler's own reading of the header
    src = tmp_path / "flag.c"
    src.write_text('#include <stdio.h>\n#include "takgpu.h"\nint main(void) { printf("%u %u %d\\n", TG_SOLVE_ROAD_ONLY, '
                   "TG_SOLVE_ALL_MOVES | TG_SOLVE_ROAD_ONLY, (int)sizeof(TgSolveConfig)); return 0; }\n")
    exe = str(tmp_path / "flag")
    subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["4", "5", "32"]
    assert "pub const TG_SOLVE_ROAD_ONLY: i32 = 4;" in open(LIB_RS).read()
    wrapper = open(os.path.join(ROOT, "rust", "takgpu", "src", "solve.rs")).read()
    assert "SOLVE_ROAD_ONLY: u32 = 4" in wrapper and "SOLVE_ALL_MOVES: u32 = 1" in wrapper
    # no new entry points: `nm -D` is still exactly the header
    assert defined_symbols() == {name for name, _, _ in h["functions"]}
    assert Engine._solve_flags(False, False) == 0 and Engine._solve_flags(True, False) == 1
    assert Engine._solve_flags(False, True) == 4 and Engine._solve_flags(True, True) == 5
    for fn in (Engine.solve, Engine.search_solve):
        assert inspect.signature(fn).parameters["road_only"].default is False
    assert inspect.signature(tak_amd.Player.__init__).parameters["tactics_road_only"].default is False


def test_the_documents_no_longer_call_the_tinue_missing():
    header = open(os.path.join(ROOT, "include", "takgpu.h")).read()
    assert "not a road-only tinue" not in header and "Bit 1" in header
    assert "not the road-only tinuë" not in open(os.path.join(ROOT, "README.md")).read()
    assert "not the road-only tinuë" not in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the analysis text ------------------------------------------------------------------------------------------------------
class _Stub:
    """stands in for the Engine: play returns a state whose first byte is the played move's low byte (the to_move byte flips), solve
    answers (value, best) from a table keyed by (that byte, depth, to_move byte of the state) and records its keyword arguments"""

    def __init__(self, table):
        self.table, self.calls = table, []

    def play(self, states, moves):
        out = np.zeros((1, 256), np.uint8)
        out[0, 0] = int(moves[0]) & 0xFF
        out[0, 256 - 15] = states[0, 256 - 15] ^ 1 if states.shape[1] == 256 else 0
        return out, np.zeros(1, np.uint8)

    def solve(self, states, depth, **kw):
        key = (int(states[0, 0]), int(depth), int(states[0, 256 - 15]))
        self.calls.append((key, kw))
        value, best = self.table.get(key, (0, 0))
        return {"value": np.array([value], np.int8), "best": np.array([best], np.uint16), "budget_hit": np.zeros(1, np.uint8)}


def _analysis(road_only):
    import tak_amd
    from tak_amd.analysis import Analysis, MoveInfo, NodeDebugInfo

    mv = [tak_amd.parse_move(5, t) for t in ("a1", "e5", "c3", "c4", "d3", "b3")]
    line = [tak_amd.parse_move(5, t) for t in ("a2", "b2", "c2")]
    lo = lambda m: m & 0xFF  # noqa: E731
    evals = [0.0, 0.0, 0.0, 0.5, -0.5, 0.5]  # the swing of the evaluation marks ply 2 (c3) as a blunder, "??"
    # (the stub's states after a played move have to_move 1: the zero state has 0)
    # c3 (marked): the opponent is lost in 2, line a2 b2; c4: the move loses in 3, line a2 b2 c2; d3: nothing proven, Tak by the flipped
    # depth-1 solve; b3: nothing
    table = {(lo(mv[2]), 3, 1): (-2, line[0]), (lo(mv[2]), 2, 1): (-2, line[0]), (lo(line[0]), 1, 0): (1, line[1]),
             (lo(mv[3]), 3, 1): (3, line[0]), (lo(line[0]), 2, 0): (-2, line[1]), (lo(line[1]), 1, 1): (1, line[2]),
             (lo(mv[4]), 1, 0): (1, 0)}
    stub = _Stub(table)
    a = Analysis(5, 4, 0)
    for m, ev in zip(mv, evals):
        info = MoveInfo(5, m, 100, np.float32(ev), np.float32(0.5))
        other = MoveInfo(5, mv[0] ^ 1, 10, np.float32(ev), np.float32(0.1))
        a.update(NodeDebugInfo([info, other]), m)
        a.annotate_tactics(stub, np.zeros(256, np.uint8), m, 3, **({"road_only": True} if road_only else {}))
    return a, stub, mv, line


def test_road_only_annotation_marks_comments_and_lines():
    a, stub, mv, line = _analysis(True)
    text = str(a)
    assert 'c3"??{evaluation:' in text and "{tinue in 2} {a2 b2}" in text       # `"` right behind the move, before the ?? mark
    assert "c4{evaluation:" in text and "{road loss in 3} {a2 b2 c2}" in text  # a losing move gets the comment and the line alone
    assert "d3'{evaluation:" in text                                           # Tak: no comment of its own
    assert "forced win" not in text and "loses in" not in text and "b3'" not in text and "a1'" not in text
    row = [ln for ln in text.splitlines() if ln.startswith("2. ")][0]
    assert row.index('c3"??') < row.index("{r:") < row.index("{tinue in 2} {a2 b2}") < row.index("c4{") < row.index("{road loss in 3}")
    assert a.tactics == {2: ('"', " {tinue in 2} {a2 b2}"), 3: ("", " {road loss in 3} {a2 b2 c2}"), 4: ("'", "")}
    # every solve carries the flag and the budget; the calls: per move the depth-3 solve, then either the line's re-solves at the
    # depths that remain or, from ply 2 on, the flipped depth-1 solve
    assert all(kw == {"node_budget": 1 << 16, "road_only": True} for _, kw in stub.calls)
    lo = lambda m: m & 0xFF  # noqa: E731
    assert [k for k, _ in stub.calls] == [
        (lo(mv[0]), 3, 1), (lo(mv[1]), 3, 1),
        (lo(mv[2]), 3, 1), (lo(mv[2]), 2, 1), (lo(line[0]), 1, 0),
        (lo(mv[3]), 3, 1), (lo(mv[3]), 3, 1), (lo(line[0]), 2, 0), (lo(line[1]), 1, 1),
        (lo(mv[4]), 3, 1), (lo(mv[4]), 1, 0),
        (lo(mv[5]), 3, 1), (lo(mv[5]), 1, 0)]


def test_the_default_annotation_never_passes_the_flag():
    a, stub, mv, _ = _analysis(False)
    assert all(kw == {"node_budget": 1 << 16} for _, kw in stub.calls)
    assert a.tactics[2] == ('"', " {forced win in 2}") and a.tactics[3] == ("", " {loses in 3}") and a.tactics[4] == ("'", "")
    assert "tinue" not in str(a) and "road loss" not in str(a)


def test_forced_line_reports_a_budget_that_ran_out():
    import pytest

    from tak_amd.analysis import forced_line

    class Cut(_Stub):
        def solve(self, states, depth, **kw):
            r = super().solve(states, depth, **kw)
            if int(depth) == 1:
                r["value"][0], r["budget_hit"][0] = 0, 1
            return r

    stub = Cut({(0, 2, 0): (-2, 7), (7, 1, 0): (1, 9)})
    with pytest.raises(RuntimeError, match="node_budget"):
        forced_line(stub, np.zeros(256, np.uint8), 2, road_only=True)
    assert forced_line(_Stub({}), np.zeros(256, np.uint8), 3) == []
