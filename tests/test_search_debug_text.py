"""Node::debug restated over hand-built trees (tests/debug_ref.py), and the host-side text of NodeDebugInfo and Analysis
(alpha-tak/src/search/debug.rs, alpha-tak/src/analysis.rs) — no GPU."""
import json
import os

import numpy as np
import pytest

from debug_ref import debug_ref, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 5


def _mv(text, n=N):
    import tak_amd

    return tak_amd.parse_move(n, text)


def _bits(x):
    return np.array([x], np.float32).view(np.uint32)[0]


# ---- the restatement on hand-built trees -----------------------------------------------------------------------------------
def _tree():
    """root with five children: two ties at 5 visits, an uninitialised child, a terminal child and an expanded child whose own
    children have no visits yet"""
    a1, b1, c1, d1, e1 = (_mv(t) for t in ("a1", "b1", "c1", "d1", "e1"))
    a2, b2, c2 = _mv("a2"), _mv("b2"), _mv("c2")
    return (0, 14, 0.1, 0.0, [
        (a1, 5, 0.5, 0.2, [(a2, 2, -0.25, 0.5, [(b1, 0.0, 0.5)]), (b2, 2, 0.75, 0.5, [])]),  # tie in the continuation: b2 (last)
        (b1, 1, -1.0, 0.3, []),                                     # terminal (no children, visited)
        (c1, 5, 0.25, 0.1, [(a2, 1, 0.5, 0.6, []), (b2, 1, 0.5, 0.4, [(c2, 0.0, 1.0)])]),
        (d1, 0.0, 0.3),                                             # uninitialised
        (e1, 1, 0.5, 0.1, [(a2, 0.0, 0.5), (b2, 0.0, 0.5)]),        # expanded, children unvisited
    ])


def test_order_ties_and_continuations():
    t = _tree()
    r = debug_ref(records(t), 10, 512)
    # visits 5, 1, 5, 0, 1 → 5 (c1, index 2), 5 (a1, 0), 1 (e1, 4), 1 (b1, 1), 0 (d1)
    assert int(r["counts"]) == 5
    assert [int(m) for m in r["moves"][:5]] == [_mv(x) for x in ("c1", "a1", "e1", "b1", "d1")]
    assert list(r["visits"][:5]) == [5, 5, 1, 1, 0]
    assert not r["moves"][5:].any() and not r["visits"][5:].any()
    # c1: its children tie at 1 visit → b2 (the last), initialised with one unvisited child → one more step, to c2
    # a1: a2 and b2 tie at 2 → b2 (the last), which has no children; e1: expanded, unvisited children → its last child, b2
    assert list(r["cont_len"][:5]) == [2, 1, 1, 0, 0]
    assert [int(m) for m in r["cont_moves"][0, :2]] == [_mv("b2"), _mv("c2")] and list(r["cont_visits"][0, :2]) == [1, 0]
    assert int(r["cont_moves"][1, 0]) == _mv("b2") and r["cont_visits"][1, 0] == 2
    assert int(r["cont_moves"][2, 0]) == _mv("b2") and r["cont_visits"][2, 0] == 0
    assert not r["cont_moves"][0, 2:].any() and not r["cont_moves"][3:].any() and not r["cont_visits"][3:].any()


def test_continuation_rules_one_by_one():
    a1, a2, b2, c2 = _mv("a1"), _mv("a2"), _mv("b2"), _mv("c2")
    # an expanded node whose children have no visits: one step, to its LAST child, with 0 visits
    t = (0, 2, 0.0, 0.0, [(a1, 1, 0.5, 1.0, [(a2, 0.0, 0.5), (b2, 0.0, 0.5)])])
    r = debug_ref(records(t), 10, 512)
    assert r["cont_len"][0] == 1 and r["cont_moves"][0, 0] == b2 and r["cont_visits"][0, 0] == 0
    # ties in a continuation: the last of the most visited
    t = (0, 9, 0.0, 0.0, [(a1, 8, 0.5, 1.0, [(a2, 3, 0.1, 0.3, []), (b2, 3, 0.1, 0.3, []), (c2, 1, 0.1, 0.4, [])])])
    r = debug_ref(records(t), 10, 512)
    assert r["cont_len"][0] == 1 and r["cont_moves"][0, 0] == b2 and r["cont_visits"][0, 0] == 3
    # a terminal child (visited, no children): empty continuation
    t = (0, 4, 0.0, 0.0, [(a1, 3, 1.0, 1.0, [])])
    r = debug_ref(records(t), 10, 512)
    assert r["cont_len"][0] == 0 and r["counts"] == 1
    # depth = 0: rows without continuations; top_k bounds which rows get one
    t = _tree()
    r0 = debug_ref(records(t), 0, 512)
    assert r0["cont_moves"].shape == (512, 0) and not r0["cont_len"].any()
    full = debug_ref(records(t), 10, 512)
    r3 = debug_ref(records(t), 1, 3)
    assert np.array_equal(r3["cont_len"], np.minimum(full["cont_len"][:3], 1))
    assert np.array_equal(r3["cont_moves"][:, 0], full["cont_moves"][:3, 0])
    for k in ("moves", "visits", "reward", "policy"):
        assert np.array_equal(r3[k], full[k])


def test_eval_and_empty_root():
    r = debug_ref(records((0, 0, 0.0, 0.0, [])), 10, 512)
    assert r["counts"] == 0 and _bits(r["eval"]) == 0  # +0.0
    # children without visits: NaN, as in the reference (0 / 0)
    r = debug_ref(records((0, 1, 0.0, 0.0, [(_mv("a1"), 0.5, 0.5), (_mv("b1"), 0.5, 0.5)])), 10, 512)
    assert r["counts"] == 2 and np.isnan(r["eval"])
    # the f32 chain in sorted order, from +0.0
    t = _tree()
    r = debug_ref(records(t), 10, 512)
    acc = np.float32(0.0)
    total = np.float32(12)
    for v, q in zip(r["visits"][:5], r["reward"][:5]):
        acc = np.float32(acc + np.float32(q * np.float32(np.float32(v) / total)))
    assert _bits(acc) == _bits(r["eval"])


# ---- NodeDebugInfo text ------------------------------------------------------------------------------------------------------
def _info(tree=None):
    from tak_amd.analysis import NodeDebugInfo

    r = debug_ref(records(tree or _tree()), 10, 512)
    d = {k: np.asarray(v)[None] for k, v in r.items()}
    return NodeDebugInfo.from_search_debug(N, d, 0)


def test_node_debug_info_format():
    info = _info()
    text = f"{info:.2}"
    lines = text.split("\n")
    assert lines[0] == f"evaluation: {float(info.eval()):+.4f}"
    assert lines[1] == "turn      visited   reward   policy | continuation"
    assert lines[2] == "c1              5  +0.2500   0.1000 | b2 c2"
    assert lines[3] == "a1              5  +0.5000   0.2000 | b2"
    assert len(lines) == 5 and lines[4] == ""  # exactly two rows, each ends with a newline
    assert str(info).count("\n") == 2 + 5
    assert f"{info:.0}".count("\n") == 2
    assert str(_info((0, 0, 0.0, 0.0, []))) == "Node has no children"
    assert format(_info((0, 0, 0.0, 0.0, [])), ".3") == "Node has no children"


def test_maybe_flip_and_negative_zero():
    a1, b1 = _mv("a1"), _mv("b1")
    info = _info((0, 3, 0.0, 0.0, [(a1, 2, 0.0, 0.5, []), (b1, 1, 0.25, 0.5, [])]))
    f = info.maybe_flip(True)
    assert _bits(f.infos[0].reward) == 0x80000000  # 0.0 * -1 = -0.0
    assert "a1              2  -0.0000   0.5000 | " in str(f)
    # eval recomputed from the flipped rewards in the same order: +0.0 + (-0.0 · 2/3) + (-0.25 · 1/3)
    exp = np.float32(np.float32(0.0) + np.float32(np.float32(-0.0) * np.float32(np.float32(2) / np.float32(3))))
    exp = np.float32(exp + np.float32(np.float32(-0.25) * np.float32(np.float32(1) / np.float32(3))))
    assert _bits(f.eval()) == _bits(exp)
    assert f.infos[0].ptn_comment(True) == " {r: +0.000, p: 0.5000, v: 2}"
    assert info.infos[0].ptn_comment(True) == " {r: -0.000, p: 0.5000, v: 2}"
    assert info.maybe_flip(False) is info
    # a flip of a root whose only child has reward 0: eval stays +0.0 (the chain starts at +0.0)
    z = _info((0, 2, 0.0, 0.0, [(a1, 1, 0.0, 1.0, [])])).maybe_flip(True)
    assert _bits(z.eval()) == 0 and str(z).startswith("evaluation: +0.0000\n")


# ---- Analysis ------------------------------------------------------------------------------------------------------------------
def test_analysis_start_as_black_known_answer():
    from tak_amd.analysis import Analysis, MoveInfo

    with open(os.path.join(ROOT, "tests", "golden", "analysis_kats.json")) as fh:
        kat = json.load(fh)["start_as_black"]
    n = kat["board_size"]
    a = Analysis(n, kat["half_komi"], kat["start_ply"])
    for m in kat["moves"]:
        code = _mv(m["move"], n)
        if m["info"] is None:
            a.add_move_without_info(code)
        else:
            i = m["info"]
            a.add_move(code, MoveInfo(n, code, i["visits"], i["reward"], i["policy"], i["continuation"]), m["eval"])
    assert str(a) == kat["expected"]


@pytest.mark.parametrize("half_komi,text", [(-3, "-1.5"), (-1, "0.5"), (0, "0"), (1, "0.5"), (4, "2"), (5, "2.5")])
def test_komi_strings(half_komi, text):
    from tak_amd.analysis import Analysis

    a = Analysis(6, half_komi, 0)
    assert str(a) == f'[Size "6"]\n[Komi "{text}"]\n'
    a.add_setting("Player1", "x")
    assert str(a).endswith('[Player1 "x"]\n')


def _two_plies(prev_eval, eval_now):
    """an Analysis whose second update sees eval_diff = -(eval_now + prev_eval) in f32 → its marks"""
    from tak_amd.analysis import Analysis, MoveInfo, NodeDebugInfo

    class Fixed(NodeDebugInfo):
        def __init__(self, infos, ev):
            super().__init__(infos)
            self.ev = np.float32(ev)

        def eval(self):
            return self.ev

    a1, b1 = _mv("a1"), _mv("b1")
    a = Analysis(N, 0, 0)
    a.update(Fixed([MoveInfo(N, a1, 1, 0.0, 1.0)], prev_eval), a1)
    a.update(Fixed([MoveInfo(N, b1, 1, 0.0, 1.0)], eval_now), b1)
    return a.marks


@pytest.mark.parametrize("diff,mark", [(-0.4, "blunder"), (-0.15, "mistake"), (0.1, "strong"), (0.3, "strong"),
                                       (-0.41, "blunder"), (-0.39, "mistake"), (-0.14, None), (0.09, None), (0.31, "brilliancy")])
def test_mark_boundaries_in_f32(diff, mark):
    # prev = 0 → eval_diff = -(eval + 0) = diff exactly when eval = -diff (f32)
    marks = _two_plies(0.0, -np.float32(diff))
    assert marks == ([(0, mark)] if mark else [])
    assert np.float32(-np.float32(-np.float32(diff) + np.float32(0.0))) == np.float32(diff)


def test_branch_text_and_visit_filter():
    from tak_amd.analysis import Analysis, MoveInfo, NodeDebugInfo

    a1, b1, c1, a2, b2, c2 = (_mv(t) for t in ("a1", "b1", "c1", "a2", "b2", "c2"))
    cont = [(a2, 10_001), (b2, 10_000), (c2, 10_001)]
    info = NodeDebugInfo([MoveInfo(N, a1, 100, 0.5, 0.5, []), MoveInfo(N, b1, 91, 0.25, 0.25, cont),
                          MoveInfo(N, c1, 90, 0.0, 0.25, cont)])
    a = Analysis(N, 4, 0)
    a.update(info, a1)
    # 91 > 0.9 · 100 is a candidate, 90 is not; b2 (exactly 10 000 visits) is filtered out of the branch
    assert [(p, i.mov) for p, i in a.branches] == [(0, b1)]
    text = str(a)
    assert text.endswith("\n{0_b1}\n1. b1  {r: +0.250, p: 0.2500, v: 91} a2\n2. c2 \n"), text
    assert str(a.without_branches()) == text.split("\n{0_b1}")[0]
    # the same candidate from black's side: the comment flips, the continuation starts on the next line
    b = Analysis(N, 4, 1)
    b.update(info, a1)
    assert str(b).endswith("\n{1_b1}\n1. -- b1  {r: -0.250, p: 0.2500, v: 91}\n2. a2 c2\n"), str(b)


def test_analysis_text_marks_and_evals():
    from tak_amd.analysis import Analysis, MoveInfo, NodeDebugInfo

    a1, b1, c1 = _mv("a1"), _mv("b1"), _mv("c1")
    a = Analysis(N, 0, 0)
    a.update(NodeDebugInfo([MoveInfo(N, a1, 4, 0.25, 1.0)]), a1)     # eval +0.25
    a.update(NodeDebugInfo([MoveInfo(N, b1, 4, 0.5, 1.0)]), b1)      # eval +0.5: diff -0.75 → ply 0 is a blunder
    a.add_move_without_info(c1)
    assert a.marks == [(0, "blunder")]
    assert str(a) == ('[Size "5"]\n[Komi "0"]\n'
                      "1. a1??{evaluation: -0.500} {r: +0.250, p: 1.0000, v: 4} b1 {r: -0.500, p: 1.0000, v: 4}\n"
                      "2. c1 \n")
