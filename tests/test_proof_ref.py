"""The reference for proven values in the tree (tests/proof_ref.py), checked on the CPU: its arithmetic against oracle.Search,
its proofs against the rules and against the exact AND/OR reference of the solver, the closure invariant, the floors that
keep the GPU comparison from passing vacuously, and the planted mistakes each check has to reject."""
import numpy as np
import pytest

import proof_ref as P
import tactics_ref
from oracle import oracle as orc

SIZES = (5, 6)
BATCHES = (1, 4)


def _head(n):
    return orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV


def _same(a, b, what):
    assert len(a) == len(b), (what, len(a), len(b))
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), (what, f, np.nonzero(a[f] != b[f])[0][:4])


# ---- 1. arithmetic pinned ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("batch", BATCHES)
def test_proof_off_equals_the_oracle(n, batch):
    """proof=False: the dumps equal oracle.Search's bit for bit, over a play and further rollouts"""
    sts = P.inputs(n)[[0, 2, 3]]
    s = orc.Search(n, head=_head(n), evaluator=orc.EVAL_HASH, batch=batch)
    s.reset(sts)
    trees = [P.Tree(n, st, P.hash_evaluator(n), batch=batch) for st in sts]
    iters = 320 // batch
    for rnd in range(2):
        s.run(iters)
        for t in trees:
            t.run(iters)
        for g, t in enumerate(trees):
            _same(t.dump(), s.dump(g), (n, batch, rnd, g))
            assert t.nodes_proven == 0 and t.ended_on_proven == 0
        if rnd == 0:
            moves = np.array([t.root_children()[0][P.pick(t.root_children()[1], t.root_children()[2], 0, True)[0]] for t in trees], np.uint16)
            assert s.play(moves) == 0
            for t, mv in zip(trees, moves):
                t.play(mv)
    assert s.counters() == (sum(t.rollouts for t in trees), sum(t.evals for t in trees))


# ---- 2. soundness, 3. closure ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("batch", BATCHES)
def test_proofs_are_sound_and_closed(n, batch):
    r = P.reference(n, batch)
    assert r["faults"] == [[] for _ in r["trees"]]  # before the play
    for t in r["trees"]:  # after the play and the second round
        assert P.check_sound(t) == []
        assert P.check_closure(t) == []


@pytest.mark.parametrize("n", SIZES)
def test_proven_roots_against_the_exact_solver(n):
    """every root proven for a colour within 3 plies is a forced win / loss of the exact AND/OR reference at that depth"""
    ref = tactics_ref.Ref(n)
    checked = 0
    for batch in BATCHES:
        r = P.reference(n, batch)
        for st, code, depth in zip(P.inputs(n), r["roots"][0], r["root_depth"]):
            if code not in (P.PROVEN_WHITE, P.PROVEN_BLACK) or depth > 3:
                continue
            wins = int(P.status(code)) == P.to_move(st)
            assert (ref.W if wins else ref.X)(st[None], depth)[0], (n, batch, code, depth)
            checked += 1
    assert checked >= 4


# ---- 5. the floors -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", BATCHES)
def test_floors(batch):
    """what the reference alone has to yield on the inputs, so that no comparison with it passes vacuously"""
    roots, and2, deep, proven_root_later = set(), 0, 0, False
    for n in SIZES:
        r = P.reference(n, batch)
        roots |= set(r["roots"][0])
        internal = 0
        for t, pb in zip(r["trees"], r["proven_by"]):
            and2 += sum(1 for x, (how, d) in pb.items() if how == "and" and t.nchild[x] >= 2)
            deep += sum(1 for x, (how, d) in pb.items() if d >= 2)
            internal += len(pb)
        assert internal >= 20, (n, internal)
        assert r["counters"][0][0] == internal and r["counters"][0][1] > 0
        assert r["counters"][1][1] > r["counters"][0][1]  # rollouts ended on proven nodes in the second round too
        proven_root_later |= any(c >= P.PROVEN_WHITE for c in r["roots"][1])
    assert P.PROVEN_WHITE in roots and P.PROVEN_BLACK in roots
    assert and2 >= 1 and deep >= 1
    assert proven_root_later, "no rollout of the second round started at a proven root"


# ---- 4. teeth ------------------------------------------------------------------------------------------------------------------
def _run(n, st, variant, rollouts):
    t = P.Tree(n, st, P.hash_evaluator(n), proof=True, variant=variant)
    t.run(rollouts)
    return t


def test_teeth_and_rule_with_an_unknown_child():
    t = _run(5, P.inputs(5)[3], "and_with_unknown", 300)
    assert any(f.startswith("sound:") for f in P.check_sound(t))
    assert P.check_sound(_run(5, P.inputs(5)[3], None, 300)) == []


def _drawn_root():
    """a 4×4 position whose two moves both end the game: one draws, one loses → the rule gives TG_PROVEN_DRAW"""
    pos = orc.playouts(4, 3000, seed=7, style=0, half_komi=0, avoid_roads=True)["prev"]
    st = pos[orc.result(4, pos) == 0][1898]
    moves, counts = orc.movegen(4, st)
    res = orc.result(4, orc.play(4, np.repeat(st[None], counts[0], 0), moves[0, : counts[0]])[0])
    assert sorted(P.status(res).tolist()) == sorted([P.D, P.to_move(st) ^ 1])
    return st


def test_teeth_draw_counted_as_a_loss():
    st = _drawn_root()
    good = _run(4, st, None, 8)
    assert int(good.code[good.root]) == P.PROVEN_DRAW and good.proven_by[good.root][0] == "and"
    assert P.check_sound(good) == [] and P.check_closure(good) == []
    bad = _run(4, st, "draw_is_loss", 8)
    assert int(bad.code[bad.root]) in (P.PROVEN_WHITE, P.PROVEN_BLACK)
    assert any(f.startswith("sound:") for f in P.check_sound(bad))
    assert any(f.startswith("closure:") for f in P.check_closure(bad))


def test_teeth_colour_from_the_wrong_parity():
    st = P.inputs(5)[0]  # the mover wins at once: the root must be proven
    assert P.check_closure(_run(5, st, None, 100)) == []
    bad = _run(5, st, "wrong_parity", 100)
    assert any(f.startswith("closure:") for f in P.check_closure(bad)) or any(f.startswith("sound:") for f in P.check_sound(bad))


def test_teeth_status_not_carried_through_play():
    """after a play onto a proven child the closure check sees an unproven root that the rule decides"""
    sts = P.inputs(5)
    for variant, clean in ((None, True), ("status_lost_in_play", False)):
        t = _run(5, sts[2], variant, P.ROLLOUTS[5])
        mv, visits, codes = t.root_children()
        k = P.pick(visits, codes, P.to_move(sts[2]), True)[0]
        assert codes[k] >= P.PROVEN_WHITE
        t.play(mv[k])
        assert (P.check_closure(t) == []) == clean


def test_teeth_pick_ignores_the_visits_order():
    visits = np.array([5, 9, 9, 3, 7], np.uint32)
    codes = np.array([P.BLACK_ROAD, P.PROVEN_WHITE, P.WHITE_FLAT, 0, P.PROVEN_WHITE], np.uint8)
    assert P.pick(visits, codes, P.W, False) == (2, 1, 0)  # among the children decided for white: most visited, the last
    assert P.pick(visits, codes, P.W, False, variant="pick_first_proven")[0] != 2


def test_pick_step_2():
    visits = np.array([50, 9, 0, 3, 50], np.uint32)
    codes = np.array([P.PROVEN_WHITE, 0, P.PROVEN_DRAW, 0, P.WHITE_ROAD], np.uint8)
    # black to move: children 0 and 4 are decided for the opponent and left out
    assert P.pick(visits, codes, P.B, True) == (1, 2, 2)
    for ply in range(8):  # the draw runs over visits (0, 9, 0, 3, 0)
        i, step, excluded = P.pick(visits, codes, P.B, False, seed=3, slot=1, generation=2, ply=ply)
        assert i in (1, 3) and (step, excluded) == (2, 2)
        assert i == orc.pick_move(np.array([0, 9, 0, 3, 0], np.uint32), False, 3, 1, 2, ply)
    # candidates without a visit: exploit over them, the last on ties; every child lost: all are candidates
    assert P.pick(np.array([7, 0, 0], np.uint32), np.array([P.PROVEN_WHITE, 0, 0], np.uint8), P.B, False) == (2, 2, 1)
    assert P.pick(np.array([7, 8, 8], np.uint32), np.array([P.PROVEN_WHITE, P.WHITE_FLAT, P.WHITE_ROAD], np.uint8), P.B, False, seed=1)[1:] == (2, 0)
