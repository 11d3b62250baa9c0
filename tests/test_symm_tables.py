"""The references of the symmetry tests, checked on the CPU: the policy permutation tables built from oracle.augment (bijective, a
group action in the order of tak/src/symm.rs:11-20, the identity at s = 0, the same from legal moves of positions as from the
enumeration of all slots), the hashed-image rule (tests/symm_ref.py: all 8 images, uniform, a function of the whole packed
state) and the f32 fold in the order include/takgpu.h states — shown to reject the two folds one would write by mistake."""
import numpy as np
import pytest

import posgen
import rng_ref
import symm_ref

CASES = [(5, True), (6, False), (5, False)]  # the FC5 head (legacy table), the 6×6 conv head, the 5×5 conv head


def _head(orc, fc5):
    return orc.HEAD_FC5 if fc5 else orc.HEAD_CONV


@pytest.mark.parametrize("n,fc5", CASES)
def test_tables_are_bijective_and_identity_first(orc, n, fc5):
    perm = symm_ref.perm_tables(n, fc5)
    P = orc.policy_size(n, _head(orc, fc5))
    assert perm.shape == (8, P) and P == {(5, True): 1575, (6, False): 9036, (5, False): 3075}[(n, fc5)]
    assert (perm >= 0).all(), "a slot without an image"
    assert np.array_equal(perm[0], np.arange(P))
    for s in range(8):
        assert np.array_equal(np.sort(perm[s]), np.arange(P)), s


@pytest.mark.parametrize("n,fc5", CASES)
def test_tables_obey_the_group_law(orc, n, fc5):
    perm = symm_ref.perm_tables(n, fc5)
    comp = symm_ref.composition(n)
    assert np.array_equal(comp[0], np.arange(8)) and np.array_equal(comp[:, 0], np.arange(8))
    assert all(sorted(comp[s]) == list(range(8)) for s in range(8))
    assert comp[1, 1] == 2 and comp[1, 3] == 0 and comp[4, 4] == 0 and comp[1, 4] == 5  # rotate² , rotate⁴ = 1, mirror² = 1, "mirror then rotate"
    for s in range(8):
        for t in range(8):
            assert np.array_equal(perm[comp[s, t]], perm[s][perm[t]]), (s, t)


@pytest.mark.parametrize("n,fc5", CASES)
def test_tables_from_legal_moves_of_positions_agree_with_the_enumeration(orc, n, fc5):
    head = _head(orc, fc5)
    perm = symm_ref.perm_tables(n, fc5)
    corners, ok = posgen.repr_corner_states(orc, n)
    sts = np.concatenate([posgen.distinct_positions(orc, n, 200, seed=40 + n, max_plies=70), corners[ok][:100]])
    mv, cnt = orc.movegen(n, sts)
    seen = np.full(perm.shape, -1, np.int64)
    for i in range(len(sts)):
        moves = mv[i, : cnt[i]]
        slots = symm_ref._image_slots(orc, n, head, sts[i], moves)
        if fc5 or n != 5:  # (oracle.move_index answers for the board size's own head: the legacy table on 5×5)
            assert np.array_equal(slots[0], orc.move_index(n, moves))
        # the images of the legal moves are the legal moves of the image
        img = symm_ref.image_states(orc, n, head, sts[i][None])[0]
        for s in (1, 6):
            lm, lc = orc.movegen(n, img[s])
            assert lc[0] == cnt[i]
        symm_ref.perm_from_moves(orc, n, head, sts[i], moves, seen)
    covered = seen >= 0
    # every placement slot and spreads besides: what play does not reach (long spreads of tall stacks) is the enumeration's to cover
    assert covered[0].sum() > 3 * n * n, covered[0].sum()
    assert np.array_equal(seen[covered], perm[covered])


def test_hashed_image_is_uniform_over_positions_and_seeds(orc):
    n = 5
    sts = posgen.distinct_positions(orc, n, 3000, seed=77, max_plies=70)
    gates = []
    for seed in (0, 1, 0x9E3779B97F4A7C15):
        s = symm_ref.hashed_symmetry(orc, n, sts, seed)
        counts = np.bincount(s, minlength=8)
        assert (counts > 0).all(), counts
        gates.append(rng_ref.chi2_gate(f"seed {seed:#x}", counts, np.full(8, len(sts) / 8.0)))
    rng_ref.report("hashed image", gates)
    assert not rng_ref.failed(gates)
    # the Philox statement is rng_ref's; the oracle's own agrees with it on this packing
    for st in sts[:16]:
        h = orc.state_hash(n, st)
        want = rng_ref.philox(5, h & rng_ref.M32, h >> 32, symm_ref.SYMM_TAG, 0)
        assert tuple(int(x) for x in orc.philox(5, h & rng_ref.M32, h >> 32, symm_ref.SYMM_TAG, 0)) == want
        assert symm_ref.hashed_symmetry(orc, n, st[None], 5)[0] == want[0] & 7
    # the counter domain collides with none of the engine's other draws: their third word is ply | purpose << 16, purpose < 16
    assert symm_ref.SYMM_TAG >> 16 >= 16


def test_hashed_image_depends_on_the_whole_packed_state(orc):
    """states that differ only in ply, or only in komi, are different positions to the hash: over 400 of them the image changes
    for some (7/8 of them in expectation) — the rule keys on the packed state, not on the board alone"""
    n = 5
    sts = posgen.distinct_positions(orc, n, 400, seed=78, max_plies=40)
    base = symm_ref.hashed_symmetry(orc, n, sts, 3)
    ply = symm_ref.hashed_symmetry(orc, n, posgen.with_header(sts, ply=posgen.header(sts, "ply") + 2), 3)
    komi = symm_ref.hashed_symmetry(orc, n, posgen.with_header(sts, half_komi=np.full(len(sts), 5)), 3)
    assert (ply != base).sum() > 200 and (komi != base).sum() > 200
    assert np.array_equal(base, symm_ref.hashed_symmetry(orc, n, sts.copy(), 3))  # and on nothing else
    assert (symm_ref.hashed_symmetry(orc, n, sts, 4) != base).sum() > 200  # the seed is the key


def test_fold_reference_has_teeth():
    """The order the header states — ascending s, product with 1/k last — against the two folds one would write by mistake, on softmax
    rows of the FC5 head's width: each wrong fold differs from the reference in the bits of some output (else it is reported as
    invisible on this data, and the gate would prove nothing about it)."""
    rng = np.random.default_rng(0)
    perm = symm_ref.perm_tables(5, True)
    P = perm.shape[1]
    logits = rng.normal(0, 3, (8, P)).astype(np.float32)
    p = np.exp(logits - logits.max(1, keepdims=True))
    p = (p / p.sum(1, keepdims=True)).astype(np.float32)
    v = np.tanh(rng.normal(0, 1, 8)).astype(np.float32)
    for mask, descending_visible, divide_first_visible in ((0xFF, True, False), (0x24, False, False), (0x07, True, True)):
        # descending: two terms commute, three or more do not.  dividing first: with k a power of two the factor 1/k scales every
        # term exactly, so the fold is bit-equal — INVISIBLE at k = 8 and k = 2 on any data; k = 3 shows it
        sel = symm_ref.selected(mask)
        want_p, want_v = symm_ref.fold(p[: len(sel)], v[: len(sel)], perm, mask)
        assert want_p.dtype == np.float32
        assert abs(float(want_p.astype(np.float64).sum()) - 1.0) < 1e-5  # a mean of permuted distributions
        for kw, visible in ((dict(order="descending"), descending_visible), (dict(divide="first"), divide_first_visible)):
            got_p, _ = symm_ref.fold(p[: len(sel)], v[: len(sel)], perm, mask, **kw)
            differs = int((got_p.view(np.uint32) != want_p.view(np.uint32)).sum())
            print(f"symm-fold teeth: mask {mask:#04x} {kw}: {differs} of {P} policy entries differ in bits"
                  + ("" if visible else " (invisible: bit-equal by arithmetic)"))
            assert (differs > 0) == visible, (mask, kw, differs)
    # one image: the fold is that image's row through the permutation, bit for bit
    for s in (0, 7):
        got_p, got_v = symm_ref.fold(p[:1], v[:1], perm, 1 << s)
        assert np.array_equal(got_p, p[0][perm[s]]) and got_v == v[0]
