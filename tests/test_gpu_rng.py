"""The kernels that spend the self-play randomness — k_dirichlet, k_sp_opening, the sampling branch of k_sp_pick — against the
independent statements and gates of tests/rng_ref.py.  Every test runs the DummyNet evaluator (no network), a seed above 2³² (the
upper half of the Philox key is in use) and a slot_base other than 0.

Bit for bit: the noise of every root over the kernel's whole domain of child counts (2 … 8, 63 … 66, 127 … 130, up to 225:
the `i += 64` lane loops and the serial sum) equals the oracle's, whose stream tests/test_rng_spec.py ties to rng.cuh, to Random123
and to the Gamma / Beta laws.  As statistics: the same kernel's output over 4096 games of one position passes the same Beta,
mean, correlation and row-sum gates — what parity with a like-wired oracle call cannot see (every game on one slot, ply not in the
key).  Self-play: each game's corner is bit 0 of rng_ref's opening draw, each game's move is the one rng_ref's big-integer rule
picks from the visit counts of its tree, and the picks of 4096 games follow visits / Σ visits.  Values: profiles/r15_a_rng_gates.txt."""
import functools
import importlib.util
import os
import time

import numpy as np
import pytest

import rng_ref as R
from search_helpers import _mk

pytestmark = pytest.mark.gpu

SEED = 0x9E3779B97F4A7C15
SLOT_BASE = 5000
requires_scipy = pytest.mark.skipif(importlib.util.find_spec("scipy") is None, reason="scipy is not installed: no CDF to gate against")


def _ply(st):
    h = len(st) - 16
    return int(st[h + 2]) | (int(st[h + 3]) << 8)


@functools.lru_cache(maxsize=None)
def _roots_by_child_count():
    """{board size: positions} whose child counts cover 2 … 8 (a root with ONE child does not turn up: the last empty square still
    takes a flat or a wall), 63 … 66 and 127 … 130, a spread of other counts, and the largest count found on each board (225 on 6×6)"""
    from oracle import oracle as orc

    out = {}
    wanted = set(range(1, 9)) | {63, 64, 65, 66, 127, 128, 129, 130}
    for n, many, plies in ((3, 20000, 40), (5, 6000, 120), (6, 20000, 300)):
        sts = orc.random_positions(n, many, seed=40 + n, max_plies=plies, half_komi=4)
        sts = sts[orc.result(n, sts) == 0]
        counts = orc.movegen(n, sts)[1]
        first = {}
        for i, c in enumerate(counts):
            first.setdefault(int(c), i)
        keep = {c for c in first if c in wanted} | {max(first)} | set(sorted(first)[:: max(1, len(first) // 24)])
        out[n] = sts[[first[c] for c in sorted(keep)]]
    return out


def _counts(orc, by_size):
    return np.concatenate([orc.movegen(n, sts)[1] for n, sts in by_size.items()])


def test_the_roots_cover_the_kernels_domain(orc):
    counts = set(int(c) for c in _counts(orc, _roots_by_child_count()))
    assert set(range(2, 9)) <= counts, sorted(counts)
    assert any(c <= 64 for c in counts) and any(64 < c <= 128 for c in counts) and any(c > 128 for c in counts), sorted(counts)
    assert {64, 65, 128, 129} <= counts, sorted(counts)  # a lane loop's last full pass and the first lane of its next one
    assert max(counts) > 192, sorted(counts)  # a fourth pass of the lane loops
    print(f"rng-gate k_dirichlet roots: child counts {sorted(counts)}")


def _noisy_roots(orc, n, sts, alpha, ratio, active=None):
    """search_create … search_apply_dirichlet on these roots → (search_root(), the oracle's noise per game).  The ABI takes α as f32
    and the kernel widens it, as the oracle's drivers do: the stream to compare with is the one of the f32 value (at α = 0.2 the
    f64 value's noise differs in the last bits of the small components — invisible once a ratio of 0.5 adds half a prior)"""
    import tak_amd

    games = len(sts)
    e = _mk(n, tak_amd.EVAL_DUMMY, games)
    e.search_create(games, arena_nodes=1 << 11, seed=SEED, slot_base=SLOT_BASE)
    e.search_reset(sts)
    e.search_run(1)  # expand the roots: every prior becomes the DummyNet's 1.0
    before = e.search_root()
    e.search_apply_dirichlet(alpha, ratio, active)
    r = e.search_root()
    e.close()
    cnt = orc.movegen(n, sts)[1]
    assert np.array_equal(r["counts"], cnt) and (before["prior"][np.arange(512)[None] < cnt[:, None]] == 1.0).all()
    noise = [orc.dirichlet(int(cnt[g]), float(np.float32(alpha)), SEED, SLOT_BASE + g, 0, _ply(sts[g])) for g in range(games)]
    return r, noise


@pytest.mark.parametrize("alpha", [0.03, 0.2, 1.0, 3.0])
def test_dirichlet_bits_over_the_whole_domain(orc, alpha):
    """ratio 1.0 on the DummyNet's priors: the stored prior is the noise itself (noise · 1 + 1 · 0)"""
    t0 = time.time()
    for n, sts in _roots_by_child_count().items():
        r, noise = _noisy_roots(orc, n, sts, alpha, 1.0)
        for g in range(len(sts)):
            c = len(noise[g])
            assert np.array_equal(r["prior"][g, :c].view(np.uint32), noise[g].view(np.uint32)), (n, g, c)
            assert not r["prior"][g, c:].any()
            assert abs(float(noise[g].astype(np.float64).sum()) - 1.0) < 1e-5
    print(f"rng-gate k_dirichlet parity alpha={alpha}: {time.time() - t0:.2f} s")


def test_dirichlet_ratio_and_mask(orc):
    """ratio 0.25 under a mask that leaves every third game untouched: those keep their priors bit for bit"""
    alpha, ratio = 0.2, np.float32(0.25)
    for n, sts in _roots_by_child_count().items():
        active = (np.arange(len(sts)) % 3 != 0).astype(np.uint8)
        r, noise = _noisy_roots(orc, n, sts, alpha, float(ratio), active)
        for g in range(len(sts)):
            c = len(noise[g])
            want = noise[g] * ratio + np.float32(1.0) * (np.float32(1.0) - ratio) if active[g] else np.ones(c, np.float32)
            assert np.array_equal(r["prior"][g, :c].view(np.uint32), want.astype(np.float32).view(np.uint32)), (n, g, c, active[g])


@requires_scipy
@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_dirichlet_law_through_the_abi(orc, alpha):
    """4096 games on one 5×5 position with 69 children: rng_ref's Dirichlet gates on what search_root() returns, no two games alike,
    and every row the oracle's for (slot_base + g, ply)"""
    t0 = time.time()
    games = 4096
    st = orc.from_ptn(5, ["a1", "e5"])
    sts = np.repeat(st[None], games, 0)
    r, noise = _noisy_roots(orc, 5, sts, alpha, 1.0)
    k = int(r["counts"][0])
    assert 60 <= k <= 80 and (r["counts"] == k).all()
    rows = r["prior"][:, :k]
    gates = R.dirichlet_law_gates(rows, alpha)
    R.report(f"k_dirichlet alpha={alpha} K={k} games={games}", gates)
    assert not R.failed(gates), gates
    assert len(np.unique(rows.view(np.uint32), axis=0)) == games, "two games drew the same noise"
    assert np.array_equal(rows.view(np.uint32), np.stack(noise).view(np.uint32))
    print(f"rng-gate k_dirichlet law alpha={alpha}: {time.time() - t0:.2f} s")


def test_selfplay_opening_coin_and_weighted_pick(orc):
    """Three searched plies of 4096 DummyNet games without noise, replayed on oracle.Search with every random decision made by
    rng_ref: the corner by bit 0 of the opening draw, the move by the big-integer rule on the replay's visit counts.  The engine's
    states after every ply are the replay's, game by game — so ply enters the key (plies 2, 3 and 4 draw differently) and so do the
    slot and the upper half of the seed.  At the first searched ply all games of a corner group hold the same tree (asserted, and
    compared with Engine.search_* on that position), so their picks are 2048 independent draws from one visit vector: χ² gate."""
    import tak_amd

    t0 = time.time()
    n, games, rollouts, komi, slot_base = 5, 4096, 32, 2, 777
    e = _mk(n, tak_amd.EVAL_DUMMY, games)
    e.selfplay_create(games, arena_nodes=1 << 14, seed=SEED, slot_base=slot_base, rollouts=rollouts, noise_plies=0, exploit_plies=100,
                      komi=komi, total_games=games, max_examples=1024)
    slots = slot_base + np.arange(games, dtype=np.uint64)
    # the opening: a1, then the far corner of column a (bit 1) or of the last column (bit 0)
    bit = R.rng_draw_np(SEED, slots, 0, 0, R.RNG_OPENING, 0, 0)[:, 0] & 1
    for g in range(0, games, 512):
        assert R.opening_bit(SEED, slot_base + g, 0) == bit[g]
    heads = R.binomial_gate("corner", int(bit.sum()), games, 0.5)
    R.report(f"k_sp_opening games={games}", [heads])
    assert heads.ok, heads
    start = orc.new_game(n, half_komi=2 * komi)
    sts, status = orc.play(n, np.repeat(start[None], games, 0), np.zeros(games, np.uint16))
    assert not status.any()
    sts, status = orc.play(n, sts, np.where(bit == 1, (n - 1) * n, (n - 1) * n + n - 1).astype(np.uint16))
    assert not status.any()
    s = orc.Search(n, head=orc.HEAD_FC5, evaluator=orc.EVAL_DUMMY, seed=SEED)
    s.set_threads(min(8, os.cpu_count() or 1))
    s.reset(sts)
    for searched in range(3):
        ply = 2 + searched
        s.run(rollouts)
        root = s.root()
        moves, visits, counts = root["moves"], root["visits"], root["counts"]
        words = R.rng_draw_np(SEED, slots, 0, ply, R.RNG_PICK, 0, 0)
        want = np.array([R.pick_from_words(words[g, 0], words[g, 1], visits[g, : counts[g]]) for g in range(games)])
        assert R.pick(SEED, slot_base + 5, 0, ply, visits[5, : counts[5]]) == want[5]
        e.selfplay_step(1)
        after = e.search_states()
        # each game's played move, found by playing every legal move of its position
        played = np.full(games, -1)
        for g in range(games):
            nxt, status = orc.play(n, np.repeat(sts[g][None], counts[g], 0), moves[g, : counts[g]])
            hit = np.nonzero((nxt == after[g]).all(1) & (status == 0))[0]
            assert len(hit) == 1, (ply, g, hit)
            played[g] = hit[0]
        assert np.array_equal(played, want), (ply, np.nonzero(played != want)[0][:8])
        assert (visits[np.arange(games), played] > 0).all(), "a child without visits was played"
        if searched == 0:
            for b in (0, 1):
                grp = np.nonzero(bit == b)[0]
                # the precondition: one tree per corner group, and it is the tree the engine's own search builds there
                assert (counts[grp] == counts[grp[0]]).all() and (moves[grp] == moves[grp[0]]).all() and (visits[grp] == visits[grp[0]]).all()
                e2 = _mk(n, tak_amd.EVAL_DUMMY, 1)
                e2.search_create(1, arena_nodes=1 << 13, seed=1)
                e2.search_reset(sts[grp[0]][None])
                e2.search_run(rollouts)
                r2 = e2.search_root()
                e2.close()
                c = int(counts[grp[0]])
                assert r2["counts"][0] == c and np.array_equal(r2["visits"][0], visits[grp[0]]) and np.array_equal(r2["moves"][0], moves[grp[0]])
                v = visits[grp[0], :c].astype(np.float64)
                assert v.sum() == rollouts - 1 and (v == 0).any() and (v > 0).sum() > 1
                if importlib.util.find_spec("scipy") is not None:
                    gate = R.chi2_gate(f"pick corner {b}", np.bincount(played[grp], minlength=c), len(grp) * v / v.sum())
                    R.report(f"k_sp_pick ply={ply} games={len(grp)} children={c} visited={int((v > 0).sum())}", [gate])
                    assert gate.ok, gate
        mv = moves[np.arange(games), played]
        assert s.play(mv) == 0
        sts = s.states()
        assert np.array_equal(sts, after)
    st = e.selfplay_stats()
    assert st["plies"] == 3 and st["games_finished"] == 0 and st["instant_wins"] == 0 and st["aborted_games"] == 0
    e.close()
    print(f"rng-gate selfplay coin and pick: {time.time() - t0:.2f} s")
