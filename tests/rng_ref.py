"""Independent statements of the self-play randomness and the gates its tests share.  A plain module, like
torch_ref.py and posgen.py: Python integers, numpy and (for the gates that need a CDF) scipy; nothing here is transcribed from
tak_amd/csrc/rng.cuh or oracle/tak_mcts.hpp.

Bit level
  philox / philox_np   Philox4x32-10 as published (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11;
                       Random123's philox4x32_R(10, ctr, key)): a round multiplies words 0 and 2 of the counter by 0xD2511F53 and
                       0xCD9E8D57, the new counter is (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), and the key is bumped by the Weyl
                       constants (0x9E3779B9, 0xBB67AE85) between rounds.  The known-answer vectors of Random123's kat_vectors are KATS.
  rng_draw             the counter packing as DESIGN.md words it: key = seed (low word, high word), counter = (slot, generation,
                       ply | purpose << 16, index | attempt << 16)
  pick                 WeightedIndex over visit counts from one draw: target = (x · total) >> 64 with x = word0 << 32 | word1, the
                       first child whose running visit sum exceeds target
  shuffle              the training order: Fisher–Yates from the last position down, position i swaps with (x · (i + 1)) >> 64 where
                       x comes from Philox(seed; i, "rain", 0, 0)

Gates — one place for every threshold.  p = P_GATE = 1e-6 per gate: the seeds are fixed, so nothing flakes; p only states how
surprising a result must be before the sampler is called wrong.  The bounds are derived (below), never measured on the code under
test.
  ks_gate      one-sample Kolmogorov–Smirnov distance D against a CDF; D ≤ sqrt(ln(2 / p) / (2 n)), the Dvoretzky–Kiefer–Wolfowitz
               inequality with Massart's constant: P(D > ε) ≤ 2 exp(−2 n ε²) at every n
  chi2_gate    Pearson's X² over cells, cells of expected count < 5 pooled into one (the usual validity rule of the χ² approximation);
               passes when scipy.stats.chi2.sf(X², cells − 1) ≥ p
  z_gate       |estimate − expectation| ≤ z(p) · standard error, z(p) the two-sided normal quantile (4.89 at 1e-6);
               binomial_gate is the same for a count of n Bernoulli(q) trials, standard error sqrt(n q (1 − q))
"""
import math
import statistics
from collections import namedtuple

import numpy as np

M32 = 0xFFFFFFFF
RNG_OPENING, RNG_GAMMA, RNG_PICK = 1, 2, 3
TRAIN_TAG = int.from_bytes(b"rain", "big")  # 0x7261696e, the second counter word of the training shuffle

# counter, key, result: Random123 kat_vectors, philox4x32 10
KATS = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((M32, M32, M32, M32), (M32, M32), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


# ---- bit level ----------------------------------------------------------------------------------------------------------------------

def philox_ctr_key(ctr, key, rounds=10):
    """philox4x32_R(rounds, ctr, key) on Python integers"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for r in range(rounds):
        if r:
            k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
        hi0, lo0 = divmod(0xD2511F53 * c0, 1 << 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c2, 1 << 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def philox(seed, c0, c1, c2, c3):
    """the engine's keying: the 64-bit seed is the key, low word first"""
    return philox_ctr_key((c0, c1, c2, c3), (seed & M32, (seed >> 32) & M32))


def rng_draw(seed, slot, generation, ply, purpose, index, attempt):
    assert 0 <= ply < 1 << 16 and 0 <= purpose < 1 << 16 and 0 <= index < 1 << 16 and 0 <= attempt < 1 << 16
    return philox(seed, slot & M32, generation & M32, ply | (purpose << 16), index | (attempt << 16))


def philox_np(seed, c0, c1, c2, c3):
    """the same on numpy arrays (any broadcastable mix of arrays and integers) → uint32 array [..., 4]"""
    seed, c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, np.uint64) for v in (seed, c0, c1, c2, c3)])
    m = np.uint64(M32)
    s32 = np.uint64(32)
    k0, k1 = seed & m, seed >> s32
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & m, (k1 + np.uint64(0xBB67AE85)) & m
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2  # 32 × 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m, (p0 >> s32) ^ c3 ^ k1, p0 & m
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def rng_draw_np(seed, slot, generation, ply, purpose, index, attempt):
    u = lambda v: np.asarray(v, np.uint64)
    return philox_np(seed, slot, generation, u(ply) | (u(purpose) << np.uint64(16)), u(index) | (u(attempt) << np.uint64(16)))


def pick_from_words(w0, w1, visits):
    """the weighted pick given the draw's first two words; visits: non-negative integers with a positive sum"""
    visits = [int(v) for v in visits]
    total = sum(visits)
    assert total > 0
    target = (((int(w0) << 32) | int(w1)) * total) >> 64
    running = 0
    for i, v in enumerate(visits):
        running += v
        if running > target:
            return i
    raise AssertionError("target < total always holds")


def pick(seed, slot, generation, ply, visits):
    w = rng_draw(seed, slot, generation, ply, RNG_PICK, 0, 0)
    return pick_from_words(w[0], w[1], visits)


def opening_bit(seed, slot, generation):
    """bit 0 of word 0 of the opening draw: 1 = the far corner of column a, 0 = the far corner of the last column"""
    return rng_draw(seed, slot, generation, 0, RNG_OPENING, 0, 0)[0] & 1


def shuffle(seed, n):
    order = list(range(n))
    for i in range(n - 1, 0, -1):
        w = philox(seed, i, TRAIN_TAG, 0, 0)
        j = (((w[0] << 32) | w[1]) * (i + 1)) >> 64
        order[i], order[j] = order[j], order[i]
    return order


# ---- gates --------------------------------------------------------------------------------------------------------------------------

P_GATE = 1e-6
Gate = namedtuple("Gate", "name value bound ok")


def _scipy_stats():
    import scipy.stats

    return scipy.stats


def z_crit(p=P_GATE):
    return statistics.NormalDist().inv_cdf(1.0 - p / 2.0)


def ks_bound(n, p=P_GATE):
    return math.sqrt(math.log(2.0 / p) / (2.0 * n))


def ks_distance(samples, cdf, lo=None):
    """sup |F_n − F| with F_n the empirical CDF of ALL samples, the sup taken at the samples ≥ lo (all of them without lo)"""
    x = np.sort(np.asarray(samples, np.float64))
    n = len(x)
    first = 0 if lo is None else int(np.searchsorted(x, lo, "left"))
    f = cdf(x[first:])
    i = np.arange(first, n, dtype=np.float64)
    return float(max(((i + 1.0) / n - f).max(), (f - i / n).max()))


def ks_gate(name, samples, cdf, lo=None, p=P_GATE):
    d, b = ks_distance(samples, cdf, lo), ks_bound(len(samples), p)
    return Gate(name, d, b, d <= b)


def chi2_gate(name, observed, expected, p=P_GATE):
    """value = the p-value, bound = p; a cell whose expectation is 0 must be empty (value −1 otherwise: no p-value excuses it)"""
    o, e = np.asarray(observed, np.float64).ravel(), np.asarray(expected, np.float64).ravel()
    assert o.shape == e.shape and abs(o.sum() - e.sum()) <= 1e-6 * e.sum()
    if o[e == 0].any():
        return Gate(name, -1.0, p, False)
    small = e < 5.0
    oo, ee = list(o[~small]), list(e[~small])
    if e[small].sum() > 0:
        oo.append(o[small].sum())
        ee.append(e[small].sum())
        if ee[-1] < 5.0 and len(ee) > 1:  # the pool itself is still small: it joins the smallest other cell
            k = int(np.argmin(ee[:-1]))
            oo[k] += oo.pop()
            ee[k] += ee.pop()
    oo, ee = np.array(oo), np.array(ee)
    assert len(ee) >= 2
    sf = float(_scipy_stats().chi2.sf(((oo - ee) ** 2 / ee).sum(), len(ee) - 1))
    return Gate(name, sf, p, sf >= p)


def z_gate(name, estimate, expectation, std_error, p=P_GATE):
    z = abs(float(estimate) - float(expectation)) / float(std_error)
    return Gate(name, z, z_crit(p), z <= z_crit(p))


def binomial_gate(name, count, n, q, p=P_GATE):
    return z_gate(name, count, n * q, math.sqrt(n * q * (1.0 - q)), p)


def failed(gates):
    return [g.name for g in gates if not g.ok]


def report(what, gates):
    for g in gates:
        print(f"rng-gate {what}: {g.name:10s} {g.value:.4g} (bound {g.bound:.4g}) {'ok' if g.ok else 'REJECTED'}")


# ---- the laws -----------------------------------------------------------------------------------------------------------------------

def gamma_law_gates(x, alpha):
    """Gamma(alpha, 1) draws: every draw finite and > 0; KS against scipy's gamma; mean alpha with standard error sqrt(alpha / n);
    variance alpha, the sample variance's standard error sqrt((μ4 − σ⁴) / n) with μ4 = 3 α² + 6 α"""
    x = np.asarray(x, np.float64)
    n = len(x)
    bad = int((~np.isfinite(x)).sum() + (x <= 0).sum())
    return [
        Gate("positive", bad, 0, bad == 0),
        ks_gate("ks", x, _scipy_stats().gamma(alpha).cdf),
        z_gate("mean", x.mean(), alpha, math.sqrt(alpha / n)),
        z_gate("variance", x.var(), alpha, math.sqrt((2.0 * alpha * alpha + 6.0 * alpha) / n)),
    ]


def _dirichlet_moment(alpha, k, a, b):
    """E[X1^a · X2^b] of the symmetric Dirichlet(alpha) on k components = Γ(A) / Γ(A + a + b) · Γ(α + a) / Γ(α) · Γ(α + b) / Γ(α)"""
    lg = math.lgamma
    return math.exp(lg(k * alpha) - lg(k * alpha + a + b) + lg(alpha + a) + lg(alpha + b) - 2.0 * lg(alpha))


def dirichlet_law_gates(rows, alpha, pairs=None):
    """rows: games × K noise vectors as the engine stores them (f32).
    rowsum    every row sums to 1 within 1e-5
    ks        one component per game (index g mod K, so the samples are independent) against Beta(α, (K − 1) α), compared at
              x ≥ 1e-30 only: a component below f32's range is a property of the f32 output, not of the sampler
    mean      per index, the mean over games against 1 / K, standard error sqrt(var / games), var = (1/K)(1 − 1/K) / (K α + 1);
              the largest |z| over the indices is reported, every index is held to z(p)
    corr      for a few fixed pairs (i, j) the correlation over games, with the known mean and variance:
              r = mean((x_i − 1/K)(x_j − 1/K)) / var against −1 / (K − 1); the standard error of that mean comes from the exact
              fourth moments of the Dirichlet (_dirichlet_moment); the pair with the largest |z| is reported, every pair held to z(p)"""
    rows = np.asarray(rows)
    games, k = rows.shape
    x = rows.astype(np.float64)
    dev = float(np.abs(x.sum(1) - 1.0).max())
    own = x[np.arange(games), np.arange(games) % k]
    mu, var = 1.0 / k, (1.0 / k) * (1.0 - 1.0 / k) / (k * alpha + 1.0)
    zmean = np.abs(x.mean(0) - mu) / math.sqrt(var / games)
    # c = (x_i − μ)(x_j − μ): E c = cov = −μ² / (Kα + 1) = var · (−1 / (K − 1)), E c² from the moments up to order (2, 2)
    m = lambda a, b: _dirichlet_moment(alpha, k, a, b)
    cov = m(1, 1) - mu * mu
    ec2 = sum(math.comb(2, a) * math.comb(2, b) * (-mu) ** (4 - a - b) * (m(a, b) if a + b else 1.0) for a in range(3) for b in range(3))
    se = math.sqrt((ec2 - cov * cov) / games) / var
    if pairs is None:
        pairs = sorted({(0, 1), (0, k - 1), (1, 2), (k // 2, k - 1)})
    zc = [abs(float(((x[:, i] - mu) * (x[:, j] - mu)).mean()) / var - cov / var) / se for i, j in pairs]
    assert abs(cov / var + 1.0 / (k - 1)) < 1e-12
    return [
        Gate("rowsum", dev, 1e-5, dev <= 1e-5),
        ks_gate("ks", own, _scipy_stats().beta(alpha, (k - 1) * alpha).cdf, lo=1e-30),
        Gate("mean", float(zmean.max()), z_crit(), bool((zmean <= z_crit()).all())),
        Gate("corr", max(zc), z_crit(), max(zc) <= z_crit()),
    ]
