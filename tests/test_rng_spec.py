"""The self-play randomness against references outside the engine / oracle pair (tests/rng_ref.py), on the CPU.

tak_amd/csrc/rng.cuh itself — included, not copied — is compiled for the host with the flags both Makefiles use
(-ffp-contract=off) behind a two-line stand-in for hip/hip_runtime.h, and asked three questions the oracle, a second statement of the
same specification by the same hand, cannot answer: is it Philox (Random123's known answers, an independent Python Philox), is the
noise Dirichlet(α) (Kolmogorov–Smirnov against scipy's Gamma and Beta, moments, correlations), is a move picked in proportion to
its visits (χ² against visits / Σ visits; the big-integer rule).  The det_* helpers are held to libm.

The teeth are in the same file: the gates, at the same sample sizes, reject numpy-made samples of six deliberately wrong samplers
and accept numpy's own gamma / dirichlet under 20 seeds.  Measured values: profiles/r15_a_rng_gates.txt."""
import ctypes as C
import importlib.util
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import rng_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.environ.get("TG_RNG_SPEC_CSRC") or os.path.join(ROOT, "tak_amd", "csrc")  # (a scratch copy with a planted mistake)
SEED_HI = 0x9E3779B97F4A7C15  # a seed whose upper half is not 0

SHIM = r"""
#include <stddef.h>
#include "rng.cuh"
using namespace tg;
extern "C" {
void h_philox(int n, const uint64_t* seed, const uint32_t* c, uint32_t* out) {
    for (int i = 0; i < n; i++) {
        U4 r = philox4x32_10(seed[i], c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
        for (int k = 0; k < 4; k++) out[4 * i + k] = r.v[k];
    }
}
void h_rng_draw(int n, const uint64_t* seed, const uint32_t* f, uint32_t* out) {
    for (int i = 0; i < n; i++) {
        U4 r = rng_draw(seed[i], f[6 * i], f[6 * i + 1], f[6 * i + 2], f[6 * i + 3], f[6 * i + 4], f[6 * i + 5]);
        for (int k = 0; k < 4; k++) out[4 * i + k] = r.v[k];
    }
}
void h_det(int which, int n, const double* x, double* y) {
    for (int i = 0; i < n; i++) y[i] = which == 0 ? det_log(x[i]) : which == 1 ? det_exp(x[i]) : det_sqrt(x[i]);
}
double h_u32_unit(uint32_t x) { return u32_unit(x); }
void h_gamma(double alpha, uint64_t seed, uint32_t generation, uint32_t ply, uint32_t slot0, int slots, int indices, double* out) {
    for (int s = 0; s < slots; s++)
        for (int i = 0; i < indices; i++) out[(size_t)s * indices + i] = gamma_sample(alpha, seed, slot0 + (uint32_t)s, generation, ply, (uint32_t)i);
}
// how many draws the rejection loop of gamma_sample used: every draw whose first two words lie inside the unit disc gives a normal x
// through rng.cuh's own helpers; the draw that gamma_sample returned from is the first whose d·v (· boost) is its result
long long h_gamma_draws(double alpha, uint64_t seed, uint32_t generation, uint32_t ply, uint32_t slot0, int slots, int indices, const double* got) {
    long long draws = 0;
    double a = alpha < 1.0 ? alpha + 1.0 : alpha, d = a - 1.0 / 3.0, c = 1.0 / det_sqrt(9.0 * d);
    for (int s = 0; s < slots; s++)
        for (int i = 0; i < indices; i++) {
            uint32_t at = 0;
            for (; at < 65535; at++) {
                U4 r = rng_draw(seed, slot0 + (uint32_t)s, generation, ply, RNG_GAMMA, (uint32_t)i, at);
                double v1 = 2.0 * u32_unit(r.v[0]) - 1.0, v2 = 2.0 * u32_unit(r.v[1]) - 1.0, q = v1 * v1 + v2 * v2;
                if (q >= 1.0 || q == 0.0) continue;
                double w = 1.0 + c * (v1 * det_sqrt(-2.0 * det_log(q) / q)), g = d * (w * w * w);
                if (alpha < 1.0) g = g * det_exp(det_log(u32_unit(r.v[3])) / alpha);
                if (g == got[(size_t)s * indices + i]) break;
            }
            if (at == 65535) return -1;
            draws += at + 1;
        }
    return draws;
}
}
"""


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """rng.cuh compiled for the host: ctypes handle"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("rng_host")
    os.makedirs(d / "hip")
    (d / "hip" / "hip_runtime.h").write_text("#define __host__\n#define __device__\n")
    (d / "shim.cpp").write_text(SHIM)
    so = str(d / "librng_host.so")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared", "-I" + str(d), "-I" + CSRC, str(d / "shim.cpp"), "-o", so],
                   check=True)
    l = C.CDLL(so)
    l.h_u32_unit.restype = C.c_double
    l.h_u32_unit.argtypes = [C.c_uint32]
    l.h_gamma.argtypes = [C.c_double, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_void_p]
    l.h_gamma_draws.argtypes = l.h_gamma.argtypes
    l.h_gamma_draws.restype = C.c_longlong
    return l


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _philox(host, seeds, ctrs):
    seeds, ctrs = np.ascontiguousarray(seeds, np.uint64), np.ascontiguousarray(ctrs, np.uint32)
    out = np.zeros((len(seeds), 4), np.uint32)
    host.h_philox(len(seeds), _p(seeds), _p(ctrs), _p(out))
    return out


def _draw(host, seeds, fields):
    seeds, fields = np.ascontiguousarray(seeds, np.uint64), np.ascontiguousarray(fields, np.uint32)
    out = np.zeros((len(seeds), 4), np.uint32)
    host.h_rng_draw(len(seeds), _p(seeds), _p(fields), _p(out))
    return out


def _det(host, which, x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    host.h_det(which, len(x), _p(x), _p(y))
    return y


def _gamma(host, alpha, seed=SEED_HI, generation=1, ply=7, slot0=4000, slots=2048, indices=512, draws=False):
    out = np.zeros(slots * indices, np.float64)
    host.h_gamma(alpha, seed, generation, ply, slot0, slots, indices, _p(out))
    if not draws:
        return out
    return out, int(host.h_gamma_draws(alpha, seed, generation, ply, slot0, slots, indices, _p(out)))


HAVE_SCIPY = importlib.util.find_spec("scipy") is not None
requires_scipy = pytest.mark.skipif(not HAVE_SCIPY, reason="scipy is not installed: no CDF to gate against")


# ---- is it Philox? ------------------------------------------------------------------------------------------------------------------

def test_philox_known_answers(host, orc):
    """Random123's vectors, through rng.cuh, the oracle and rng_ref's two statements"""
    for ctr, key, want in R.KATS:
        seed = key[0] | (key[1] << 32)
        assert R.philox_ctr_key(ctr, key) == want
        assert tuple(int(v) for v in R.philox_np(seed, *ctr)) == want
        assert tuple(int(v) for v in _philox(host, [seed], [ctr])[0]) == want, "rng.cuh is not Philox4x32-10"
        assert tuple(int(v) for v in orc.philox(seed, *ctr)) == want, "the oracle is not Philox4x32-10"


def test_philox_on_random_tuples_with_the_upper_key_half_in_use(host, orc):
    rng = np.random.default_rng(1)
    n = 4096
    seeds = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    seeds[:64] |= np.uint64(0xFFFFFFFF00000000)  # every bit of the upper half set
    seeds[64:96] = np.uint64(1) << np.arange(32, 64, dtype=np.uint64)  # each bit of the upper half alone
    seeds[96:128] &= np.uint64(0xFFFFFFFF)  # and the upper half 0, as every older test has it
    ctrs = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint32)
    got = _philox(host, seeds, ctrs)
    assert np.array_equal(got, R.philox_np(seeds, ctrs[:, 0], ctrs[:, 1], ctrs[:, 2], ctrs[:, 3]))
    for i in range(n):
        s, c = int(seeds[i]), [int(v) for v in ctrs[i]]
        assert tuple(int(v) for v in got[i]) == R.philox(s, *c), (hex(s), c)
        assert np.array_equal(got[i], orc.philox(s, *c)), (hex(s), c)
    # the upper half is part of the key: the same counters under seeds that differ only there
    lo = seeds & np.uint64(0xFFFFFFFF)
    assert not (_philox(host, lo, ctrs) == got)[seeds != lo].all(1).any()


FIELD_MAX = dict(slot=0xFFFFFFFF, generation=0xFFFFFFFF, ply=65535, purpose=65535, index=65535, attempt=65534)


def test_rng_draw_streams(host):
    """every field of the key at 0 and at its largest packed value; changing exactly one field by one gives another output, and
    rng.cuh packs the counter as DESIGN.md words it (rng_ref.rng_draw)"""
    names = list(FIELD_MAX)
    points = []
    for corner in range(1 << 6):
        base = [FIELD_MAX[f] if corner >> b & 1 else 0 for b, f in enumerate(names)]
        points.append(tuple(base))
        for b in range(6):
            nb = list(base)
            nb[b] += -1 if base[b] else 1
            points.append(tuple(nb))
    points = sorted(set(points))
    fields = np.array(points, np.uint64).astype(np.uint32)
    for seed in (3, SEED_HI):
        got = _draw(host, np.full(len(points), seed, np.uint64), fields)
        for p, g in zip(points[::7], got[::7]):
            assert tuple(int(v) for v in g) == R.rng_draw(seed, *p), p
        assert np.array_equal(got, R.rng_draw_np(seed, *[fields[:, b] for b in range(6)]))
        rows = {p: tuple(g) for p, g in zip(points, got)}
        assert len(set(rows.values())) == len(points), "two keys that differ in one field share an output"
        for p in points:  # not even one of the four words is shared between a key and its neighbour in one field
            for b in range(6):
                nb = tuple(v + (i == b) for i, v in enumerate(p))
                if nb in rows:
                    assert not any(x == y for x, y in zip(rows[p], rows[nb])), (p, nb)


# ---- det_* against libm -------------------------------------------------------------------------------------------------------------

ULP16 = 16 * 2.0 ** -52  # 3.6e-15: the spec fixes + − × ÷ sequences, not correctly rounded results; a slipped constant or a missing
#                          Newton step costs ≥ 1e-10, and no f32 noise value can see 16 ulp of f64


def _rel(got, want):
    return float(np.max(np.abs(got - want) / np.abs(want)))


def test_det_log_against_libm(host):
    rng = np.random.default_rng(2)
    u = (rng.integers(0, 1 << 32, 1 << 18).astype(np.float64) + 0.5) / 4294967296.0  # u32_unit's values
    edge = np.array([host.h_u32_unit(0), host.h_u32_unit(1), host.h_u32_unit(0xFFFFFFFF), 2.0 ** -33, 8.0, 0.5, 2.0, math.sqrt(2.0)])
    assert edge[0] == 2.0 ** -33 and edge[2] == 1.0 - 2.0 ** -33
    x = np.concatenate([u, edge, np.exp(rng.uniform(math.log(2.0 ** -33), math.log(8.0), 1 << 18)),  # (2⁻³³, 8]: u and the disc's s
                        np.exp(rng.uniform(math.log(1e-6), math.log(2.0), 1 << 18)) ** 3,  # v = w³ for w down to 1e-6
                        1.0 + rng.uniform(-1e-3, 1e-3, 1 << 16), 1.0 + rng.uniform(-1.0, 1.0, 1 << 10) * 1e-9])
    x = x[x != 1.0]
    err = _rel(_det(host, 0, x), np.log(x))
    print(f"rng-gate det_log: worst relative error {err:.3e} over {len(x)} arguments (bound {ULP16:.3e})")
    assert _det(host, 0, np.array([1.0]))[0] == 0.0
    assert err <= ULP16


def test_det_exp_against_libm(host):
    rng = np.random.default_rng(3)
    y = np.concatenate([rng.uniform(-700.0, 0.0, 1 << 18), -np.exp(rng.uniform(math.log(1e-12), math.log(700.0), 1 << 18)),
                        np.array([0.0, -700.0, -1e-300, -0.5 * math.log(2.0), -math.log(2.0)]),
                        np.log((rng.integers(0, 1 << 32, 1 << 16).astype(np.float64) + 0.5) / 4294967296.0) / 0.2])  # the boost's own arguments
    y = y[y >= -700.0]
    err = _rel(_det(host, 1, y), np.exp(y))
    print(f"rng-gate det_exp: worst relative error {err:.3e} over {len(y)} arguments (bound {ULP16:.3e})")
    assert err <= ULP16
    # below −700 the spec returns 0 where the true value is under 1e-304: the boost of u32_unit(0) at α = 0.03 is such an argument
    far = _det(host, 0, np.array([host.h_u32_unit(0)]))[0] / 0.03
    assert far < -700.0 and math.exp(-700.0) < 1e-304
    assert (_det(host, 1, np.array([far, np.nextafter(-700.0, -np.inf), -1e4])) == 0.0).all()


def test_det_sqrt_against_libm(host):
    rng = np.random.default_rng(4)
    a = np.concatenate([np.exp(rng.uniform(math.log(1e-12), math.log(1e3), 1 << 19)), np.array([1e-12, 1e3, 1.0, 2.0, 4.0, 9.0 * (1.2 - 1.0 / 3.0)])])
    err = _rel(_det(host, 2, a), np.sqrt(a))
    print(f"rng-gate det_sqrt: worst relative error {err:.3e} over {len(a)} arguments (bound {ULP16:.3e})")
    assert err <= ULP16


# ---- is the noise Dirichlet(α)? -----------------------------------------------------------------------------------------------------

@requires_scipy
@pytest.mark.parametrize("alpha", [0.2, 1.0, 3.0])
def test_gamma_sample_law(host, alpha):
    """2²⁰ draws of gamma_sample — indices 0 … 511 of 2048 slots, the way k_dirichlet walks them — are Gamma(α, 1)"""
    x, draws = _gamma(host, alpha, draws=True)
    assert len(x) == 1 << 20
    gates = R.gamma_law_gates(x, alpha)
    R.report(f"gamma_sample alpha={alpha} n=2^20", gates)
    assert not R.failed(gates), gates
    assert draws >= len(x), "the shim's count of the rejection loop's draws no longer follows gamma_sample"
    print(f"rng-gate gamma_sample alpha={alpha}: {len(x) / draws:.4f} of the draws are accepted ({draws} draws)")
    # with the upper key half dropped the draws would be another seed's: the streams differ
    assert not np.array_equal(_gamma(host, alpha, slots=1), _gamma(host, alpha, seed=SEED_HI & 0xFFFFFFFF, slots=1))


def _noise(orc, alpha, k, games, seed=SEED_HI, slot0=5000, generation=2, ply=9):
    return np.stack([orc.dirichlet(k, alpha, seed, slot0 + g, generation, ply) for g in range(games)])


@requires_scipy
@pytest.mark.parametrize("k", [3, 23, 150])
@pytest.mark.parametrize("alpha", [0.2, 1.0])
def test_noise_law(orc, alpha, k):
    rows = _noise(orc, alpha, k, 4096)
    assert rows.dtype == np.float32
    gates = R.dirichlet_law_gates(rows, alpha)
    R.report(f"noise alpha={alpha} K={k} games=4096", gates)
    assert not R.failed(gates), gates


def test_noise_is_the_normalised_gamma_sample_of_rng_cuh(host, orc):
    """what ties the two law tests together: the oracle's noise is rng.cuh's gamma_sample divided by its sum in child order"""
    for alpha, k in ((0.2, 150), (3.0, 23), (0.03, 70)):
        g = _gamma(host, alpha, seed=SEED_HI, generation=2, ply=9, slot0=5001, slots=1, indices=k)
        total = 0.0
        for v in g:
            total += v
        assert total > 0
        assert np.array_equal((g / total).astype(np.float32).view(np.uint32), orc.dirichlet(k, alpha, SEED_HI, 5001, 2, 9).view(np.uint32))


# ---- teeth --------------------------------------------------------------------------------------------------------------------------

def mt_gamma(rng, alpha, n, d_off=1.0 / 3.0, polar_div=True, boost="1/alpha"):
    """Marsaglia–Tsang as DESIGN.md §RNG words it, in numpy with libm, with one knob per planted mistake"""
    a = alpha + 1.0 if alpha < 1.0 else alpha
    d = a - d_off
    c = 1.0 / math.sqrt(9.0 * d)
    out = np.zeros(0)
    while len(out) < n:
        m = 2 * (n - len(out)) + 1024
        v1, v2, u, ub = rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), rng.uniform(0, 1, m), rng.uniform(0, 1, m)
        s = v1 * v1 + v2 * v2
        ok = (s < 1.0) & (s > 0.0)
        v1, s, u, ub = v1[ok], s[ok], u[ok], ub[ok]
        x = v1 * np.sqrt(-2.0 * np.log(s) / s) if polar_div else v1 * np.sqrt(-2.0 * np.log(s))
        w = 1.0 + c * x
        ok = w > 0.0
        x, w, u, ub = x[ok], w[ok], u[ok], ub[ok]
        v = w ** 3
        ok = np.log(u) < 0.5 * x * x + d - d * v + d * np.log(v)
        g = d * v[ok]
        if alpha < 1.0 and boost == "1/alpha":
            g = g * ub[ok] ** (1.0 / alpha)
        elif alpha < 1.0 and boost == "1/(alpha+1)":
            g = g * ub[ok] ** (1.0 / (alpha + 1.0))
        out = np.concatenate([out, g])
    return out[:n]


# mistake → (sampler knobs or None, the alphas it shows at, the gate that must reject it)
GAMMA_MISTAKES = {
    "boost left out": (dict(boost="none"), (0.2,), "ks"),
    "boost exponent 1/(alpha+1)": (dict(boost="1/(alpha+1)"), (0.2,), "ks"),
    "d = a - 1/2": (dict(d_off=0.5), (0.2, 1.0, 3.0), "ks"),
    "polar normal without / s": (dict(polar_div=False), (0.2, 1.0, 3.0), "ks"),
    "alpha doubled": (None, (0.2, 1.0, 3.0), "ks"),
}
N_GAMMA = 1 << 20


@requires_scipy
def test_gates_accept_a_correct_marsaglia_tsang():
    """mt_gamma with every knob at its right value passes: the mistakes below are then one knob each"""
    for alpha in (0.2, 1.0, 3.0):
        gates = R.gamma_law_gates(mt_gamma(np.random.default_rng(11), alpha, N_GAMMA), alpha)
        assert not R.failed(gates), (alpha, gates)


@requires_scipy
@pytest.mark.parametrize("mistake", list(GAMMA_MISTAKES))
def test_gamma_gates_reject(mistake):
    knobs, alphas, gate = GAMMA_MISTAKES[mistake]
    for alpha in alphas:
        rng = np.random.default_rng(12)
        x = rng.gamma(2.0 * alpha, size=N_GAMMA) if knobs is None else mt_gamma(rng, alpha, N_GAMMA, **knobs)
        gates = R.gamma_law_gates(x, alpha)
        R.report(f"WRONG gamma ({mistake}) alpha={alpha} n=2^20", gates)
        assert gate in R.failed(gates), (mistake, alpha, gates)


@requires_scipy
@pytest.mark.slow
def test_gates_accept_numpy_under_20_seeds():
    """the reference alone stays within every gate: numpy's gamma at n = 2²⁰ and numpy's dirichlet at 4096 games, 20 seeds each"""
    worst = {}
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        for alpha in (0.2, 1.0, 3.0):
            gates = R.gamma_law_gates(rng.gamma(alpha, size=N_GAMMA), alpha)
            assert not R.failed(gates), (seed, alpha, gates)
            for g in gates:
                worst[("gamma", g.name)] = max(worst.get(("gamma", g.name), 0.0), g.value / g.bound if g.bound else 0.0)
        for alpha in (0.2, 1.0):
            for k in (3, 23, 70, 150):
                gates = R.dirichlet_law_gates(rng.dirichlet([alpha] * k, 4096).astype(np.float32), alpha)
                assert not R.failed(gates), (seed, alpha, k, gates)
                for g in gates:
                    worst[("dirichlet", g.name)] = max(worst.get(("dirichlet", g.name), 0.0), g.value / g.bound)
    for key, v in sorted(worst.items()):
        print(f"rng-gate numpy x 20 seeds: {key[0]:9s} {key[1]:9s} worst value / bound {v:.3f}")


@requires_scipy
def test_noise_gates_reject():
    """noise normalised by the sum of its first 64 components only: the same vector for K ≤ 64 — invisible there by construction,
    asserted — and rejected at K = 150 by the row sums (and by the Kolmogorov–Smirnov distance of the too large components);
    alpha doubled: rejected by the Kolmogorov–Smirnov gate at every K"""
    for alpha in (0.2, 1.0):
        for k in (3, 23, 150):
            rng = np.random.default_rng(13)
            g = rng.gamma(alpha, size=(4096, k))
            first64 = (g / g[:, :64].sum(1, keepdims=True)).astype(np.float32)
            gates = R.dirichlet_law_gates(first64, alpha)
            R.report(f"WRONG noise (sum of the first 64) alpha={alpha} K={k}", gates)
            if k <= 64:
                assert np.array_equal(first64, (g / g.sum(1, keepdims=True)).astype(np.float32)) and not R.failed(gates)
            else:
                assert {"rowsum", "ks"} <= set(R.failed(gates)), gates
            gates = R.dirichlet_law_gates(rng.dirichlet([2.0 * alpha] * k, 4096).astype(np.float32), alpha)
            R.report(f"WRONG noise (alpha doubled) alpha={alpha} K={k}", gates)
            assert "ks" in R.failed(gates), gates


# ---- is a move picked in proportion to its visits? ----------------------------------------------------------------------------------

def _visit_vectors():
    rng = np.random.default_rng(5)
    flat = np.full(23, 7, np.uint32)
    holes = rng.integers(1, 40, 69).astype(np.uint32)
    holes[[0, 1, 30, 31, 32, 67, 68]] = 0  # zeros at both ends and in the middle
    big = rng.integers(0, 1 << 26, 200).astype(np.uint32)  # 200 children, total > 2³²
    big[[0, 50, 199]] = 0
    big[7] = 0xFFFFFFFF
    assert int(big.astype(np.uint64).sum()) > 1 << 32
    return {"flat": flat, "holes": holes, "big": big}


@pytest.mark.parametrize("name", ["flat", "holes", "big"])
def test_pick_rule(orc, name):
    """the oracle's pick_move equals the big-integer rule, and over 2¹⁶ slots its picks follow visits / Σ visits"""
    visits = _visit_vectors()[name]
    slots, gen, ply, slot0 = 1 << 16, 3, 11, 70000
    words = R.rng_draw_np(SEED_HI, slot0 + np.arange(slots, dtype=np.uint64), gen, ply, R.RNG_PICK, 0, 0)
    got = np.array([orc.pick_move(visits, False, SEED_HI, slot0 + s, gen, ply) for s in range(slots)])
    want = np.array([R.pick_from_words(words[s, 0], words[s, 1], visits) for s in range(slots)])
    assert np.array_equal(got, want)
    for s in range(0, slots, 4099):
        assert R.pick(SEED_HI, slot0 + s, gen, ply, visits) == got[s]
    counts = np.bincount(got, minlength=len(visits))
    assert not counts[visits == 0].any(), "a child without visits was picked"
    if HAVE_SCIPY:
        total = float(visits.astype(np.uint64).sum())
        gate = R.chi2_gate("pick", counts, slots * visits.astype(np.float64) / total)
        R.report(f"pick {name} slots=2^16", [gate])
        assert gate.ok, gate
    # the extremes of the draw: x = 0 takes the first child with visits, x = 2⁶⁴ − 1 the last one
    nz = np.nonzero(visits)[0]
    assert R.pick_from_words(0, 0, visits) == nz[0] and R.pick_from_words(R.M32, R.M32, visits) == nz[-1]


@requires_scipy
def test_pick_gate_rejects_a_32_bit_total():
    """teeth of the χ² gate at this size: the pick with Σ visits truncated to 32 bits (the 200-children vector's total is above 2³²)"""
    visits = _visit_vectors()["big"]
    slots = 1 << 16
    words = R.rng_draw_np(SEED_HI, 70000 + np.arange(slots, dtype=np.uint64), 3, 11, R.RNG_PICK, 0, 0)
    total = int(visits.astype(np.uint64).sum())
    cum = np.cumsum(visits.astype(np.uint64))
    wrong = np.zeros(slots, np.int64)
    for s in range(slots):
        target = (((int(words[s, 0]) << 32) | int(words[s, 1])) * (total & R.M32)) >> 64
        wrong[s] = int(np.searchsorted(cum, target, "right"))
    gate = R.chi2_gate("pick", np.bincount(wrong, minlength=len(visits)), slots * visits.astype(np.float64) / total)
    R.report("WRONG pick (32-bit total) big slots=2^16", [gate])
    assert not gate.ok
