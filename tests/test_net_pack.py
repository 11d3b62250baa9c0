"""The weight packers of tak_amd/csrc/net_pack.h on the CPU, element for element.

tests/net_pack_host.cpp (its own main, nothing from HIP) fills tensors from a fixed integer pattern, runs every packer and writes
the results as raw arrays.  It is built twice with the host compiler — plain, and with -fsanitize=address,undefined — and both
programs run as child processes; nothing is loaded into Python.  Each array is compared with a numpy restatement of its layout,
written from the layout's comment (shape by shape, with reshape / transpose where the packer has index arithmetic), never by
calling the code under test.  Teeth: every restatement takes a planted index mistake (`bug=`), and the packer's output must differ
from it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tak_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "net_pack_host.cpp")
f32 = np.float32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def out(request, tmp_path_factory):
    """the directory of raw arrays one build of the program wrote"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("net_pack_" + request.param)
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if request.param == "sanitized" else ["-O2"]
    exe = str(d / "net_pack_host")
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", *flags, "-I" + CSRC, SRC, "-o", exe], check=True)
    os.makedirs(d / "arrays")
    r = subprocess.run([exe, str(d / "arrays")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    return d / "arrays"


def load(out, name, dtype=f32):
    return np.fromfile(str(out / name), dtype=dtype)


# ---- the program's inputs, restated ----
def tensor(count, salt):
    h = (np.arange(count, dtype=np.uint64) * 2654435761 + salt * 40503) & 0xFFFFFFFF
    return ((((h >> 8) & 0xFFFF).astype(np.int64) - 32768) / 256.0).astype(f32)


def folded(O, I, salt):
    return tensor(O * I * 9, salt).reshape(O, I, 9), tensor(O, salt + 1)


# ---- bf16 ----
def bf16(x):
    """round to nearest even; infinities and NaNs truncated"""
    u = np.asarray(x, f32).view(np.uint32).astype(np.uint64)
    rounded = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where((u & 0x7F800000) == 0x7F800000, u >> 16, rounded).astype(np.uint16)


def split(x, bug=None):
    hi = bf16(x)
    with np.errstate(invalid="ignore", over="ignore"):
        lo = bf16(np.asarray(x, f32) - (hi.astype(np.uint32) << 16).view(f32))
    return (lo, hi) if bug == "hi and lo swapped" else (hi, lo)


def test_bf16_rounding_and_split(out):
    x = load(out, "bf16_x")
    assert len(x) == 80
    hi, lo = split(x)
    assert np.array_equal(load(out, "bf16_hi", np.uint16), hi)
    finite = (hi & 0x7F80) != 0x7F80  # (∞ − ∞: the sign of the NaN is the platform's)
    assert finite.sum() >= 75 and np.array_equal(load(out, "bf16_lo", np.uint16)[finite], lo[finite])
    # ties to even, both ways, and a carry into the exponent, spelled out
    assert list(hi[2:7]) == [0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x4000] and hi[7] == 0x7F80 and hi[10] == 0x7FC0
    assert np.any(lo[16:] != 0) and not np.array_equal(load(out, "bf16_hi", np.uint16), split(x, "hi and lo swapped")[0])


def test_padding_rules(out):
    up = lambda v, m: -(-v // m) * m
    want = [up(P, 208) if K % 64 == 0 else up(P, 64) for K in (64, 72, 1600, 2400) for P in (1, 30, 64, 208, 209, 1575)]
    want += [up(v, 112) for v in (0, 1, 63, 64, 65, 1575)]
    assert list(load(out, "padding", np.int32)) == want
    assert want[5] == 1664 and want[23] == 1600  # the policy head of 5×5: K % 64 == 0 → 8 × 208; else 25 × 64


# ---- fold ----
def test_find_and_fold(out):
    O, I = 5, 26
    w, b = tensor(O * I * 9, 1).reshape(O, I * 9), tensor(O, 2)
    g, be, mu, var = tensor(O, 3), tensor(O, 4), tensor(O, 5), np.abs(tensor(O, 6)) + f32(0.5)
    s = g / np.sqrt(var + f32(1e-5))
    assert s.dtype == f32
    assert np.array_equal(load(out, "fold_w"), (w * s[:, None]).ravel())
    assert np.array_equal(load(out, "fold_b"), (b - mu) * s + be)
    assert np.array_equal(load(out, "fold_raw_w"), w.ravel())
    assert not np.array_equal(load(out, "fold_b"), (b - mu) * s + g)  # teeth: γ in β's place
    assert (out / "errors.txt").read_text() == "tensor n.bias has 6 elements, expected 5\nmissing tensor n.running_mean\nmissing tensor d.weight\n"


# ---- convolutions ----
def ref_conv(w, b, Ipad, last_t, bug=None):
    """Wp[(tap·Ipad + c')/16][OP][(tap·Ipad + c')%16]; c' = c but in the last 16-channel chunk, where real channel i sits at
    4·(i / last_t) + i % last_t"""
    O, I, _ = w.shape
    OP = -(-O // 64) * 64
    wp = np.zeros((9 * Ipad // 16, OP, 16), f32)
    for c in range(I):
        cp = c
        if last_t < 4 and c >= Ipad - 16:
            i = c - (Ipad - 16)
            cp = Ipad - 16 + (4 * (i % last_t) + i // last_t if bug == "quad and position exchanged" else 4 * (i // last_t) + i % last_t)
        for tap in range(9):
            k = (cp * 9 + tap) if bug == "channel-major k" else tap * Ipad + cp
            wp[k // 16, :O, k % 16] = w[:, c, tap]
    return wp.ravel(), np.concatenate([b, np.zeros(OP - O, f32)])


@pytest.mark.parametrize("last_t", [4, 3])
def test_conv_f32_layout(out, last_t):
    w, b = folded(5, 26, 10)
    wp, bp = ref_conv(w, b, 32, last_t)
    got = load(out, f"conv_t{last_t}_w")
    assert got.shape == (9 * 32 * 64,) and np.array_equal(got, wp)
    assert np.array_equal(load(out, f"conv_t{last_t}_b"), bp)
    assert not np.array_equal(got, ref_conv(w, b, 32, last_t, "channel-major k")[0])
    if last_t == 3:
        assert not np.array_equal(got, ref_conv(w, b, 32, 3, "quad and position exchanged")[0])
        assert not np.array_equal(got, load(out, "conv_t4_w"))


def ref_conv_s3(w, KC, OP, bug=None):
    """[chunk = tap·KC + kc][cout tile][hi|lo][q][cout in tile][8 bf16], channel = 32·kc + 8q + j; of every 32 output channels,
    channel 8q' + 4t + i goes to row 4q' + i of the pair's tile t"""
    O, I, _ = w.shape
    hi, lo = split(w, "hi and lo swapped" if bug == "hi and lo swapped" else None)
    r = np.zeros((9, KC, OP // 16, 2, 4, 16, 8), np.uint16)
    for o in range(O):
        qq, t, i = (o % 32) // 8, (o % 8) // 4, o % 4
        tile, row = (o // 32) * 2 + t, 4 * qq + i
        if bug == "no row interleave":
            tile, row = o // 16, o % 16
        for c in range(I):
            kc, q, j = c // 32, (c % 32) // 8, c % 8
            if bug == "q and j exchanged":
                q, j = (c % 32) % 4, (c % 32) // 4
            r[:, kc, tile, 0, q, row, j] = hi[o, c]
            r[:, kc, tile, 1, q, row, j] = lo[o, c]
    return r.ravel()


@pytest.mark.parametrize("O,OP,salt", [(64, 64, 20), (36, 64, 22)])
def test_conv_split_layout(out, O, OP, salt):
    w, _ = folded(O, 40, salt)
    got = load(out, f"conv_s3_{O}", np.uint16)
    assert got.shape == (9 * 2 * OP * 64,) and np.array_equal(got, ref_conv_s3(w, 2, OP))
    for bug in ("hi and lo swapped", "no row interleave", "q and j exchanged"):
        assert not np.array_equal(got, ref_conv_s3(w, 2, OP, bug)), bug


# ---- constant planes as a bias ----
def ref_cplane_sums(w, bc, bug=None):
    """S[plane − bc][border class = 3·cy + cx][O]: the taps (dy, dx) that stay on the board, summed in tap order in f32;
    cy / cx 0: first row / column (no dy / dx = −1), 2: last (no +1)"""
    O, I, _ = w.shape
    S = np.zeros((I - bc, 9, O), f32)
    for cls in range(9):
        cy, cx = (cls % 3, cls // 3) if bug == "cy and cx exchanged" else (cls // 3, cls % 3)
        for tap in range(9):
            dy, dx = tap // 3 - 1, tap % 3 - 1
            if (cy == 0 and dy < 0) or (cy == 2 and dy > 0) or (cx == 0 and dx < 0) or (cx == 2 and dx > 0):
                continue
            S[:, cls, :] = S[:, cls, :] + w[:, bc:, tap].T
    return S


def test_board_restriction_and_constant_plane_sums(out):
    w, b = folded(3, 7, 30)
    assert np.array_equal(load(out, "board_w"), w[:, :2].ravel()) and np.array_equal(load(out, "board_b"), b)
    assert not np.array_equal(load(out, "board_w"), w[:, 5:].ravel())  # teeth: the last planes
    S = ref_cplane_sums(w, 2)
    assert all(len(set(S[pl, :, o])) == 9 for pl in range(5) for o in range(3)), "every border class a different sum"
    got = load(out, "cplane_sums")
    assert got.shape == (5 * 9 * 3,) and np.array_equal(got, S.ravel())
    assert not np.array_equal(got, ref_cplane_sums(w, 2, "cy and cx exchanged").ravel())
    assert not np.array_equal(got, S.transpose(0, 2, 1).ravel())  # teeth: [plane][O][class]


# ---- the policy FC ----
def fc_columns(F, nsq, P, NP, salt, bug=None):
    """A[column][k = sq·F + c] from policy.weight [P, c·nsq + sq] and — where NP > P — value.weight as column P; bias padded to NP"""
    K = F * nsq
    w, b, wv, bv = tensor(P * K, salt).reshape(P, F, nsq), tensor(P, salt + 1), tensor(K, salt + 2).reshape(1, F, nsq), tensor(1, salt + 3)
    A = np.zeros((P + 1 if NP > P else P, K), f32)
    bias = np.zeros(NP, f32)
    A[:P] = (w if bug == "NCHW order kept" else w.transpose(0, 2, 1)).reshape(P, K)
    bias[:P] = b
    if NP > P:
        at = P - 1 if bug == "value column one to the left" else P
        A[at], bias[at] = wv.transpose(0, 2, 1).reshape(K), bv[0]
    return A, bias


def ref_fc(A, NP):
    """Wp[K/16][NP][16], whole chunks, zero padded"""
    cols, K = A.shape
    chunks = -(-K // 16)
    Ap = np.zeros((NP, chunks * 16), f32)
    Ap[:cols, :K] = A
    return Ap.reshape(NP, chunks, 16).transpose(1, 0, 2)


def ref_fc_lanes(Wp, bug=None):
    """per (chunk, tile of 16 columns): slot q·16 + r holds the 4 floats k = 16·chunk + 4q … 4q + 3 of column 16·tile + r"""
    chunks, NP, _ = Wp.shape
    blocks = Wp.reshape(chunks, NP // 16, 16, 4, 4)  # [chunk][tile][r][q][u]
    return (blocks if bug == "q and r exchanged" else blocks.transpose(0, 1, 3, 2, 4)).ravel()


@pytest.mark.parametrize("tag,F,nsq,P,NP,salt", [("fc_k64_p30", 16, 4, 30, 208, 40), ("fc_k72_p30", 8, 9, 30, 64, 44), ("fc_k72_p64", 8, 9, 64, 64, 48)])
def test_fc_f32_layouts(out, tag, F, nsq, P, NP, salt):
    assert list(load(out, tag + "_np", np.int32)) == [NP, P + (NP > P)]
    A, bias = fc_columns(F, nsq, P, NP, salt)
    Wp = ref_fc(A, NP)
    got, lanes = load(out, tag + "_w"), load(out, tag + "_lanes")
    assert got.shape == Wp.ravel().shape and np.array_equal(got, Wp.ravel())
    assert np.array_equal(load(out, tag + "_b"), bias)
    assert np.array_equal(lanes, ref_fc_lanes(Wp))
    assert not np.array_equal(lanes, ref_fc_lanes(Wp, "q and r exchanged"))
    assert not np.array_equal(got, ref_fc(fc_columns(F, nsq, P, NP, salt, "NCHW order kept")[0], NP).ravel())
    assert not np.array_equal(got, Wp.transpose(1, 0, 2).ravel())  # teeth: [NP][K/16][16]
    if NP > P:
        Ab, bb = fc_columns(F, nsq, P, NP, salt, "value column one to the left")
        assert not np.array_equal(got, ref_fc(Ab, NP).ravel()) and not np.array_equal(load(out, tag + "_b"), bb)
        assert np.any(Wp[:, P, :] != 0) and not np.any(Wp[:, P + 1 :, :])
    else:
        assert np.array_equal(Wp[:, :P, :].ravel(), got)  # no column beyond the policy's


def ref_fc_s3(A, NP, CB, bug=None):
    """[chunk of 32 k][NP / CB column blocks][q][hi|lo][column in block][8 bf16], k = 32·chunk + 8q + j"""
    cols, K = A.shape
    hi, lo = split(A, "hi and lo swapped" if bug == "hi and lo swapped" else None)
    r = np.zeros((K // 32, NP // CB, 4, 2, CB, 8), np.uint16)
    for o in range(cols):
        r[:, o // CB, :, 0, o % CB, :] = hi[o].reshape(K // 32, 4, 8)
        r[:, o // CB, :, 1, o % CB, :] = lo[o].reshape(K // 32, 4, 8)
    return (r.transpose(0, 1, 3, 2, 4, 5) if bug == "q and half exchanged" else r).ravel()


def ref_fc_s3_ring(A, tiles, bug=None):
    """[chunk of 32 k][tile][hi|lo][lane = q·16 + column in tile][8 bf16]"""
    cols, K = A.shape
    hi, lo = split(A, "hi and lo swapped" if bug == "hi and lo swapped" else None)
    r = np.zeros((K // 32, tiles, 2, 4, 16, 8), np.uint16)
    for o in range(cols):
        r[:, o // 16, 0, :, o % 16, :] = hi[o].reshape(K // 32, 4, 8)
        r[:, o // 16, 1, :, o % 16, :] = lo[o].reshape(K // 32, 4, 8)
    return (r.transpose(0, 1, 2, 4, 3, 5) if bug == "lane = column·4 + q" else r).ravel()


@pytest.mark.parametrize("tag,P", [("s3_p100", 100), ("s3_p112", 112)])
def test_fc_split_layouts(out, tag, P):
    F, nsq, NP, CB, salt = 16, 4, 112, 112, 52 if P == 100 else 56
    A, bias = fc_columns(F, nsq, P, NP, salt)
    assert A.shape[0] == (101 if P == 100 else 112)
    got = load(out, tag + "_w", np.uint16)
    assert got.shape == (2 * NP * 64,) and np.array_equal(got, ref_fc_s3(A, NP, CB))
    assert np.array_equal(load(out, tag + "_b"), bias)
    for bug in ("hi and lo swapped", "q and half exchanged"):
        assert not np.array_equal(got, ref_fc_s3(A, NP, CB, bug)), bug
    if P == 100:
        Ab, _ = fc_columns(F, nsq, P, NP, salt, "value column one to the left")
        assert not np.array_equal(got, ref_fc_s3(Ab, NP, CB))
        ring = load(out, tag + "_ring", np.uint16)
        assert ring.shape == (2 * 8 * 2 * 64 * 8,) and np.array_equal(ring, ref_fc_s3_ring(A, 8))
        for bug in ("hi and lo swapped", "lane = column·4 + q"):
            assert not np.array_equal(ring, ref_fc_s3_ring(A, 8, bug)), bug
        assert not np.array_equal(ring, ref_fc_s3_ring(Ab, 8))
    else:
        assert not (out / (tag + "_ring")).exists()


def test_value_weights_in_nhwc_order(out):
    wv = tensor(64, 60).reshape(16, 4)  # [c][sq]
    assert np.array_equal(load(out, "value_w"), wv.T.ravel())
    assert not np.array_equal(load(out, "value_w"), wv.ravel())
