"""The ring arithmetic of the example window and of the self-play ring (tak_amd/csrc/window.h), without a GPU, and the teeth of the
GPU test that compares tg_window_train with tg_train (tests/test_gpu_window.py, test 6).

window.h holds plain host functions, so it is compiled into a program of its own with AddressSanitizer and
UndefinedBehaviorSanitizer (a stand-alone executable: nothing sanitised is loaded into Python) and run once: every (C, first, n) with
C ≤ 9 against a modulo loop, and the ends of the range — C = 2³¹ − 1, first + n passing 2³² and 2⁶⁴."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import window_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tak_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include "window.h"
using namespace tg;
typedef unsigned __int128 u128;
static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)

// the definition: row of cursor position first + i, without overflow
static uint64_t row(uint64_t first, uint64_t i, uint64_t C) { return (uint64_t)(((u128)first + (u128)i) % (u128)C); }

// every row of the range against the modulo loop (n small), and the run structure
static void against_loop(uint64_t C, uint64_t first, uint64_t n) {
    const RingRuns r = ring_runs(first, n, C);
    CHECK(r.count == (n == 0 ? 0 : (first % C) + n > C ? 2 : 1));
    CHECK(r.len[0] + r.len[1] == n && r.at[0] == 0 && r.at[1] == r.len[0] && r.start[1] == 0);
    for (int k = 0; k < 2; k++) CHECK(r.len[k] == 0 || r.start[k] + r.len[k] <= C);
    for (int k = r.count; k < 2; k++) CHECK(r.len[k] == 0);
    uint64_t i = 0;
    for (int k = 0; k < r.count; k++)
        for (uint64_t j = 0; j < r.len[k]; j++, i++) {
            CHECK(r.at[k] + j == i);
            CHECK(r.start[k] + j == row(first, i, C));
            CHECK(ring_row(first, i, C) == row(first, i, C));
        }
    CHECK(i == n);
}

// the same for a range too long to walk: its two ends and the seam
static void at_the_ends(uint64_t C, uint64_t first, uint64_t n) {
    const RingRuns r = ring_runs(first, n, C);
    CHECK(r.count >= 0 && r.len[0] + r.len[1] == n && r.at[1] == r.len[0]);
    if (n == 0) { CHECK(r.count == 0); return; }
    CHECK(r.start[0] == row(first, 0, C) && r.len[0] >= 1 && r.start[0] + r.len[0] <= C);
    CHECK(r.start[0] + r.len[0] - 1 == row(first, r.len[0] - 1, C));
    if (r.len[1]) {
        CHECK(r.count == 2 && r.start[0] + r.len[0] == C);  // the first run ends at the physical end …
        CHECK(row(first, r.len[0], C) == 0 && r.start[1] == 0);  // … and the next row is row 0
        CHECK(r.len[1] - 1 == row(first, n - 1, C) && r.len[1] <= r.start[0]);
    } else CHECK(r.count == 1);
    const uint64_t probe[] = {0, 1, n / 2, n - 1};
    for (uint64_t i : probe) CHECK(ring_row(first, i, C) == row(first, i, C));
}

int main() {
    for (uint64_t C = 1; C <= 9; C++)
        for (uint64_t first = 0; first <= 4 * C + 1; first++)
            for (uint64_t n = 0; n <= C; n++) against_loop(C, first, n);
    // refused: an empty ring, a range longer than the ring
    CHECK(ring_runs(0, 0, 0).count == -1 && ring_runs(3, 10, 9).count == -1 && ring_runs(0, 1ull << 31, (1ull << 31) - 1).count == -1);
    // the largest ring an int capacity allows, cursors around 2^31, 2^32 and 2^64
    const uint64_t C = (1ull << 31) - 1, two32 = 1ull << 32, top = ~0ull;
    const uint64_t firsts[] = {0, 1, C - 1, C, C + 1, two32 - 5, two32 - 1, two32, two32 + 3, 3 * C - 2, top - 9, top - 1, top};
    const uint64_t counts[] = {0, 1, 2, 10, C - 1, C};
    for (uint64_t f : firsts)
        for (uint64_t n : counts) {
            at_the_ends(C, f, n);
            if (n <= 10) against_loop(C, f, n);
        }
    {   // first + n passes 2^32 inside the range: rows follow the 64-bit cursor, not a 32-bit one.  2^32 = 2 (mod C), so the range
        // starts at row C - 3 and wraps the ring after 3 rows
        const RingRuns r = ring_runs(two32 - 5, 10, C);
        CHECK(r.count == 2 && r.start[0] == C - 3 && r.len[0] == 3 && r.start[1] == 0 && r.len[1] == 7);
        against_loop(C, two32 - 5, 10);
        const RingRuns q = ring_runs(two32 - 5 + 100, 10, C);  // ... and the same cursor away from the seam
        CHECK(q.count == 1 && q.start[0] == 97 && q.len[0] == 10);
    }
    for (uint64_t c : {uint64_t(7), uint64_t(48), C})  // small rings under the same cursors
        for (uint64_t f : firsts) against_loop(c, f, c < 10 ? c : 10);
    // more arrive than fit: the oldest are skipped
    CHECK(ring_skip(0, 5) == 0 && ring_skip(5, 5) == 0 && ring_skip(6, 5) == 1 && ring_skip(top, C) == top - C);
    std::printf("ok %ld checks\n", checks);
    return 0;
}
"""


def test_run_splitting_against_a_modulo_loop_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    src, exe = tmp_path / "ring_check.cpp", tmp_path / "ring_check"
    src.write_text(PROGRAM)
    # the sanitisers' runtimes are linked statically: the program brings its own and asks nothing of the loader's environment
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *static,
           "-I", CSRC, str(src), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr)
    assert int(r.stdout.split()[1]) > 10000


def test_window_h_has_no_hip_types():
    import re

    code = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "window.h")).read())
    assert "hip" not in code.lower() and "__device__" not in code and re.findall(r"#include\s*(\S+)", code) == ["<cstdint>"]


# ---- teeth of tests/test_gpu_window.py::test_window_train_is_tg_train ----------------------------------------------------------
@pytest.fixture(scope="module")
def case(orc):
    import eval_examples_ref as ref
    import tak_amd

    ex = ref.make_examples(orc, 5, wr.PUSHED, seed=17)
    assert len(set(ex["states"].tobytes()[i * 256:(i + 1) * 256] for i in range(wr.PUSHED))) == wr.PUSHED  # rows tell examples apart
    return wr.canonical(ex), wr.physical(ex), [tak_amd.train_order(seed, wr.COUNT) for seed in wr.SEEDS]


def test_the_numpy_gather_is_the_shuffled_range(case):
    """gather() against the definition spelled out with plain indexing: chunk example i = pushed example 30 + 3 + order[8k + i]"""
    ex, phys, orders = case
    for order in orders:
        assert sorted(order.tolist()) == list(range(wr.COUNT))
        for k in range(wr.COUNT // wr.CHUNK):
            got = wr.gather(phys, wr.HEAD, wr.FIRST, order, k)
            idx = (wr.PUSHED - wr.CAPACITY) + wr.FIRST + order[k * wr.CHUNK:(k + 1) * wr.CHUNK]
            want = {f: ex[f][idx] for f in ("states", "n_moves", "moves", "visits")}
            want["zt"] = np.repeat(ex["results"][idx], 8)
            assert wr.same(got, want)


@pytest.mark.parametrize("mistake", ["physical_order", "zt_row", "late_wrap"])
def test_each_planted_mistake_changes_a_gathered_chunk_of_both_calls(case, mistake):
    """The GPU test compares training results, which depend on nothing but the chunks' contents: a mistake it must catch has to change
    a chunk the call really trains on (the 5 examples of the remainder are dropped), for BOTH seeds it uses, on its own shapes."""
    _, phys, orders = case
    for order in orders:
        changed = []
        for k in range(wr.COUNT // wr.CHUNK):
            good, bad = wr.gather(phys, wr.HEAD, wr.FIRST, order, k), wr.gather(phys, wr.HEAD, wr.FIRST, order, k, mistake=mistake)
            changed.append(not wr.same(good, bad))
            if mistake == "zt_row":  # … and only the value targets
                assert all(np.array_equal(good[f], bad[f]) for f in ("states", "n_moves", "moves", "visits"))
        assert any(changed), (mistake, changed)
    if mistake == "late_wrap":  # the one row that is read late is row 0 = logical CAPACITY − HEAD − FIRST inside the range: it must be trained on
        for order in orders:
            assert wr.CAPACITY - wr.HEAD - wr.FIRST in order[: wr.COUNT // wr.CHUNK * wr.CHUNK].tolist()
