// window.h — ring arithmetic of the example window (window.hip) and of the self-play example ring (selfplay.hip): where a run of
// consecutive logical rows lives physically.  Plain host functions on integers, no HIP types: tests/test_window_ring.py compiles
// them into a program of its own and checks them against a modulo loop.
//
// A ring of C rows is filled in arrival order: the k-th row that ever entered (k = 0, 1, …, a 64-bit cursor that never wraps in
// practice and is allowed to) lives at physical row k % C.  A range of n ≤ C consecutive rows starting at cursor `first` is therefore
// at most two contiguous physical runs: [first % C, …) up to the physical end, then [0, …).
#pragma once
#include <cstdint>

namespace tg {

struct RingRuns {
    uint64_t start[2];  // physical row of each run
    uint64_t len[2];    // rows of each run; len[0] + len[1] = n, len[1] = 0 when the range does not wrap
    uint64_t at[2];     // position of each run inside the range (at[0] = 0, at[1] = len[0])
    int count;          // runs that hold rows: 0 (n = 0), 1 or 2
};

// physical row of cursor position first + i (the sum may pass 2^64: both terms are reduced first)
inline uint64_t ring_row(uint64_t first, uint64_t i, uint64_t C) {
    const uint64_t a = first % C, b = i % C;
    return a >= C - b ? a - (C - b) : a + b;
}

// the physical runs of the n rows at cursor positions first … first + n − 1.  C > 0 and n ≤ C (a range longer than the ring would
// name a row twice); anything else gives count = −1
inline RingRuns ring_runs(uint64_t first, uint64_t n, uint64_t C) {
    RingRuns r{{0, 0}, {0, 0}, {0, 0}, 0};
    if (C == 0 || n > C) { r.count = -1; return r; }
    const uint64_t o = first % C;
    const uint64_t l0 = n < C - o ? n : C - o;
    r.start[0] = o; r.len[0] = l0; r.at[0] = 0;
    r.start[1] = 0; r.len[1] = n - l0; r.at[1] = l0;
    r.count = n == 0 ? 0 : (r.len[1] ? 2 : 1);
    return r;
}

// of `k` arriving rows only the newest `C` can stay: how many of the oldest are skipped (they count as entered and evicted)
inline uint64_t ring_skip(uint64_t k, uint64_t C) { return k > C ? k - C : 0; }

}  // namespace tg
