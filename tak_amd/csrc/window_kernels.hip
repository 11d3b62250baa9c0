// window_kernels.hip — device side of the example window (window.hip; the Vec<Example> of training_loop, train/src/main.rs:26,56-123):
// the self-play ring's finished examples enter the window (k_window_absorb), a training chunk leaves it (k_window_gather), both
// without the host in between.  A translation unit of its own: no existing code object changes.
//
// One wave per example in both kernels.  A row is a packed state (256 or 384 bytes), EX_MOVES u16 moves (1024 bytes) and EX_MOVES
// u32 visits (2048 bytes): 16 bytes per lane and request, every row 16-byte aligned (hipMalloc bases, row sizes multiples of 16).
#include "kernels.h"
#include "search.cuh"

namespace tg {

namespace {
constexpr int WAVES = 4;  // per workgroup

__device__ inline void copy_state(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint32_t bytes, int lane) {
    const uint32_t* s = (const uint32_t*)src;
    uint32_t* d = (uint32_t*)dst;
    for (uint32_t j = (uint32_t)lane; j < bytes / 4; j += 64) d[j] = s[j];  // lane-strided dwords: 64 or 96 of them
}
}  // namespace

// Example i of the k that enter: ring row (src0 + i) % max_examples → window row (dst0 + i) % capacity.  The ring keeps whatever an
// earlier example left past n_moves (selfplay.hip, tg_selfplay_drain clears it on the host); a window row is canonical: zero there.
__global__ __launch_bounds__(WAVES * 64) void k_window_absorb(SelfPlayDev P, WindowDev W, uint32_t src0, uint32_t dst0, int k) {
    const int i = (int)(blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (i >= k) return;
    const int lane = threadIdx.x & 63;
    const size_t s = (size_t)((src0 + (uint32_t)i) % (uint32_t)P.max_examples);  // both sums < 2^32: every term < 2^31
    const size_t d = (size_t)((dst0 + (uint32_t)i) % W.capacity);
    const ExampleRec h = P.out_hdr[s];
    const int nm = min(max(h.n_moves, 0), EX_MOVES);
    copy_state(P.out_state + s * W.bytes, W.states + d * W.bytes, W.bytes, lane);
    if (lane == 0) {
        W.n_moves[d] = h.n_moves;
        W.result[d] = h.result;
        W.game_id[d] = h.slot | (h.generation << 20);
    }
    {   // moves: one uint4 = 8 moves per lane
        uint4 v = ((const uint4*)(P.out_moves + s * EX_MOVES))[lane];
        uint32_t c[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4; q++) {
            const int m = lane * 8 + q * 2;  // the dword holds moves m (low half) and m + 1
            c[q] = m + 1 < nm ? c[q] : m < nm ? (c[q] & 0xFFFFu) : 0u;
        }
        ((uint4*)(W.moves + d * EX_MOVES))[lane] = make_uint4(c[0], c[1], c[2], c[3]);
    }
    for (int r = 0; r < 2; r++) {  // visits: two uint4 = 2 × 4 counts per lane
        const int j = r * 64 + lane;
        uint4 v = ((const uint4*)(P.out_visits + s * EX_MOVES))[j];
        uint32_t c[4] = {v.x, v.y, v.z, v.w};
        for (int q = 0; q < 4; q++) c[q] = j * 4 + q < nm ? c[q] : 0u;
        ((uint4*)(W.visits + d * EX_MOVES))[j] = make_uint4(c[0], c[1], c[2], c[3]);
    }
}

// Chunk example i ← window row (row0 + order[i]) % capacity: the rows upload_chunk (train.hip) copies from the host, and the value
// targets of the example's 8 symmetries.  Whole rows: a window row is canonical, as the caller's rows of tg_train are.
__global__ __launch_bounds__(WAVES * 64) void k_window_gather(WindowDev W, uint32_t row0, const int32_t* __restrict__ order, int n,
                                                              uint8_t* __restrict__ states, int32_t* __restrict__ n_moves,
                                                              uint16_t* __restrict__ moves, uint32_t* __restrict__ visits, float* __restrict__ zt) {
    const int i = (int)(blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (i >= n) return;
    const int lane = threadIdx.x & 63;
    const size_t s = (size_t)((row0 + (uint32_t)order[i]) % W.capacity);  // < 2^32: both terms < 2^31
    copy_state(W.states + s * W.bytes, states + (size_t)i * W.bytes, W.bytes, lane);
    if (lane == 0) n_moves[i] = W.n_moves[s];
    if (lane < 8) zt[(size_t)i * 8 + lane] = W.result[s];
    ((uint4*)(moves + (size_t)i * EX_MOVES))[lane] = ((const uint4*)(W.moves + s * EX_MOVES))[lane];
    for (int r = 0; r < 2; r++)
        ((uint4*)(visits + (size_t)i * EX_MOVES))[r * 64 + lane] = ((const uint4*)(W.visits + s * EX_MOVES))[r * 64 + lane];
}

hipError_t launch_window_absorb(hipStream_t st, const SelfPlayDev& P, const WindowDev& W, uint32_t src0, uint32_t dst0, int k) {
    if (k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_window_absorb, dim3((unsigned)((k + WAVES - 1) / WAVES)), dim3(WAVES * 64), 0, st, P, W, src0, dst0, k);
    return hipGetLastError();
}

hipError_t launch_window_gather(hipStream_t st, const WindowDev& W, uint32_t row0, const int32_t* order, int n, uint8_t* states,
                                int32_t* n_moves, uint16_t* moves, uint32_t* visits, float* zt) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_window_gather, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(WAVES * 64), 0, st, W, row0, order, n, states,
                       n_moves, moves, visits, zt);
    return hipGetLastError();
}

}  // namespace tg
