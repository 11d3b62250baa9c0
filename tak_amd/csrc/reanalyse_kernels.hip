// reanalyse_kernels.hip — device side of tg_reanalyse (reanalyse.hip): the two ends of the path between the example window and the
// lock-step search.  k_reanalyse_roots makes a slice of window rows the roots of the search object's slots, k_reanalyse_store writes
// the searched roots' visit counts (Node::improved_policy, alpha-tak/src/search/play.rs:13-21) back into those rows.  No counterpart
// in the reference, which retrains on the targets an example was born with (train/src/main.rs:82-95).  A translation unit of its
// own: no existing code object changes.
//
// As window_kernels.hip: one wave per row / slot, 4 waves per workgroup, 16 bytes per lane and request for the rows, lane-strided
// dwords for the state.
#include "kernels.h"
#include "search.cuh"

namespace tg {

namespace {
constexpr int WAVES = 4;  // per workgroup
}  // namespace

// Slot g < S.G of the search: alive and rooted at window row (row0 + g) % capacity when g < k, dead otherwise (as a retired
// self-play slot: the tree kernels leave it at once).  op[g] = −2 for every slot: the k_reroot behind this launch makes every
// tree Node::default() and returns its chunks, a dead slot's too.
__global__ __launch_bounds__(WAVES * 64) void k_reanalyse_roots(SearchDev S, WindowDev W, uint32_t row0, int k, int32_t* __restrict__ op) {
    const int g = (int)(blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (g >= S.G) return;
    const int lane = threadIdx.x & 63;
    if (g < k) {
        const size_t r = (size_t)((row0 + (uint32_t)g) % W.capacity);  // < 2^32: both terms < 2^31
        const uint32_t* s = (const uint32_t*)(W.states + r * W.bytes);
        uint32_t* d = (uint32_t*)(S.root_state + (size_t)g * W.bytes);
        for (uint32_t j = (uint32_t)lane; j < W.bytes / 4; j += 64) d[j] = s[j];  // lane-strided dwords: 64 or 96 of them
    }
    if (lane == 0) {
        S.alive[g] = g < k ? 1 : 0;
        op[g] = -2;
    }
}

// Slot g < k → window row (row0 + g) % capacity.  The row's visits are rewritten only when the root's children ARE the row's move
// list (same count, same move at every index) and at least one of them was visited; status[g] says which of the three it was.
// Nothing else of the row is written, and a row that is not updated is not written at all.
__global__ __launch_bounds__(WAVES * 64) void k_reanalyse_store(SearchDev S, WindowDev W, uint32_t row0, int k, uint8_t* __restrict__ status) {
    const int g = (int)(blockIdx.x * WAVES + (threadIdx.x >> 6));
    if (g >= k) return;
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)((row0 + (uint32_t)g) % W.capacity);
    const uint32_t root = S.root[g];
    const NodeCold rc = S.cold[root];
    const uint32_t nchild = (uint32_t)rc.nres & 0xfffu, cb = rc.child;
    const int32_t nm = W.n_moves[r];
    const size_t pool = (size_t)S.n_chunks << S.chunk_shift;
    // (the children block is checked against the pool before anything of it is read)
    bool same = nm >= 1 && nm <= EX_MOVES && nchild == (uint32_t)nm && cb != 0 && (size_t)cb + nchild <= pool;
    unsigned long long sum = 0;
    uint32_t c[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    if (same) {
        const uint16_t* rm = W.moves + r * EX_MOVES;
        bool differ = false;
        for (uint32_t i = (uint32_t)lane; i < nchild; i += 64) differ |= S.cold[cb + i].mv != rm[i];
        same = __ballot(differ) == 0ull;
    }
    if (same) {
        for (int q2 = 0; q2 < 2; q2++)  // the two uint4 runs of the row this lane writes: counts (q2·64 + lane)·4 … + 4
            for (int q = 0; q < 4; q++) {
                const uint32_t i = (uint32_t)((q2 * 64 + lane) * 4 + q);
                c[q2][q] = i < nchild ? S.hot[cb + i].visits : 0u;  // real visits: every virtual one is resolved after a backup
                sum += c[q2][q];
            }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    }
    const bool write = same && sum > 0ull;
    if (write) {
        uint4* dst = (uint4*)(W.visits + r * EX_MOVES);
        for (int q2 = 0; q2 < 2; q2++) dst[q2 * 64 + lane] = make_uint4(c[q2][0], c[q2][1], c[q2][2], c[q2][3]);
    }
    if (lane == 0) status[g] = write ? REANALYSE_UPDATED : same ? REANALYSE_UNVISITED : REANALYSE_MISMATCHED;
}

hipError_t launch_reanalyse_roots(hipStream_t st, const SearchDev& S, const WindowDev& W, uint32_t row0, int k, int32_t* op) {
    hipLaunchKernelGGL(k_reanalyse_roots, dim3((unsigned)((S.G + WAVES - 1) / WAVES)), dim3(WAVES * 64), 0, st, S, W, row0, k, op);
    return hipGetLastError();
}

hipError_t launch_reanalyse_store(hipStream_t st, const SearchDev& S, const WindowDev& W, uint32_t row0, int k, uint8_t* status) {
    if (k <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reanalyse_store, dim3((unsigned)((k + WAVES - 1) / WAVES)), dim3(WAVES * 64), 0, st, S, W, row0, k, status);
    return hipGetLastError();
}

}  // namespace tg
