// symm_kernels.hip — the dihedral symmetries at the evaluation (tg_policy_eval_symm) and in the search (TG_SYMM_HASHED).  No
// counterpart in the reference, which uses Symmetry (tak/src/symm.rs:11-20) for training examples only.  A translation unit of
// its own: every other code object stays what it was.
//   k_symm_perm     perm[s][j] = policy slot of the image under s of the move whose slot is j, from move_symm_image and
//                   move_index_dev over every move code that has a slot (once per engine, tg_net_finalize);
//   k_symm_images   one wave per (state, selected image): the image states of a slice, row i·k + r of the forward's batch;
//   k_symm_fold     policy[i][j] = (Σ_s p_s[i][perm[s][j]]) · (1/k), eval[i] = (Σ_s v_s[i]) · (1/k), ascending s;
//   k_symm_leaves   one wave per leaf slot of a search iteration: the leaf's state → its image under the hashed s, the
//                   children's policy indices → perm[s] of them.
#include "symm.cuh"
#include "tree_pass.cuh"  // ws_hash: the one statement of the state hash

namespace tg {

constexpr int SYMM_WAVES = 4;  // waves per 256-thread block

// Every move code that has a policy slot: thread = (square, field f, pattern byte).  Placements: f = piece ≤ 2, pattern 0.
// Spreads: the pattern's n significant bits sit at the top of the byte, values 1 … 2^n − 2 (move_map.rs:19-48; the legacy 5×5
// table decides for itself through lut5).  Two codes never share a slot, so every entry has one writer.
__global__ __launch_bounds__(256) void k_symm_perm(int n, int P, int legacy5, const int16_t* __restrict__ lut5, int32_t* __restrict__ perm) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    const uint32_t pat = t & 255u, f = (t >> 8) & 3u, sq = t >> 10;
    if ((int)sq >= n * n) return;
    if (pat == 0) { if (f > 2u) return; }
    else {
        const uint32_t low = n < 8 ? (1u << (8 - n)) - 1u : 0u, v = pat >> (8 - n);
        if ((pat & low) || v < 1u || v > (1u << n) - 2u) return;
    }
    const uint32_t m = sq | (f << 6) | (pat << 8);
    const int j = move_index_dev(m, n, legacy5 != 0, lut5);
    if (j < 0 || j >= P) return;
    for (int s = 0; s < 8; s++) {
        const int i = move_index_dev(move_symm_image(m, n, s), n, legacy5 != 0, lut5);
        perm[(size_t)s * P + j] = i >= 0 && i < P ? i : -1;
    }
}

// the r-th selected image of `mask` (r < popcount(mask))
__device__ inline int nth_image(uint32_t mask, int r) {
    int s = 0;
    for (; s < 8; s++)
        if ((mask >> s) & 1u) { if (r == 0) break; r--; }
    return s;
}

// states[i] under the r-th selected symmetry → out[i·k + r]; count = n·k waves
__global__ __launch_bounds__(256) void k_symm_images(const uint8_t* __restrict__ states, int count, int k, uint32_t mask, int n,
                                                     uint8_t* __restrict__ out) {
    const int w = (int)(blockIdx.x * SYMM_WAVES + (threadIdx.x >> 6));
    if (w >= count) return;
    const int i = w / k, sym = nth_image(mask, w % k);
    const Geom g = make_geom(n);
    WState s;
    ws_load(s, states + (size_t)i * g.bytes, g);
    const WState t = ws_symm_image(s, g, sym);
    ws_store(t, out + (size_t)w * g.bytes, g);
}

// blockIdx.y = state i, thread = output slot j: the WRITE of the output row and the read of perm[s] are coalesced, the read of
// p_s through perm[s] is the gather (a permutation of a row that the forward has just left in L2).  f32 adds in ascending s,
// the first selected image starts the sum, the product with 1/k comes last (takgpu.h states this order).  Thread 0 of a
// state's first block takes the value mean the same way.
__global__ __launch_bounds__(256) void k_symm_fold(const float* __restrict__ p, const float* __restrict__ v, const int32_t* __restrict__ perm,
                                                   int P, int k, uint32_t mask, float inv_k, float* __restrict__ policy,
                                                   float* __restrict__ eval) {
    const int i = (int)blockIdx.y;
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    const float* rows = p + (size_t)i * k * P;
    if (j < P) {
        float acc = 0.0f;
        int r = 0;
        for (int s = 0; s < 8; s++) {
            if (!((mask >> s) & 1u)) continue;
            const int src = perm[(size_t)s * P + j];
            const float x = src >= 0 ? rows[(size_t)r * P + src] : 0.0f;
            acc = r == 0 ? x : acc + x;
            r++;
        }
        policy[(size_t)i * P + j] = acc * inv_k;
    }
    if (j == 0) {
        float acc = v[(size_t)i * k];
        for (int r = 1; r < k; r++) acc += v[(size_t)i * k + r];
        eval[i] = acc * inv_k;
    }
}

// One wave per leaf slot the iteration hands to the network.  A slot that is not evaluated this iteration (leaf_kind ≠ 1: a
// terminal leaf, a skipped, dead or retired game) is left alone — the select writes every slot's kind in every iteration.
__global__ __launch_bounds__(256) void k_symm_leaves(SearchDev S, int leaves, const int32_t* __restrict__ perm,
                                                     unsigned long long* __restrict__ transformed) {
    const int slot = (int)(blockIdx.x * SYMM_WAVES + (threadIdx.x >> 6));
    if (slot >= leaves) return;
    if (uni((uint32_t)S.leaf_kind[slot]) != 1u) return;
    const int lane = lane_id();
    const Geom g = make_geom(S.n);
    uint8_t* st = S.leaf_state + (size_t)slot * g.bytes;
    WState s;
    ws_load(s, st, g);
    const uint64_t h = ws_hash(s, g);
    const int sym = (int)(uni(philox4x32_10(S.seed, (uint32_t)h, (uint32_t)(h >> 32), RNG_SYMM_TAG, 0u).v[0]) & 7u);
    if (sym == 0) return;
    const WState t = ws_symm_image(s, g, sym);
    ws_store(t, st, g);
    const uint32_t nchild = min(uni(S.leaf_rec[2 * (size_t)slot + 1]), (uint32_t)EX_MOVES);
    uint16_t* pidx = S.child_pidx + (size_t)slot * EX_MOVES;
    const int32_t* ps = perm + (size_t)sym * S.P;
    for (uint32_t i = lane; i < nchild; i += 64) {
        const uint32_t idx = pidx[i];
        if (idx == 0xFFFFu || (int)idx >= S.P) continue;  // unmapped entries stay 0xFFFF
        const int to = ps[idx];
        pidx[i] = to >= 0 ? (uint16_t)to : (uint16_t)0xFFFF;
    }
    if (lane == 0) __hip_atomic_fetch_add(transformed, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- launchers --------------------------------------------------------------------------------
hipError_t launch_symm_perm(hipStream_t st, int n, int P, bool legacy5, const int16_t* lut5, int32_t* perm) {
    hipLaunchKernelGGL(k_symm_perm, dim3((unsigned)(n * n) * 4u), dim3(256), 0, st, n, P, legacy5 ? 1 : 0, lut5, perm);
    return hipGetLastError();
}

hipError_t launch_symm_images(hipStream_t st, const uint8_t* states, int count, int k, uint32_t mask, int n, uint8_t* out) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_symm_images, dim3((count * k + SYMM_WAVES - 1) / SYMM_WAVES), dim3(256), 0, st, states, count * k, k, mask, n, out);
    return hipGetLastError();
}

hipError_t launch_symm_fold(hipStream_t st, const float* p, const float* v, const int32_t* perm, int count, int P, int k, uint32_t mask,
                            float* policy, float* eval) {
    for (int i0 = 0; i0 < count; i0 += 32768) {  // (grid.y stays below 2^16)
        const int c = count - i0 < 32768 ? count - i0 : 32768;
        hipLaunchKernelGGL(k_symm_fold, dim3((P + 255) / 256, c), dim3(256), 0, st, p + (size_t)i0 * k * P, v + (size_t)i0 * k, perm, P, k, mask,
                           1.0f / (float)k, policy + (size_t)i0 * P, eval + i0);
    }
    return hipGetLastError();
}

hipError_t launch_symm_leaves(hipStream_t st, const SearchDev& S, int leaves, const int32_t* perm, unsigned long long* transformed) {
    if (leaves <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_symm_leaves, dim3((leaves + SYMM_WAVES - 1) / SYMM_WAVES), dim3(256), 0, st, S, leaves, perm, transformed);
    return hipGetLastError();
}

}  // namespace tg
