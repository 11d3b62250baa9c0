// fc_kernels.hip — policy FC, softmax and value head of the policy/value resnet, exact f32 (layout and arithmetic: conv_kernels.hip).
//
// Kernels, in the order of the file:
//   k_gemm                  generic GEMM
//   k_fc_ring               policy FC for full batches: LDS-DMA ring of three K-steps, flag counters instead of barriers
//   k_fc_small              policy FC for ≤ 2048 rows (no LDS, no barrier)
//   k_fc_stats, k_softmax_stats, k_value_head, k_softmax(_conv), k_nchw_to_nhwc
// Both FC kernels accumulate every output element over k in the same order: a position's logits are the same bits whatever
// batch (and therefore kernel) evaluates it (tests/test_gpu_net.py, tests/test_gpu_variants.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "conv_mainloop.cuh"
#include "fc_ring.cuh"
#include "softmax.cuh"
#include "tower_stamps.cuh"
#include "kernels.h"

namespace tg {

// Plain GEMM out[M][N] = A[M][K]·W[K][N] + bias for the 5×5 policy FC (net5.rs:56-61,108): the same
// fragments, A staged through LDS in K-chunks of 32.
template <int RT, int CT>
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ A, int lda, const float* __restrict__ Wp,
                                              const float* __restrict__ bias, float* __restrict__ out, int M, int K,
                                              int NP, int out_stride, int n_valid) {
    constexpr int TM = 64 * RT;
    constexpr int KC = 32;
    constexpr int LS = KC + LDS_PAD;
    __shared__ __attribute__((aligned(16))) float lds[2][TM * LS];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * TM;
    const int wave = tid >> 6, lane = tid & 63;
    const int wr = wave & 1, wc = wave >> 1;
    const int i = lane & 31, h = lane >> 5;
    const int col0 = blockIdx.y * (64 * CT) + wc * (32 * CT);
    const float* wlane = Wp + ((size_t)(col0 + i) * 16 + 4 * h);
    const size_t wchunk_stride = (size_t)NP * 16;

    f32x16 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rt][ct][r] = 0.0f;

    auto stage = [&](int buf, int k0) {
        // TM rows × 8 float4
        for (int idx = tid; idx < TM * (KC / 4); idx += 256) {
            int r = idx >> 3, v = idx & 7;
            int m = m0 + r;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m < M) x = *(const float4*)(A + (size_t)m * lda + k0 + v * 4);
            *(float4*)&lds[buf][r * LS + v * 4] = x;
        }
    };

    const int nchunk = K / KC;
    stage(0, 0);
    __syncthreads();
    for (int kc = 0; kc < nchunk; kc++) {
        const int buf = kc & 1;
        if (kc + 1 < nchunk) stage(buf ^ 1, (kc + 1) * KC);
#pragma unroll
        for (int c8 = 0; c8 < KC / 8; c8++) {
            f32x4 a[RT], b[CT];
            const size_t kchunk = (size_t)kc * (KC / 8) + c8;
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
                b[ct] = *(const f32x4*)(wlane + (kchunk >> 1) * wchunk_stride + (size_t)ct * 32 * 16 + 8 * (kchunk & 1));
#pragma unroll
            for (int rt = 0; rt < RT; rt++) a[rt] = *(const f32x4*)&lds[buf][((wr * RT + rt) * 32 + i) * LS + c8 * 8 + 4 * h];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int ct = 0; ct < CT; ct++)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rt][t], b[ct][t], acc[rt][ct], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const int col = col0 + ct * 32 + i;
            const float bv = bias[col];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                int m = m0 + (wr * RT + rt) * 32 + row;
                if (m < M && col < n_valid) out[(size_t)m * out_stride + col] = acc[rt][ct][r] + bv;
            }
        }
}


// Policy FC (net5.rs:56-61,108) for the BASELINE shape M = 4096, K = 1600, N = 1575 (+ the value head in column 1575): 1576
// useful columns are 98.5 MFMA tiles of 16 → FC_TILES = 99.  A workgroup covers 128 rows (8 row tiles, one per wave) × 12 MAIN
// tiles (column block cb: tiles 12 cb … 12 cb + 11 = 192 columns) → 32 × 8 = 256 workgroups, one per CU — and ONE of the three
// leftover tiles (96, 97, 98) for some of its row tiles: the 8 row tiles × 3 leftover tiles of a row block are 24 (row tile,
// tile) pairs, dealt 3 / 3 / 2 / 3 / 3 / 2 / 4 / 4 to the 8 workgroups of the row block (fc_extra): workgroup cb computes
// leftover tile 96 + l for the row tiles s … s + ne − 1, in its waves 0 … ne − 1 — different SIMDs (waves w and w + 4 share
// one), so a SIMD carries 12 + 12 or 12 + 13 tile chains where round 3's 8 × 13-tile blocks (104 tiles, 5 of them padding)
// made it 26.  Wave w owns row tile (w + s) mod 8: the rotation puts the rows that need the leftover tile into waves 0 … ne − 1.
// The weights (shared by the 8 waves) go global → LDS in K-steps of 64, in four 16-byte-slot planes (one per k-quarter) so that
// a wave's 16 lanes of one plane hit 16 different bank groups: conflict-free ds_read_b128; slot 12 of a chunk's 13 tile slots
// holds the workgroup's leftover tile.  The wave's own 16 activation rows are the MFMA B operand, read straight from global.
constexpr int FC_CT = FC_MAIN_TILES + 1;  // tile slots per workgroup: 12 main + its leftover tile
constexpr int FC_KSTEP = 64;              // 4 chunks of 16
constexpr int FC_PLANE = (FC_KSTEP / 16) * FC_CT * 16;  // 832 slots per k-quarter plane (≡ 0 mod 16)

// Barrier-free ring: three weight buffers of one K-step filled by LDS-DMA (global_load_lds_dwordx4: no staging registers, no
// ds_write phase, 16 cache lines per instruction); the eight waves synchronise through two sets of monotonic counters in LDS
// instead of s_barrier:
//   ready[b] += 1 by every wave once its share of the K-step now in buffer b has landed (s_waitcnt vmcnt),
//   done[b]  += 1 by every wave once it has read the last fragment of the K-step in buffer b.
// A wave reads step s after ready[s % 3] = 8·(s/3 + 1) and refills buffer (s + 2) % 3 — in the MIDDLE of step s, half a
// step after it finished reading it itself — after done[(s + 2) % 3] = 8·⌊(s + 2)/3⌋.  Both flags are read half a chunk
// before they are needed and normally hold by then, so no wave waits out a round trip and the waves may drift half a step
// apart instead of draining the MFMA pipe at a barrier every 17 k cycles.  Every output element is accumulated over k in the
// same order by the same MFMA as in k_fc_small → identical logits bits (tests/test_gpu_net.py, batch independence).
// What bounds it (round 4's probe builds, profiles/r04_b_fc_candidates.txt): with neither refills nor flags the loop is 17 µs shorter —
// the LDS-DMA pieces' issue slots beside the fragment reads and waves held back for a slower one; the MFMAs of the 88 padded
// columns were 3.2 µs, the logits burst 3.7 µs.  Measured and discarded: a ninth wave that only fills the ring (8 – 10 µs
// slower), non-temporal logits stores, the barrier version k_fc_lds (rounds 1 – 3: + 6 µs), a register-tiled FC without LDS
// (k_fc_reg, scripts/probes/fc_reg.cuh: 227 µs — 2.7 × the operand bytes through the vector-memory path); round 4 also: a static
// s_setprio 1 for waves 4-7 (−1 µs, inside the noise) or for waves 0-3 (0), and waves 4-7 issuing their share of a refill half a
// step after waves 0-3 so that the two waves of a SIMD never issue LDS-DMA pieces at the same time (+ 11 µs: the older wave of
// a SIMD runs ahead of the younger one anyway, and the later refill makes the younger one the workgroup's laggard).
constexpr int FC_RING = 3;
constexpr int FC_RING_SLOTS = 4 * FC_PLANE;                                        // f32x4 slots per buffer (3328)
constexpr size_t FC_RING_LDS = (size_t)FC_RING * FC_RING_SLOTS * 16 + 2 * FC_RING * sizeof(uint32_t);
// (diagnostic build only — scripts/probes/fc_ring_stamps.hip: stamps of workgroup (0, 0); s_memtime has another base on every XCD)
#define TG_FC_STAMP(step, slot) do { if (blockIdx.y == 0) { TG_STAMP(step, slot); } } while (0)
template <int GEOM>  // 0: the policy head's 99 tiles (8 blocks + 3 leftover tiles, fc_extra); 1: 25x tiles as 2x blocks + x leftover tiles
__global__ __launch_bounds__(512) void k_fc_ring(const float* __restrict__ A, int lda, const float* __restrict__ Wp,
                                                 const float* __restrict__ bias, float* __restrict__ out, int M, int K, int NP,
                                                 int out_stride, int n_valid, int a_frag, float* __restrict__ stats, int n_soft,
                                                 const FcGather gather, const float* __restrict__ Wlin) {
    extern __shared__ __attribute__((aligned(16))) float fc_ring_lds[];
    f32x4* wl = (f32x4*)fc_ring_lds;                                // [FC_RING][chunk][tile slot][q][r16]
    uint32_t* flags = (uint32_t*)(wl + FC_RING * FC_RING_SLOTS);    // ready[FC_RING], done[FC_RING]
    const uint32_t ready0 = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t*)flags;  // LDS byte addresses
    const uint32_t done0 = ready0 + FC_RING * 4;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r16 = lane & 15, q = lane >> 4;
    // Which (row block, column block) this workgroup computes.  Workgroups go to the 8 XCDs round robin by their linear index, so with
    // (row block, column block) = blockIdx every XCD's L2 fetches ALL the weights (8 × 10.1 MB) and its quarter of the rows once: 107 MB.
    // An XCD that computes a column blocks × 32 / a row blocks fetches 10.1 a + 210 / a MB: least at a = 4 — XCD c gets column blocks
    // 4 (c & 1) … + 3 and every fourth row block from c >> 1 on.  Measured (scripts/probes/fc_xcd_map.sh): memory-side traffic 134.0 →
    // 120.5 MB with logits rows (3.64 → 3.27 × algorithmic), the launch time unchanged (166.3 – 166.6 µs either way: L2 misses that hit
    // the Infinity Cache were never what it waited for).  The same results by other workgroups: nothing changes in the output.
    int rbx = (int)blockIdx.x, cbx = (int)blockIdx.y;
    if (GEOM == 0 && (gridDim.x & 7) == 0) {
        const int xcd = rbx & 7, j = (rbx >> 3) + (int)(gridDim.x >> 3) * cbx;
        cbx = 4 * (xcd & 1) + (j & 3);
        rbx = (xcd >> 1) + 4 * (j >> 2);
    }
    const int cb = cbx;
    // GEOM 1 (round 4: the training step's FC data gradient, 200 tiles = 16 × 12 + 8): gridDim.y = 2x blocks; leftover tile cb / 2 for
    // row tiles 0 … 3 (even cb) or 4 … 7 (odd cb), in waves 0 … 3 — every SIMD carries 12 + 13 tile chains, no tile is padding.  (A template
    // parameter: the block count as a kernel argument cost the policy head 2.7 µs, 167.5 against 164.8 µs.)
    const int mb = GEOM == 0 ? FC_MAIN_BLOCKS : (int)gridDim.y;
    const FcExtra X = GEOM == 0 ? fc_extra(cb) : FcExtra{cb >> 1, 4 * (cb & 1), 4};
    const bool has13 = wave < X.ne;                    // this wave also computes the leftover tile for its rows (wave-uniform)
    const int rt = (wave + X.s) & 7;                   // row tile of the row block owned by this wave
    const int row = rbx * 128 + rt * 16 + r16;
    const bool row_ok = row < M;
    const int n0 = cb * (FC_MAIN_TILES * 16);          // first column of the main tiles
    const int nx = (FC_MAIN_TILES * mb + X.l) * 16;               // first column of the leftover tile
    // loads are unconditional (rows past the end read a valid row and are never stored): hipcc puts s_waitcnt vmcnt(0)
    // right behind an exec-masked global load.  Activations: row-major (one 16-B slot of its row per lane and chunk), or
    // fragment-major (TowerParams.frag_out: the wave's 16 rows × 16 k of a chunk are one contiguous KB)
    const int last_tile = (M - 1) >> 4;
    const int my_tile = min(rbx * 8 + rt, last_tile);
    const f32x4* ap = a_frag ? (const f32x4*)A + (size_t)my_tile * (K >> 4) * 64 + r16 * 4 + q
                             : (const f32x4*)(A + (size_t)(row_ok ? row : M - 1) * lda) + q;
    const size_t achunk = a_frag ? 64 : 4;
    const f32x4* wg = (const f32x4*)Wp;  // slot (chunk, col, q) at (chunk*NP + col)*4 + q
    const int nsteps = K / FC_KSTEP;
    const int nchunks = nsteps * 4;

    // LDS-DMA: one wave-instruction fills 64 consecutive slots of a buffer (1 KB) = one (chunk, tile slot) block, slot
    // q·16 + r16 inside it — the lane number of its reader, so the fragment reads are contiguous and conflict free — from
    // the block's 1 KB of the weight matrix (slot r16·4 + q: the permutation is on the source side, 16 cache lines per
    // instruction).  52 blocks per K-step, issued by the filler waves (below).
    // Wlin (optional): the same weights with every (chunk, tile) block stored in the READER's lane order — slot (chunk·NP/16 + tile)·64 +
    // q·16 + r16 — so that an LDS-DMA instruction's 64 lanes read 64 consecutive 16-byte slots (the permuted source makes each
    // quarter-wave touch 16 different cache lines of the block)
    if (Wlin) wg = (const f32x4*)Wlin;
    // Who issues the refills: waves 4-7 — the YOUNGER wave of every SIMD — issue all 52 pieces of a K-step (13 each), waves 0-3 none,
    // and ready[] counts 4 per use.  The older wave of a SIMD wins the matrix pipe and runs ahead; the younger one lags anyway, and
    // while it spends 2 – 3.5 k cycles per step handing pieces to the memory pipe its partner issues MFMAs undisturbed (measured,
    // profiles/r04_b_fc_candidates.txt §7: every wave issuing its share 168.9 µs, waves 0-3 all of them 168.5 µs, waves 4-7 all of
    // them 166.2 µs; TG_FC_ALL_FILL restores the first)
#ifdef TG_FC_ALL_FILL
    constexpr int FILLERS = 8, PER = 7;
    const int fwave = wave;
#else
    constexpr int FILLERS = 4, PER = 13;
    const int fwave = wave - 4;
#endif
    constexpr bool HALF_FILL = FILLERS < 8;
    uint32_t src0[PER];
#pragma unroll
    for (int u = 0; u < PER; u++) {
        int blk = (fwave < 0 ? 0 : fwave) + FILLERS * u;
        blk = blk < FC_RING_SLOTS / 64 ? blk : FC_RING_SLOTS / 64 - 1;
        const int c = blk / FC_CT, j = blk - c * FC_CT;
        const int col0 = j < FC_MAIN_TILES ? n0 + j * 16 : nx;
        src0[u] = Wlin ? (uint32_t)(((size_t)c * (NP >> 4) + (col0 >> 4)) * 64 + lane) : (uint32_t)(((size_t)c * NP + col0 + r16) * 4 + q);
    }
    const uint32_t step_slots = (uint32_t)(4 * NP * 4);  // f32x4 slots of the weights per K-step (either layout)
    auto fill = [&](int step, int buf) {
        if (HALF_FILL && (fwave < 0 || fwave >= FILLERS)) return;
#pragma unroll
        for (int u = 0; u < PER; u++)
            if (fwave + FILLERS * u < FC_RING_SLOTS / 64)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wg + (size_t)step * step_slots + src0[u]),
                                                 (__attribute__((address_space(3))) void*)(wl + buf * FC_RING_SLOTS + (fwave + FILLERS * u) * 64), 16, 0, 0);
    };
    auto aload = [&](int kc) { return ap[(size_t)(kc < nchunks ? kc : nchunks - 1) * achunk]; };
    if (tid < 2 * FC_RING) flags[tid] = 0u;
    __syncthreads();
    fill(0, 0);
    if (nsteps > 1) fill(1, 1);
    f32x4 acc[FC_CT];
#pragma unroll
    for (int j = 0; j < FC_CT; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // Activations: hipcc waits vmcnt(0) wherever the result of an ordinary load is consumed while an LDS-DMA load may be in
    // flight, and loads return in order.  So the four chunks up to the middle of the next step are requested at the top of
    // a step and forced to complete right before the refill is issued (two chunks later): no activation load is ever queued
    // behind a young refill, whose data comes from the MALL or HBM and takes its time.
    f32x4 a0 = aload(0), a1 = aload(1), a2, a3, b0, b1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const bool filler = !HALF_FILL || (fwave >= 0 && fwave < FILLERS);
    if (filler) {
        fc_ring_signal(ready0);
        if (nsteps > 1) fc_ring_signal(ready0 + 4);
    }
    // One chunk: the 13 weight fragments in two halves (7 + 6 tile slots; the 13th only feeds MFMAs in the waves that own a
    // leftover tile); each half is requested while the other half's MFMAs run, across chunk boundaries inside a step (the
    // tower's half-tile pipeline, conv_mainloop.cuh).
    constexpr int FC_H1 = 7;
    f32x4 w[FC_CT];
#define TG_FC_LOAD(C, J0, J1) _Pragma("unroll") for (int j = J0; j < J1; j++) w[j] = wb[((C) * FC_CT + j) * 64 + lane];
#define TG_FC_MFMA(AV, J0, J1)                                                                                       \
    _Pragma("unroll") for (int t = 0; t < 4; t++)                                                                    \
        _Pragma("unroll") for (int j = J0; j < J1; j++)                                                              \
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j][t], (AV)[t], acc[j], 0, 0, 0);
#define TG_FC_CHUNK(C, AV, NEXT, EARLY)                                                                              \
    TG_FC_LOAD(C, FC_H1, FC_CT)                                                                                      \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    TG_FC_MFMA(AV, 0, FC_H1)                                                                                         \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    if (NEXT) { TG_FC_LOAD((C) + 1, 0, FC_H1) }                                                                      \
    EARLY;                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    TG_FC_MFMA(AV, FC_H1, FC_MAIN_TILES)                                                                             \
    if (has13) { TG_FC_MFMA(AV, FC_MAIN_TILES, FC_CT) }                                                              \
    __builtin_amdgcn_sched_barrier(0);
    const volatile __attribute__((address_space(3))) uint32_t* flag_lds = (const volatile __attribute__((address_space(3))) uint32_t*)flags;
    uint32_t early_ready = 0u, early_done = 0u;
    // gather mode: what the epilogue needs of this wave's rows is requested under the last K-steps' MFMAs — row r16's child
    // count in lane r16, and per row the first 128 child indices, two 16-bit indices per lane
    uint32_t g_cnt = 0u, g_pidx[16];
#pragma unroll
    for (int r = 0; r < 16; r++) g_pidx[r] = 0u;
    for (int step = 0; step < nsteps; step++) {
        const int buf = step % FC_RING;
        const f32x4* wb = wl + buf * FC_RING_SLOTS;
        // (the flags were read half a chunk ago, under the MFMAs: they normally hold already and nobody waits out a round trip)
        TG_FC_STAMP(step, 0);  // (diagnostic build only: scripts/probes/fc_ring_stamps.hip)
        if ((int)__builtin_amdgcn_readfirstlane((int)early_ready) < FILLERS * (step / FC_RING + 1))
            fc_ring_wait(ready0 + 4 * buf, (uint32_t)FILLERS * (uint32_t)(step / FC_RING + 1));
        TG_FC_STAMP(step, 1);
        __builtin_amdgcn_sched_barrier(0);
        TG_FC_LOAD(0, 0, FC_H1)
        a2 = aload(step * 4 + 2);
        a3 = aload(step * 4 + 3);
        b0 = aload(step * 4 + 4);
        b1 = aload(step * 4 + 5);
        if (gather.child_logit && step == nsteps - 1) {  // (no refill follows in the last step: these loads wait for nobody)
            const int tile_row0 = rbx * 128 + rt * 16;
            g_cnt = gather.leaf_rec[2 * (size_t)min(tile_row0 + r16, M - 1) + 1];
#pragma unroll
            for (int r = 0; r < 16; r++)
                g_pidx[r] = ((const uint32_t*)(gather.child_pidx + (size_t)min(tile_row0 + r, M - 1) * gather.stride))[lane];
        }
        __builtin_amdgcn_sched_barrier(0);
        TG_FC_CHUNK(0, a0, true, (void)0)
        TG_FC_CHUNK(1, a1, true, early_done = flag_lds[FC_RING + (step + 2) % FC_RING])
        // the middle of the step: signal the step after this one, refill the buffer of the step before it
        TG_FC_STAMP(step, 2);
        asm volatile("" : "+v"(a2), "+v"(a3), "+v"(b0), "+v"(b1));  // the compiler's own wait for the four loads above …
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // … which, loads returning in order, covers last step's refill too
        // (leaving this wait to the compiler in the waves that issue no LDS-DMA: no change, 165.6 – 167.3 against 165.7 – 165.9 µs)
        TG_FC_STAMP(step, 3);
        if (step >= 1 && step + 1 < nsteps && filler) fc_ring_signal(ready0 + 4 * ((step + 1) % FC_RING));
        if (step + 2 < nsteps && filler) {
            if ((int)__builtin_amdgcn_readfirstlane((int)early_done) < 8 * ((step + 2) / FC_RING))
                fc_ring_wait(done0 + 4 * ((step + 2) % FC_RING), 8u * (uint32_t)((step + 2) / FC_RING));
            TG_FC_STAMP(step, 4);
            fill(step + 2, (step + 2) % FC_RING);
        }
        TG_FC_STAMP(step, 5);
        __builtin_amdgcn_sched_barrier(0);
        TG_FC_CHUNK(2, a2, true, (void)0)
        TG_FC_CHUNK(3, a3, false, early_ready = flag_lds[(step + 1) % FC_RING])
        fc_ring_signal(done0 + 4 * buf);
        TG_FC_STAMP(step, 6);
        a0 = b0;
        a1 = b1;
    }
    TG_FC_STAMP(nsteps, 0);
#undef TG_FC_LOAD
#undef TG_FC_MFMA
#undef TG_FC_CHUNK
    // ---- epilogue: bias; logits or the children's logits; the statistics of this wave's blocks of its rows ----
    f32x4 v[FC_CT];
#pragma unroll
    for (int j = 0; j < FC_MAIN_TILES; j++) v[j] = acc[j] + *(const f32x4*)&bias[n0 + j * 16 + 4 * q];
    v[FC_MAIN_TILES] = acc[FC_MAIN_TILES] + *(const f32x4*)&bias[nx + 4 * q];
    if (stats) {
        float m, sm;
        float* srow = stats + (size_t)(row_ok ? row : 0) * (FC_STAT_STRIDE * 2);
        fc_block_stats<FC_MAIN_TILES>(*reinterpret_cast<const f32x4(*)[FC_MAIN_TILES]>(&v[0]), n0 + 4 * q, min(n_soft, n0 + FC_MAIN_TILES * 16), m, sm);
        if (row_ok && q == 0) *(float2*)&srow[cb * 2] = make_float2(m, sm);
        if (has13) {
            fc_block_stats<1>(*reinterpret_cast<const f32x4(*)[1]>(&v[FC_MAIN_TILES]), nx + 4 * q, min(n_soft, nx + 16), m, sm);
            if (row_ok && q == 0) *(float2*)&srow[(FC_MAIN_BLOCKS + X.l) * 2] = make_float2(m, sm);
            // column n_soft (= P) is the value head's pre-activation: pair FC_STAT_BLOCKS of the record
            const int dv = n_soft - (nx + 4 * q);
            if (row_ok && dv >= 0 && dv < 4) *(float2*)&srow[FC_STAT_BLOCKS * 2] = make_float2(dv == 0 ? v[FC_MAIN_TILES][0] : dv == 1 ? v[FC_MAIN_TILES][1] : dv == 2 ? v[FC_MAIN_TILES][2] : v[FC_MAIN_TILES][3], 0.0f);
        }
    }
    if (out && row_ok) {
#pragma unroll
        for (int j = 0; j < FC_CT; j++) {
            const int nn = (j < FC_MAIN_TILES ? n0 + j * 16 : nx) + 4 * q;
            if (nn < n_valid && (j < FC_MAIN_TILES || has13)) {
                float* o = out + (size_t)row * out_stride + nn;
                if (nn + 3 < n_valid) *(f32x4*)o = v[j];
                else for (int t = 0; t < 4; t++) if (nn + t < n_valid) o[t] = v[j][t];
            }
        }
    }
    if (gather.child_logit) {
        // This wave's 16 rows × 13 tile slots (13 312 B) go into its eighth of the two ring buffers that hold no data of the last
        // K-step, once every wave has read the steps that lived there (done[] — normally long true: a wave is at most half a
        // step behind); every LDS-DMA into them landed steps ago.  The laggard of the workgroup never waits here.
        const int bA = nsteps % FC_RING, bB = (nsteps + 1) % FC_RING;
        auto uses = [&](int b) { return b < nsteps ? (nsteps - b + FC_RING - 1) / FC_RING : 0; };
        fc_ring_wait(done0 + 4 * bA, 8u * (uint32_t)uses(bA));
        fc_ring_wait(done0 + 4 * bB, 8u * (uint32_t)uses(bB));
        constexpr int RP = FC_CT * 16;  // floats per parked row (208)
        float* park[2] = {(float*)(wl + bA * FC_RING_SLOTS) + wave * (8 * RP), (float*)(wl + bB * FC_RING_SLOTS) + wave * (8 * RP)};
        {
            float* dst = park[r16 >> 3] + (r16 & 7) * RP + 4 * q;
#pragma unroll
            for (int j = 0; j < FC_CT; j++) *(f32x4*)&dst[j * 16] = v[j];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own parked rows, now read by other lanes of the same wave
        const int tile_row0 = rbx * 128 + rt * 16;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int grow = min(tile_row0 + r, M - 1);
            const uint32_t cnt = tile_row0 + r < M ? min((uint32_t)__builtin_amdgcn_readlane((int)g_cnt, r), (uint32_t)gather.stride) : 0u;
            const float* prow = park[r >> 3] + (r & 7) * RP;
            float* crow = gather.child_logit + (size_t)grow * gather.stride;
            const uint16_t* irow = gather.child_pidx + (size_t)grow * gather.stride;
            for (uint32_t c0 = 0; c0 < cnt; c0 += 128) {
                const uint32_t pair = c0 == 0 ? g_pidx[r] : ((const uint32_t*)(irow + c0))[lane];
#pragma unroll
                for (int hlf = 0; hlf < 2; hlf++) {
                    const uint32_t c = c0 + 2 * lane + hlf;
                    const uint32_t p = hlf ? pair >> 16 : pair & 0xFFFFu;
                    const uint32_t dm = p - (uint32_t)n0, dx = p - (uint32_t)nx;
                    const bool in_main = dm < (uint32_t)(FC_MAIN_TILES * 16), in_x = has13 && dx < 16u;
                    if (c < cnt && (in_main || in_x)) crow[c] = prow[in_main ? dm : FC_MAIN_TILES * 16 + dx];
                }
            }
        }
    }
}

// The same FC for SMALL batches (host-driven MCTS evaluates 16–32 leaves per call; Player, pit): k_fc_ring gives a row block
// of 128 positions to one workgroup and needs ≥ 4096 rows to fill the chip, so a 32-row call took as long as a 4096-row
// one.  Here a wave owns one 16-row tile × 2 output tiles and streams both operands straight from global (no LDS, no
// barrier): M/16 × NP/32 waves.  Every output element is accumulated over k in the same order by the same MFMA as in
// k_fc_ring, so the two kernels return identical bits and the choice between them is invisible.
constexpr int FCS_CT = 2;
// up to here the small-batch kernel is the faster one: k_fc_ring's launch takes ≈ 160 µs whatever the rows (M / 128 row blocks × 8 column
// blocks of workgroups, each through the whole K loop: 64 of 256 CUs at 1024 rows), k_fc_small 39 µs per 512 rows.  Round 6 (the games sweep's
// plateau between 512 and 1024 games was THIS, not the tower): 512 → 2048; 700 games 423 → 320 µs per iteration, 1024: 422 → 342, 1500:
// 589 → 527, 2048: 591 → 566 (profiles/r06_e_tower_pw_sweep.txt)
constexpr int FC_SMALL_ROWS = 2048;
__global__ __launch_bounds__(256) void k_fc_small(const float* __restrict__ A, int lda, const float* __restrict__ Wp,
                                                  const float* __restrict__ bias, float* __restrict__ out, int M, int K, int NP,
                                                  int out_stride, int n_valid, int a_frag) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r16 = lane & 15, q = lane >> 4;
    const int row = blockIdx.x * 16 + r16;
    const bool row_ok = row < M;
    const int n0 = (blockIdx.y * 4 + wave) * (FCS_CT * 16);
    if (n0 >= NP) return;
    const f32x4* ap = a_frag ? (const f32x4*)A + (size_t)blockIdx.x * (K >> 4) * 64 + r16 * 4 + q
                             : (const f32x4*)(A + (size_t)(row_ok ? row : M - 1) * lda) + q;
    const size_t achunk = a_frag ? 64 : 4;
    const f32x4* wg = (const f32x4*)Wp + ((size_t)(n0 + r16) * 4 + q);  // slot (chunk, col, q) at (chunk*NP + col)*4 + q
    const size_t wchunk = (size_t)NP * 4;
    const int nchunks = K >> 4;
    constexpr int D = 4;  // chunks in flight
    f32x4 a[D], w[D][FCS_CT];
#pragma unroll
    for (int d = 0; d < D; d++) {
        const int kc = d < nchunks ? d : nchunks - 1;
        a[d] = ap[(size_t)kc * achunk];
#pragma unroll
        for (int j = 0; j < FCS_CT; j++) w[d][j] = wg[(size_t)kc * wchunk + j * 64];
    }
    f32x4 acc[FCS_CT];
#pragma unroll
    for (int j = 0; j < FCS_CT; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    for (int kc0 = 0; kc0 < nchunks; kc0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            if (kc0 + d < nchunks) {
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int j = 0; j < FCS_CT; j++) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w[d][j][t], a[d][t], acc[j], 0, 0, 0);
            }
            const int kn = kc0 + d + D < nchunks ? kc0 + d + D : nchunks - 1;
            a[d] = ap[(size_t)kn * achunk];
#pragma unroll
            for (int j = 0; j < FCS_CT; j++) w[d][j] = wg[(size_t)kn * wchunk + j * 64];
        }
    }
    if (row_ok) {
#pragma unroll
        for (int j = 0; j < FCS_CT; j++) {
            const int nn = n0 + j * 16 + 4 * q;
            if (nn < n_valid) {
                f32x4 v = acc[j] + *(const f32x4*)&bias[nn];
                float* o = out + (size_t)row * out_stride + nn;
                if (nn + 3 < n_valid) *(f32x4*)o = v;
                else for (int t = 0; t < 4; t++) if (nn + t < n_valid) o[t] = v[t];
            }
        }
    }
}

// The softmax statistics of softmax.cuh from logits already in memory, for the producers that cannot emit them from their
// accumulators (k_fc_small: a wave there owns 2 output tiles, not a block's 12).  A wave covers 16 (row, block) pairs with the
// FC's own lane layout — lane = pair + 16·q holds columns col0(block) + 16 j + 4 q + t — so fc_block_stats runs unchanged (a
// single-tile block through the 12-tile template with its limit at the block's end: the same bits); the wave that handles a
// row's block 0 also copies the value pre-activation (column n_soft) into pair FC_STAT_BLOCKS of the record.
__global__ __launch_bounds__(256) void k_fc_stats(const float* __restrict__ logits, int ld, int M, int n_soft, float* __restrict__ stats) {
    const int lane = threadIdx.x & 63, r16 = lane & 15, q = lane >> 4;
    const long pair0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16;
    const long total = (long)M * FC_STAT_BLOCKS;
    if (pair0 >= total) return;
    const long pair = pair0 + r16 < total ? pair0 + r16 : total - 1;
    const int row = (int)(pair / FC_STAT_BLOCKS), b = (int)(pair - (long)row * FC_STAT_BLOCKS);
    const int col0 = fc_stat_col0(b), tiles = fc_stat_tiles(b);
    const float* x = logits + (size_t)row * ld + col0 + 4 * q;
    f32x4 v[FC_MAIN_TILES];
#pragma unroll
    for (int j = 0; j < FC_MAIN_TILES; j++) v[j] = j < tiles ? *(const f32x4*)&x[16 * j] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m, sm;
    fc_block_stats<FC_MAIN_TILES>(v, col0 + 4 * q, min(n_soft, col0 + 16 * tiles), m, sm);
    if (q == 0 && pair0 + r16 < total) {
        float* srow = stats + (size_t)row * (FC_STAT_STRIDE * 2);
        *(float2*)&srow[b * 2] = make_float2(m, sm);
        if (b == 0) *(float2*)&srow[FC_STAT_BLOCKS * 2] = make_float2(logits[(size_t)row * ld + n_soft], 0.0f);
    }
}

// softmax of the FC head from the block statistics (tg_policy_eval; the search never materialises probabilities): the same
// exp(x − M) · (1 / S) the tree backup evaluates for a leaf's children, so host-side trees built from these probabilities
// and the engine's own agree bit for bit.  One block per position.
__global__ __launch_bounds__(256) void k_softmax_stats(const float* __restrict__ logits, int row_stride, const float* __restrict__ stats,
                                                       int blocks, int stat_stride, int P, float* __restrict__ policy, float* __restrict__ eval) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (size_t)b * row_stride;
    float mx, inv;
    fc_combine_stats(stats + (size_t)b * stat_stride * 2, blocks, mx, inv);
    if (eval && tid == 0) eval[b] = tanhf(x[P]);
    float* o = policy + (size_t)b * P;
    for (int p = tid; p < P; p += 256) o[p] = stat_exp(x[p] - mx) * inv;
}

// value head: Linear(F·N² → 1) + tanh (net5.rs:62,109 / net6.rs:57,104-107).  One wave per position;
// wv is permuted to the NHWC order of the activations.
__global__ __launch_bounds__(256) void k_value_head(const float* __restrict__ act, const float* __restrict__ wv, float bv,
                                                    int B, int len, float* __restrict__ eval) {
    int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int lane = threadIdx.x & 63;
    const float4* a = (const float4*)(act + (size_t)b * len);
    const float4* w = (const float4*)wv;
    float s = 0.0f;
    for (int k = lane; k < (len >> 2); k += 64) {
        float4 x = a[k], y = w[k];
        s = fmaf(x.x, y.x, s);
        s = fmaf(x.y, y.y, s);
        s = fmaf(x.z, y.z, s);
        s = fmaf(x.w, y.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) eval[b] = tanhf(s + bv);
}

// softmax over ALL P outputs (no legal-move mask; net5.rs:108, net6.rs:100-103).  One 256-thread block
// per position.  logits are stored [b][row_stride] with element (sq, ch) at sq*ch_stride + ch when
// conv_head (NHWC conv output) or simply [b][p] for the FC head; the probabilities are written in the
// reference's order p = ch·N² + sq.
__global__ __launch_bounds__(256) void k_softmax(const float* __restrict__ logits, int row_stride, int conv_head, int nsq,
                                                 int ch_stride, int P, float* __restrict__ policy, float* __restrict__ eval) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x = logits + (size_t)b * row_stride;
    if (eval && tid == 0) eval[b] = tanhf(x[P]);  // FC head: column P of the policy FC is the value head's pre-activation
    auto at = [&](int p) -> float {
        if (!conv_head) return x[p];
        int ch = p / nsq, sq = p - ch * nsq;
        return x[sq * ch_stride + ch];
    };
    // the row is read once and kept in registers when it fits (P ≤ 8·256: the FC head's 1575 outputs)
    constexpr int KEEP = SOFTMAX_KEEP;
    const bool cached = P <= KEEP * 256;
    float v[KEEP];
    float mx = -INFINITY;
    if (cached) {
#pragma unroll
        for (int k = 0; k < KEEP; k++) {
            int p = tid + k * 256;
            v[k] = p < P ? at(p) : -INFINITY;
            mx = fmaxf(mx, v[k]);
        }
    } else {
        for (int p = tid; p < P; p += 256) mx = fmaxf(mx, at(p));
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float s = 0.0f;
    if (cached) {
#pragma unroll
        for (int k = 0; k < KEEP; k++) {
            int p = tid + k * 256;
            v[k] = p < P ? expf(v[k] - mx) : 0.0f;
            s += v[k];
        }
    } else {
        for (int p = tid; p < P; p += 256) s += expf(at(p) - mx);
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    float inv = 1.0f / s;
    float* o = policy + (size_t)b * P;
    if (cached) {
#pragma unroll
        for (int k = 0; k < KEEP; k++) {
            int p = tid + k * 256;
            if (p < P) o[p] = v[k] * inv;
        }
    } else {
        for (int p = tid; p < P; p += 256) o[p] = expf(at(p) - mx) * inv;
    }
}

// Conv policy head (net6.rs:98-103): the logits sit in NHWC ([sq][ch_stride]) and the probabilities leave in the
// reference's order p = ch·N² + sq.  One block per position: the row is read once, coalesced, into LDS (pitch
// ch_stride + 1 so that the transposed read-out is bank-conflict free), exp is evaluated once per output.
// act != nullptr (round 6): the block's first wave also computes the position's value head — k_value_head's sum, lane for lane — so the
// conv-head forward is one launch shorter (7 µs of the 291 µs iteration at the reference's 32 leaves)
__global__ __launch_bounds__(256) void k_softmax_conv(const float* __restrict__ logits, int nsq, int ch_stride, int C,
                                                      float* __restrict__ policy, const float* __restrict__ act,
                                                      const float* __restrict__ wv, float bv, int len, float* __restrict__ eval) {
    extern __shared__ float row[];  // nsq × (ch_stride + 1)
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pitch = ch_stride + 1;
    const int vpr = ch_stride >> 2;
    const f32x4* x4 = (const f32x4*)(logits + (size_t)b * nsq * ch_stride);
    float mx = -INFINITY;
    for (int idx = tid; idx < nsq * vpr; idx += 256) {
        int sq = idx / vpr, v = idx - sq * vpr;
        f32x4 x = x4[idx];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            int ch = 4 * v + t;
            row[sq * pitch + ch] = x[t];
            if (ch < C) mx = fmaxf(mx, x[t]);
        }
    }
    mx = wave_max(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    const int P = C * nsq;
    float s = 0.0f;
    for (int p = tid; p < P; p += 256) {
        int ch = p / nsq, sq = p - ch * nsq;
        float e = expf(row[sq * pitch + ch] - mx);
        row[sq * pitch + ch] = e;
        s += e;
    }
    s = wave_sum(s);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    s = (red[0] + red[1]) + (red[2] + red[3]);
    const float inv = 1.0f / s;
    float* o = policy + (size_t)b * P;
    for (int p = tid; p < P; p += 256) {
        int ch = p / nsq, sq = p - ch * nsq;
        o[p] = row[sq * pitch + ch] * inv;
    }
    if (act && tid < 64) {  // value head: Linear(F·N² → 1) + tanh, exactly as k_value_head (one wave per position, lane = tid)
        const float4* a = (const float4*)(act + (size_t)b * len);
        const float4* w = (const float4*)wv;
        float v = 0.0f;
        for (int k = tid; k < (len >> 2); k += 64) {
            float4 x = a[k], y = w[k];
            v = fmaf(x.x, y.x, v);
            v = fmaf(x.y, y.y, v);
            v = fmaf(x.z, y.z, v);
            v = fmaf(x.w, y.w, v);
        }
        v = wave_sum(v);
        if (tid == 0) eval[b] = tanhf(v + bv);
    }
}

// NCHW planes (the reference tensor layout) → NHWC rows padded to Cpad channels
__global__ void k_nchw_to_nhwc(const float* __restrict__ src, int B, int C, int nsq, int Cpad, float* __restrict__ dst) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)B * nsq * Cpad;
    if (idx >= total) return;
    int c = (int)(idx % Cpad);
    size_t r = idx / Cpad;
    int sq = (int)(r % nsq);
    size_t b = r / nsq;
    dst[idx] = c < C ? src[(b * C + c) * nsq + sq] : 0.0f;
}

// the gather epilogue (k_fc_ring<0> only) is offered above this many rows: FC_SMALL_ROWS' value, inherited, not separately measured
constexpr int FC_GATHER_ABOVE_ROWS = 2048;
static_assert(FC_GATHER_ABOVE_ROWS >= FC_SMALL_ROWS, "k_fc_small has no gather epilogue");
// plain 25x-tile GEMMs (the FC data gradient of the training step) take k_fc_ring<1> above this many rows: inherited likewise, not separately measured
constexpr int FC_RING_GEMM_ABOVE_ROWS = 2048;
// the FC kernels of the 5×5 policy head: K-steps of 64, the 99 tiles of softmax.cuh's geometry inside NP columns
static bool fc_shape_ok(int K, int NP) { return K % FC_KSTEP == 0 && NP >= FC_TILES * 16 && NP % (FCS_CT * 16) == 0; }
bool fc_frag_supported(int K, int NP) { return fc_shape_ok(K, NP); }
bool fc_stats_supported(int K, int NP, int out_stride) { return fc_shape_ok(K, NP) && out_stride == NP; }
bool fc_gather_supported(int M, int K, int NP) { return fc_shape_ok(K, NP) && M > FC_GATHER_ABOVE_ROWS; }

hipError_t launch_gemm(hipStream_t st, const float* A, int lda, const float* Wp, const float* bias, float* out, int M, int K,
                       int NP, int out_stride, int n_valid, bool a_frag, float* stats, int n_soft, const FcGatherArgs* gather,
                       const float* Wlin) {
    if (a_frag && !fc_frag_supported(K, NP)) return hipErrorInvalidValue;
    if (stats && (!fc_stats_supported(K, NP, out_stride) || n_valid > FC_TILES * 16)) return hipErrorInvalidValue;
    if (gather && (!stats || !fc_gather_supported(M, K, NP))) return hipErrorInvalidValue;
    const bool fc = fc_shape_ok(K, NP) && n_valid <= FC_TILES * 16;
    if (fc && M <= FC_SMALL_ROWS) {
        dim3 grid((M + 15) / 16, (NP / (FCS_CT * 16) + 3) / 4);
        hipLaunchKernelGGL(k_fc_small, grid, dim3(256), 0, st, A, lda, Wp, bias, out, M, K, NP, out_stride, n_valid, a_frag ? 1 : 0);
        if (stats) {  // (columns ≥ n_valid of `out` are never written by any FC kernel and never enter the statistics: n_soft < n_valid)
            const long pairs = (long)M * FC_STAT_BLOCKS;
            hipLaunchKernelGGL(k_fc_stats, dim3((unsigned)((pairs + 63) / 64)), dim3(256), 0, st, out, out_stride, M, n_soft, stats);
        }
        return hipGetLastError();
    }
    if (fc) {
        static LdsAttr lds_attr;
        if (hipError_t e = lds_attr.ensure((const void*)k_fc_ring<0>, FC_RING_LDS); e != hipSuccess) return e;
        FcGather g{nullptr, nullptr, nullptr, 0};
        if (gather) g = FcGather{gather->child_pidx, gather->leaf_rec, gather->child_logit, gather->stride};
        hipLaunchKernelGGL(k_fc_ring<0>, dim3((M + 127) / 128, FC_MAIN_BLOCKS), dim3(512), FC_RING_LDS, st, A, lda, Wp, bias, gather ? nullptr : out, M, K, NP,
                           out_stride, n_valid, a_frag ? 1 : 0, stats, n_soft, g, Wlin);
        return hipGetLastError();
    }
    // Round 4: plain row-major GEMMs whose 25x output tiles split into 2x blocks of 12 + x leftover tiles take the ring too — the FC
    // head's data gradient in the training step (dlogits[4000 × 1600] · Wᵀ → 3200 columns = 200 tiles): 465 µs in k_gemm below
    if (K % FC_KSTEP == 0 && NP % 400 == 0 && M > FC_RING_GEMM_ABOVE_ROWS && !a_frag && !stats && !gather) {
        static LdsAttr lds_attr;
        if (hipError_t e = lds_attr.ensure((const void*)k_fc_ring<1>, FC_RING_LDS); e != hipSuccess) return e;
        hipLaunchKernelGGL(k_fc_ring<1>, dim3((M + 127) / 128, NP / 200), dim3(512), FC_RING_LDS, st, A, lda, Wp, bias, out, M, K, NP, out_stride, n_valid, 0,
                           nullptr, 0, FcGather{nullptr, nullptr, nullptr, 0}, nullptr);
        return hipGetLastError();
    }
    dim3 grid((M + 127) / 128, NP / 64);
    hipLaunchKernelGGL((k_gemm<2, 1>), grid, dim3(256), 0, st, A, lda, Wp, bias, out, M, K, NP, out_stride, n_valid);
    return hipGetLastError();
}

hipError_t launch_fc_stats(hipStream_t st, const float* logits, int ld, int M, int n_soft, float* stats) {
    const long pairs = (long)M * FC_STAT_BLOCKS;
    hipLaunchKernelGGL(k_fc_stats, dim3((unsigned)((pairs + 63) / 64)), dim3(256), 0, st, logits, ld, M, n_soft, stats);
    return hipGetLastError();
}

hipError_t launch_value_head(hipStream_t st, const float* act, const float* wv, float bv, int B, int len, float* eval) {
    hipLaunchKernelGGL(k_value_head, dim3((B + 3) / 4), dim3(256), 0, st, act, wv, bv, B, len, eval);
    return hipGetLastError();
}

// value (optional, conv head only): the value head's inputs — when the transposing kernel takes the batch it computes the eval too and
// *value_done is set; otherwise the caller launches k_value_head as before
hipError_t launch_softmax(hipStream_t st, const float* logits, int row_stride, bool conv_head, int nsq, int ch_stride, int P,
                          int B, float* policy, float* eval, const ValueHeadArgs* value, bool* value_done) {
    if (value_done) *value_done = false;
    if (conv_head && (ch_stride & 3) == 0 && (size_t)nsq * (ch_stride + 1) * 4 <= 64 * 1024) {
        const bool fuse = value && value->act && value->eval && (value->len & 3) == 0;
        hipLaunchKernelGGL(k_softmax_conv, dim3(B), dim3(256), (size_t)nsq * (ch_stride + 1) * 4, st, logits, nsq, ch_stride, P / nsq, policy,
                           fuse ? value->act : nullptr, fuse ? value->wv : nullptr, fuse ? value->bv : 0.0f, fuse ? value->len : 0,
                           fuse ? value->eval : nullptr);
        if (value_done) *value_done = fuse;
        return hipGetLastError();
    }
    hipLaunchKernelGGL(k_softmax, dim3(B), dim3(256), 0, st, logits, row_stride, conv_head ? 1 : 0, nsq, ch_stride, P, policy, conv_head ? nullptr : eval);
    return hipGetLastError();
}

hipError_t launch_softmax_stats(hipStream_t st, const float* logits, int row_stride, const float* stats, int blocks, int stat_stride, int P,
                                int B, float* policy, float* eval) {
    hipLaunchKernelGGL(k_softmax_stats, dim3(B), dim3(256), 0, st, logits, row_stride, stats, blocks, stat_stride, P, policy, eval);
    return hipGetLastError();
}

hipError_t launch_nchw_to_nhwc(hipStream_t st, const float* src, int B, int C, int nsq, int Cpad, float* dst) {
    size_t total = (size_t)B * nsq * Cpad;
    hipLaunchKernelGGL(k_nchw_to_nhwc, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, B, C, nsq, Cpad, dst);
    return hipGetLastError();
}

}  // namespace tg
