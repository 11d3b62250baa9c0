// net_s3_kernels.hip — the residual tower on the bf16 matrix cores with split operands ("bf16x3").
//
// Every f32 value x is carried as two bf16 numbers, hi = bf16(x) and lo = bf16(x − hi) (16 mantissa bits together),
// and a product a·w is evaluated as a_hi·w_hi + a_lo·w_hi + a_hi·w_lo by three v_mfma_f32_16x16x32_bf16 into an f32
// accumulator (bf16×bf16 products are exact in f32; only the a_lo·w_lo term, ≈ 2⁻¹⁶ relative, is dropped).  The bf16
// pipe runs 16× the f32 MFMA rate per MAC, so three passes cost 3/16 of the exact-f32 tower.  Deviation from the f32
// forward on the BASELINE networks: policy ≤ 1e-8 absolute / 1e-5 relative, eval ≤ 3e-6 (tests/test_gpu_net.py) —
// well inside the 1e-4 of BASELINE.json's north_star; plain bf16 (one pass) would miss it by 10×.
// This is the throughput variant of SURVEY.md §7 step 5; the exact-f32 tower (tower_kernels.hip) stays the default.
//
// Structure = the f32 towers: a workgroup keeps PW whole positions in LDS for all 1+2R layers, one launch.
//   k_tower_s3        plain LDS image (batches below 256 positions).  Row of a board square: per chunk of 32 channels eight
//                     16-byte slots — hi of the channel groups q = 0..3, then lo of q = 0..3 — and 32 B of padding; a zero
//                     REGION for off-board taps.  An MFMA B operand (32 k × 16 rows) is two ds_read_b128 per lane (slots q
//                     and 4 + q of the chunk); ds_read_b128 is served in lane groups that pair 8 rows of one q with 8 rows
//                     of the next (MI355X_MICROARCH.md §LDS), and this pitch keeps a group on 16 distinct bank quads.
//   k_tower_s3_halo   the halo image of k_tower_halo (tower_kernels.hip): cell pitch F/4 + 1 slots, the same slot table,
//                     taps as ds_read immediates, pinned half-tile pipeline, weight stream across layers.  Full batches.
// The A operand (16 output channels × 32 k) is two 16-B loads of the pre-split weights [chunk][tile][hi|lo][q][cout]; a wave
// owns 2 channel tiles × RTW row tiles (every activation fragment feeds 6 MFMAs) and its 32 output channels are ordered so
// that lane group q ends up with channels 8q … 8q + 7 — one hi and one lo slot of the image (net.hip upload_conv_s3).
//   k_fc_s3b, k_fc_s3_ring, k_value_head_s3   policy FC (≤ 512 rows / full batches) and value head on the split activations.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "board.cuh"
#include "conv_mainloop.cuh"
#include "softmax.cuh"
#include "fc_ring.cuh"
#include "tower_stage.cuh"
#include "kernels.h"


namespace tg {

// Diagnostic build only (scripts/probes/tower_s3_stamps.hip, -DTG_S3_STAMPS): s_memtime stamps of one workgroup's waves at the
// phase boundaries of every layer of k_tower_s3_halo.  The product build compiles none of it.
#ifdef TG_S3_STAMPS
__device__ unsigned long long* g_s3_stamps = nullptr;  // [layer][wave][8]
#define TG_S3_STAMP(layer, slot)                                                                                    \
    do {                                                                                                            \
        if (blockIdx.x == 8 && g_s3_stamps && (threadIdx.x & 63) == 0)                                              \
            g_s3_stamps[((size_t)(layer) * 16 + (threadIdx.x >> 6)) * 8 + (slot)] = __builtin_amdgcn_s_memtime();  \
    } while (0)
#else
#define TG_S3_STAMP(layer, slot) do { } while (0)
#endif

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using u32x2 = __attribute__((ext_vector_type(2))) uint32_t;

__device__ __forceinline__ uint32_t pk_bf16(float a, float b) {  // (bf16(a), bf16(b)), round to nearest even
    uint32_t r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float bf16_lo_f32(uint32_t pk) { return __uint_as_float(pk << 16); }
__device__ __forceinline__ float bf16_hi_f32(uint32_t pk) { return __uint_as_float(pk & 0xffff0000u); }

// 4 floats → their hi and lo halves, packed as 4 bf16 each
__device__ __forceinline__ void split4(const f32x4& v, u32x2& hi, u32x2& lo) {
    hi[0] = pk_bf16(v[0], v[1]);
    hi[1] = pk_bf16(v[2], v[3]);
    lo[0] = pk_bf16(v[0] - bf16_lo_f32(hi[0]), v[1] - bf16_hi_f32(hi[0]));
    lo[1] = pk_bf16(v[2] - bf16_lo_f32(hi[1]), v[3] - bf16_hi_f32(hi[1]));
}
__device__ __forceinline__ f32x4 join4(const u32x2& hi, const u32x2& lo) {
    f32x4 v;
    v[0] = bf16_lo_f32(hi[0]) + bf16_lo_f32(lo[0]);
    v[1] = bf16_hi_f32(hi[0]) + bf16_hi_f32(lo[0]);
    v[2] = bf16_lo_f32(hi[1]) + bf16_lo_f32(lo[1]);
    v[3] = bf16_hi_f32(hi[1]) + bf16_hi_f32(lo[1]);
    return v;
}

__device__ __forceinline__ bf16x8 as_bf(const u32x4& v) { return __builtin_bit_cast(bf16x8, v); }

// One layer for NT row tiles × 2 channel tiles.  lds4: image in 16-byte slots, row pitch LS4, chunk kc of a row at
// slot kc·8 + q (hi) and kc·8 + 4 + q (lo).  wp: this lane's weight slot pair of chunk 0 (channel tile 0), tile 1 at +t1,
// next chunk at +wstride (all in 16-byte units).
template <int NT, int KC>
__device__ __forceinline__ void s3_mainloop(const u32x4* __restrict__ lds4, const u32x4* __restrict__ wp, int t1, int wstride, int LS4,
                                            int zrow, int zshift, int n, int rho0, int q, const int* vmask, f32x4 (&acc)[NT][2]) {
    // A tap that leaves the board reads zeros.  zshift = 1: from a zero REGION addressed like the image (row zrow + tap
    // shift, zrow ≡ this lane's row mod 16), so that the masked lanes keep the bank pattern of the others — a single zero row
    // (zshift = 0) costs ≈ 7 LDS cycles per ds_read_b128 instead of 4 in the bank model of MI355X_MICROARCH.md §LDS.
    const int zero4 = zrow * LS4 + q;
    const int base0 = rho0 * LS4 + q;
    u32x4 wh0 = wp[0], wl0 = wp[64], wh1 = wp[t1], wl1 = wp[t1 + 64];
    int kk = 0;
    constexpr int total = 9 * KC;
#pragma unroll 1
    for (int tap = 0; tap < 9; tap++) {
        const int sh = ((tap / 3 - 1) * n + (tap % 3 - 1)) * LS4;
        int aoff[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) aoff[j] = ((vmask[j] >> tap) & 1) ? base0 + j * 16 * LS4 + sh : zero4 + sh * zshift;
#pragma unroll
        for (int kc = 0; kc < KC; kc++) {
            const int kn = kk + 1 < total ? kk + 1 : kk;
            const u32x4* wn = wp + (size_t)kn * wstride;
            const u32x4 nh0 = wn[0], nl0 = wn[64], nh1 = wn[t1], nl1 = wn[t1 + 64];
            u32x4 ah[NT], al[NT];
#pragma unroll
            for (int j = 0; j < NT; j++) {
                ah[j] = lds4[aoff[j] + kc * 8];
                al[j] = lds4[aoff[j] + kc * 8 + 4];
            }
#pragma unroll
            for (int j = 0; j < NT; j++) {
                acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh0), as_bf(ah[j]), acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh1), as_bf(ah[j]), acc[j][1], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NT; j++) {
                acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh0), as_bf(al[j]), acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh1), as_bf(al[j]), acc[j][1], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < NT; j++) {
                acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wl0), as_bf(ah[j]), acc[j][0], 0, 0, 0);
                acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wl1), as_bf(ah[j]), acc[j][1], 0, 0, 0);
            }
            wh0 = nh0; wl0 = nl0; wh1 = nh1; wl1 = nl1;
            kk++;
        }
    }
}


// The same layer over the HALO image (conv_mainloop.cuh: zero cells between board rows and positions, taps as immediates of
// ds_read_b128, squares dealt to tile slots by tower_halo_slotmap).  Cell pitch = F/4 + 1 slots of 16 B (8·KC + 1): hi
// slots q = 0..3 then lo slots of every 32-channel chunk, one slot of padding, so that the bank quad of a read is
// (cell + slot) mod 16 as in the f32 kernel.  addr4[j] = (cell − (NB + 2))·pitch + q.  One board row of taps per trip.
// Scheduling is pinned as in conv_mainloop_halo: the tiles in two halves, each half's fragments requested while the other
// half's 6·H MFMAs run; weights through a buffer descriptor, two steps ahead.  (Left to itself the compiler sinks every
// load to just before its first use to save registers and each wave then waits out the LDS and L2 latencies.  s_setprio
// turns between the two waves of a SIMD, which pay in the f32 kernel, made no difference here.)
struct S3W { u32x4 h0, l0, h1, l1; };  // one step of weights of a wave: hi / lo halves of its two 16-channel tiles
// step kk of a layer at byte kk·wstep; inside a step this lane's four 16-byte slots 1 KB apart
__device__ __forceinline__ S3W s3_load_w(const void* wlayer, int bytes, uint32_t wlane, int so) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)wlayer, 0, bytes, 0x00020000);
    S3W w;
    w.h0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, wlane, so, 0));
    w.l0 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, wlane + 1024, so, 0));
    w.h1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, wlane + 2048, so, 0));
    w.l1 = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, wlane + 3072, so, 0));
    return w;
}
// w0 / w1 arrive holding steps 0 and 1 of this layer and leave holding those of `wnext` (same geometry), requested by the
// last two steps: the epilogue and the barriers between two layers hide that latency (conv_mainloop_halo does the same).
template <int NT, int KC, int NB, int NM>
__device__ __forceinline__ void s3_mainloop_halo(const u32x4* __restrict__ lds4, const void* __restrict__ wlayer, const void* __restrict__ wnext,
                                                 uint32_t wlane, int wstep, const int (&addr4)[NM], f32x4 (&acc)[NT][2], S3W& w0, S3W& w1) {
    static_assert(NM >= NT, "an address for every row tile");
    constexpr int P4 = 8 * KC + 1, RS = NB + 1, ROW = 3 * KC, total = 9 * KC;
    constexpr int H1 = (NT + 1) / 2;
#define TG_S3_OFF(step) (((step) / KC) * P4 + ((step) % KC) * 8)
#define TG_S3_MFMA(J0, J1)                                                                                              \
    _Pragma("unroll") for (int j = J0; j < J1; j++) {                                                                   \
        acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w0.h0), as_bf(ah[j]), acc[j][0], 0, 0, 0);            \
        acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w0.h1), as_bf(ah[j]), acc[j][1], 0, 0, 0);            \
    }                                                                                                                   \
    _Pragma("unroll") for (int j = J0; j < J1; j++) {                                                                   \
        acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w0.h0), as_bf(al[j]), acc[j][0], 0, 0, 0);            \
        acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w0.h1), as_bf(al[j]), acc[j][1], 0, 0, 0);            \
    }                                                                                                                   \
    _Pragma("unroll") for (int j = J0; j < J1; j++) {                                                                   \
        acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w0.l0), as_bf(ah[j]), acc[j][0], 0, 0, 0);            \
        acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w0.l1), as_bf(ah[j]), acc[j][1], 0, 0, 0);            \
    }
    int ad[NT];
    u32x4 ah[NT], al[NT];
#pragma unroll
    for (int j = 0; j < NT; j++) ad[j] = addr4[j];
#pragma unroll
    for (int j = 0; j < H1; j++) { ah[j] = lds4[ad[j] + TG_S3_OFF(0)]; al[j] = lds4[ad[j] + TG_S3_OFF(0) + 4]; }
    int wchunk = 2;  // next step of weights to request
#pragma unroll 1
    for (int dy = 0; dy < 3; dy++) {
#pragma unroll
        for (int s = 0; s < ROW; s++) {
#pragma unroll
            for (int j = H1; j < NT; j++) { ah[j] = lds4[ad[j] + TG_S3_OFF(s)]; al[j] = lds4[ad[j] + TG_S3_OFF(s) + 4]; }
            __builtin_amdgcn_sched_barrier(0);
            TG_S3_MFMA(0, H1)
            __builtin_amdgcn_sched_barrier(0);
            S3W w2;
            if (s < ROW - 2) {
                w2 = s3_load_w(wlayer, total * wstep, wlane, wchunk * wstep);
            } else {  // the last two steps of a row of taps — of the layer when dy = 2: on to the next layer's first steps
                const bool on = dy == 2;
                w2 = s3_load_w(on ? wnext : wlayer, total * wstep, wlane, (on ? s - (ROW - 2) : wchunk) * wstep);
            }
            wchunk++;
            if (s + 1 < ROW) {
#pragma unroll
                for (int j = 0; j < H1; j++) { ah[j] = lds4[ad[j] + TG_S3_OFF(s + 1)]; al[j] = lds4[ad[j] + TG_S3_OFF(s + 1) + 4]; }
            } else {
                // row switch: the second half's fragments of this step are in registers or in flight with the old addresses
#pragma unroll
                for (int j = H1; j < NT; j++) ad[j] += RS * P4;
                if (dy < 2) {
#pragma unroll
                    for (int j = 0; j < H1; j++) { ad[j] += RS * P4; ah[j] = lds4[ad[j] + TG_S3_OFF(0)]; al[j] = lds4[ad[j] + TG_S3_OFF(0) + 4]; }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            TG_S3_MFMA(H1, NT)
            __builtin_amdgcn_sched_barrier(0);
            w0 = w1;
            w1 = w2;
        }
    }
#undef TG_S3_MFMA
#undef TG_S3_OFF
}

// RTW: row tiles of a full row group; NRG row groups × NCG channel groups (of 2 tiles) = NW waves.  With NW = 4 two
// workgroups share a CU (one wave of each per SIMD): they drift apart, so one's epilogue / barrier phases overlap the other's MFMAs.
// (the second launch bound caps the 4-wave variant at 256 registers so that two of its workgroups fit on a CU)
// CB (with FROM_STATES, KC0 = 1): layer 0 over the board planes only, the constant planes as the per-position bias PB (tower_stage.cuh)
template <int RTW, int KC0, int KC, bool FROM_STATES, bool OUT_SPLIT, int NW, bool CB = false>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void k_tower_s3(const void* __restrict__ in, TowerS3Params T, float* __restrict__ out, int B, int n,
                                                  int PW, int NCG, int pad0) {
    static_assert(!CB || (FROM_STATES && KC0 == 1), "the constant-plane bias needs the packed states and one chunk of board planes");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4* lds4 = (u32x4*)lds;
    const int tid = threadIdx.x;
    const int nsq = n * n;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int rows = npos * nsq;
    const int F = T.F;
    const int wave = tid >> 6, lane = tid & 63;
    const int cg = wave % NCG, rg = wave / NCG;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = cg * 32;

    // ---- stage the input: CP0 = 32·KC0 channels per row, hi/lo split ----
    constexpr int CP0 = 32 * KC0;
    int LS4 = (CP0 >> 2) + pad0;  // pad0 = 2 (conflict free) when the input image fits, else 1
    // CB: PB[position][class][F] (f32) behind the image and its zero region
    f32x4* pb4 = (f32x4*)(lds4 + (size_t)(((PW * nsq + n + 1 + 15) & ~15) + 16 + n + 1) * LS4);
    if (CB) {
        const Geom geo = make_geom(n);
        const uint8_t* states = (const uint8_t*)in;
        // a wave's positions are requested two at a time (tower_stage_states_cb, tower_kernels.hip)
        auto stage_one = [&](int p, const WRaw& raw) {
            WState ws;
            ws_unpack(ws, raw, geo);
            const float fcd = fcd_value(ws, geo);
            const RowMask m = ws_row_mask(ws, geo);
            if (lane < nsq) {
                u32x4* row = lds4 + (size_t)(p * nsq + lane) * LS4;
                f32x4 qd[8];
                tower_cb_board_quads(m, n, qd);
#pragma unroll
                for (int g8 = 0; g8 < 4; g8++) {  // 0 / 1 values: the lo halves are zero
                    u32x2 h0, l0, h1, l1;
                    split4(qd[2 * g8], h0, l0);
                    split4(qd[2 * g8 + 1], h1, l1);
                    row[g8] = u32x4{h0[0], h0[1], h1[0], h1[1]};
                    row[4 + g8] = u32x4{l0[0], l0[1], l1[0], l1[1]};
                }
            }
            tower_cb_table(ws, fcd, n, p, T.F >> 2, (const f32x4*)T.cplane_sums, (const f32x4*)T.b[0], pb4);
        };
        for (int p = wave; p < npos; p += 2 * NW) {
            const int p1 = p + NW;
            const WRaw r0 = ws_load_raw(states + (size_t)(pos0 + p) * geo.bytes, geo);
            const WRaw r1 = ws_load_raw(states + (size_t)(pos0 + (p1 < npos ? p1 : p)) * geo.bytes, geo);
            stage_one(p, r0);
            if (p1 < npos) stage_one(p1, r1);
        }
    } else if (FROM_STATES) {
        const Geom geo = make_geom(n);
        const uint8_t* states = (const uint8_t*)in;
        const int C = input_channels(n);
        for (int p = wave; p < npos; p += NW) {  // one wave encodes one position at a time, lane = square
            WState ws;
            ws_load(ws, states + (size_t)(pos0 + p) * geo.bytes, geo);
            const float fcd = fcd_value(ws, geo);
            const RowMask m = ws_row_mask(ws, geo);
            if (lane < nsq) {
                u32x4* row = lds4 + (size_t)(p * nsq + lane) * LS4;
                for (int g8 = 0; g8 < (CP0 >> 3); g8++) {
                    float4 a = row_mask_value(m, 2 * g8, C, fcd), b = row_mask_value(m, 2 * g8 + 1, C, fcd);
                    u32x2 h0, l0, h1, l1;
                    split4(f32x4{a.x, a.y, a.z, a.w}, h0, l0);
                    split4(f32x4{b.x, b.y, b.z, b.w}, h1, l1);
                    row[(g8 >> 2) * 8 + (g8 & 3)] = u32x4{h0[0], h0[1], h1[0], h1[1]};
                    row[(g8 >> 2) * 8 + 4 + (g8 & 3)] = u32x4{l0[0], l0[1], l1[0], l1[1]};
                }
            }
        }
    } else {
        const float* planes = (const float*)in;  // NHWC f32 rows of T.cin_pad channels
        const int cin = T.cin_pad;
        const int groups = CP0 >> 3;
        for (int idx = tid; idx < rows * groups; idx += NW * 64) {
            int r = idx / groups, g8 = idx - r * groups;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
            const float* src = planes + ((size_t)pos0 * nsq + r) * cin + 8 * g8;
            if (8 * g8 < cin) a = *(const f32x4*)src;
            if (8 * g8 + 4 < cin) b = *(const f32x4*)(src + 4);
            u32x2 h0, l0, h1, l1;
            split4(a, h0, l0);
            split4(b, h1, l1);
            lds4[r * LS4 + (g8 >> 2) * 8 + (g8 & 3)] = u32x4{h0[0], h0[1], h1[0], h1[1]};
            lds4[r * LS4 + (g8 >> 2) * 8 + 4 + (g8 & 3)] = u32x4{l0[0], l0[1], l1[0], l1[1]};
        }
    }
    // zero rows: a region [zb - (n+1), zb + 16 + n + 1) addressed like the image (see s3_mainloop) when it fits next to
    // the input image (pad0 == 2), else the single row `rows`
    const int zb = (rows + n + 1 + 15) & ~15;
    const int zlo = zb - (n + 1), zcount = 16 + 2 * (n + 1);
    const bool zregion0 = pad0 == 2;
    if (zregion0) {
        for (int idx = tid; idx < zcount * LS4; idx += NW * 64) lds4[zlo * LS4 + idx] = u32x4{0u, 0u, 0u, 0u};
    } else {
        for (int idx = tid; idx < LS4; idx += NW * 64) lds4[rows * LS4 + idx] = u32x4{0u, 0u, 0u, 0u};
    }
    __syncthreads();

    const int rho0 = rg * RTW * 16 + r16;
    int vmask[RTW];
    conv_tap_masks<RTW>(rows, n, nsq, rho0, vmask);
    const bool short_group = (rg * RTW + RTW - 1) * 16 >= rows && RTW > 1;

    f32x4 acc[RTW][2];
#pragma unroll
    for (int j = 0; j < RTW; j++) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int layer = 0; layer < T.nlayers; layer++) {
        // this lane's weight slots: [chunk][channel tile][hi|lo][q][cout in tile] in 16-byte units — a fragment load is one
        // contiguous KB per wave
        const u32x4* wp = (const u32x4*)(CB && layer == 0 ? T.w0_board : T.w[layer]) + (size_t)(ch0 >> 4) * 128 + q * 16 + r16;
        const int t1 = 128, wstride = (F >> 4) * 128;
        const bool zregion = layer > 0 || zregion0;
        const int zrow = zregion ? zb + r16 : rows, zshift = zregion ? 1 : 0;
        if (short_group) {
            f32x4 (&acs)[RTW - 1][2] = *reinterpret_cast<f32x4 (*)[RTW - 1][2]>(&acc[0][0]);
            if (layer == 0) s3_mainloop<RTW - 1, KC0>(lds4, wp, t1, wstride, LS4, zrow, zshift, n, rho0, q, vmask, acs);
            else s3_mainloop<RTW - 1, KC>(lds4, wp, t1, wstride, LS4, zrow, zshift, n, rho0, q, vmask, acs);
        } else {
            if (layer == 0) s3_mainloop<RTW, KC0>(lds4, wp, t1, wstride, LS4, zrow, zshift, n, rho0, q, vmask, acc);
            else s3_mainloop<RTW, KC>(lds4, wp, t1, wstride, LS4, zrow, zshift, n, rho0, q, vmask, acc);
        }
        // ---- epilogue: lane holds out[row rho0 + 16j][ch0 + 16t + 4q .. +3] ----
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const f32x4 bv = *(const f32x4*)&T.b[layer][ch0 + 8 * q + 4 * t];
#pragma unroll
            for (int j = 0; j < RTW; j++) {
                acc[j][t] = relu4(acc[j][t] + ((CB && layer == 0) ? pb4[tower_cb_index(rho0 + j * 16, rows, n, nsq, F >> 2, (ch0 + 8 * q + 4 * t) >> 2)] : bv));
            }
        }
        if (layer + 1 == T.nlayers && !OUT_SPLIT) {
#pragma unroll
            for (int j = 0; j < RTW; j++)
                if (rho0 + j * 16 < rows) {
                    float* o = out + ((size_t)pos0 * nsq + rho0 + j * 16) * F + ch0 + 4 * q;
                    *(f32x4*)o = acc[j][0];
                    *(f32x4*)(o + 16) = acc[j][1];
                }
            break;
        }
        __syncthreads();  // every wave has finished reading the previous image
        const int LS4n = (F >> 2) + 2;
        const bool conv1 = (layer & 1) == 1;  // next layer is conv2 of the same block: it starts from the block input
        // 8-byte half-slot of (row, channel c = ch0 + 8q + 4t — see upload_conv_s3 for the order of a wave's 32 output channels):
        // chunk c>>5, slot (c&31)>>3 = q (hi) / 4 + q (lo), half (c&7)>>2 = t
        f32x4 nxt[RTW][2];
#pragma unroll
        for (int j = 0; j < RTW; j++)
#pragma unroll
            for (int t = 0; t < 2; t++) {
                nxt[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (conv1 && rho0 + j * 16 < rows) {
                    const int c = ch0 + 8 * q + 4 * t;
                    const u32x2* p = (const u32x2*)(lds4 + (size_t)(rho0 + j * 16) * LS4n + (c >> 5) * 8 + ((c & 31) >> 3)) + ((c & 7) >> 2);
                    nxt[j][t] = join4(p[0], p[8]);  // hi slot, lo slot (+4 slots = 64 B)
                }
            }
        LS4 = LS4n;
#pragma unroll
        for (int j = 0; j < RTW; j++)
#pragma unroll
            for (int t = 0; t < 2; t++)
                if (rho0 + j * 16 < rows) {
                    const int c = ch0 + 8 * q + 4 * t;
                    u32x2 hi, lo;
                    split4(acc[j][t], hi, lo);
                    u32x2* p = (u32x2*)(lds4 + (size_t)(rho0 + j * 16) * LS4 + (c >> 5) * 8 + ((c & 31) >> 3)) + ((c & 7) >> 2);
                    p[0] = hi;
                    p[8] = lo;
                }
        if (layer == 0)  // the zero region in the pitch of the F-channel image (it lies behind the image rows)
            for (int idx = tid; idx < zcount * LS4; idx += NW * 64) lds4[zlo * LS4 + idx] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < RTW; j++) { acc[j][0] = nxt[j][0]; acc[j][1] = nxt[j][1]; }
        __syncthreads();
        if (OUT_SPLIT && layer + 1 == T.nlayers) {
            // the image now holds the final activations in the split row layout the split FC reads: copy it out, 16 B per lane
            const int spr = F >> 2;  // slots per row without the pad
            u32x4* o = (u32x4*)out + (size_t)pos0 * nsq * spr;
            for (int idx = tid; idx < rows * spr; idx += NW * 64) {
                int r = idx / spr, v = idx - r * spr;
                o[idx] = lds4[r * LS4 + v];
            }
            // conv policy head (net6.rs:56,98-103) as one more 3×3 convolution over the resident image: F → head_cout
            // channels in passes of NCG channel groups, bias only, f32 logits [position][square][head_cout] to global
            if (T.head_w) {
                const bool zregion = T.nlayers > 1 || zregion0;
                const int zrow = zregion ? zb + r16 : rows, zshift = zregion ? 1 : 0;
                const int hstride = (T.head_cout >> 4) * 128;
                for (int hc0 = cg * 32; hc0 < T.head_cout; hc0 += NCG * 32) {
#pragma unroll
                    for (int j = 0; j < RTW; j++) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const u32x4* wp = (const u32x4*)T.head_w + (size_t)(hc0 >> 4) * 128 + q * 16 + r16;
                    if (short_group) {
                        f32x4 (&acs)[RTW - 1][2] = *reinterpret_cast<f32x4 (*)[RTW - 1][2]>(&acc[0][0]);
                        s3_mainloop<RTW - 1, KC>(lds4, wp, 128, hstride, LS4, zrow, zshift, n, rho0, q, vmask, acs);
                    } else {
                        s3_mainloop<RTW, KC>(lds4, wp, 128, hstride, LS4, zrow, zshift, n, rho0, q, vmask, acc);
                    }
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const f32x4 bv = *(const f32x4*)&T.head_b[hc0 + 8 * q + 4 * t];
#pragma unroll
                        for (int j = 0; j < RTW; j++)
                            if (rho0 + j * 16 < rows)
                                *(f32x4*)&T.head_out[((size_t)pos0 * nsq + rho0 + j * 16) * T.head_cout + hc0 + 8 * q + 4 * t] = acc[j][t] + bv;
                    }
                }
            }
            break;
        }
    }
}


// ------------------------------------------------------------------------------------------------
// k_tower_s3 on the halo image (full batches): layer 0 on the plain split image with the masked loop, then the
// F-channel image in halo cells — see k_tower_halo (tower_kernels.hip) for the layout, the slot table and why.
// Same products in the same order as k_tower_s3 → identical bits.
// ------------------------------------------------------------------------------------------------
template <int RTW, int KC0, int KC, int NB, bool FROM_STATES, bool OUT_SPLIT, int NW, bool CB = false>
__global__ __launch_bounds__(NW * 64, NW == 4 ? 2 : 1) void k_tower_s3_halo(const void* __restrict__ in, TowerS3Params T, float* __restrict__ out,
                                                                          int B, int PW, int NCG) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    u32x4* lds4 = (u32x4*)lds;
    constexpr int n = NB, nsq = NB * NB, RS = NB + 1, LEAD = NB + 2, F = 32 * KC, P4 = 8 * KC + 1;
    const int PS = T.halo_ps;
    const int tid = threadIdx.x;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int rows = npos * nsq;
    const int wave = tid >> 6, lane = tid & 63;
    const int cg = wave % NCG, rg = wave / NCG;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = cg * 32;

    TG_S3_STAMP(0, 6);
    // ---- stage the input: plain image, CP0 = 32·KC0 channels per row, hi/lo split, pitch + 16 B, one zero row ----
    constexpr int CP0 = 32 * KC0;
    constexpr int LS4 = (CP0 >> 2) + 1;
    static_assert(!CB || (FROM_STATES && KC0 == 1), "the constant-plane bias needs the packed states and one chunk of board planes");
    f32x4* pb4 = (f32x4*)(lds4 + (size_t)(PW * nsq + 1) * LS4);  // CB: PB[position][class][F] (f32) behind the image and its zero row
    if (CB) {
        const Geom geo = make_geom(n);
        const uint8_t* states = (const uint8_t*)in;
        // a wave's positions are requested two at a time (tower_stage_states_cb, tower_kernels.hip)
        auto stage_one = [&](int p, const WRaw& raw) {
            WState ws;
            ws_unpack(ws, raw, geo);
            const float fcd = fcd_value(ws, geo);
            const RowMask m = ws_row_mask(ws, geo);
            if (lane < nsq) {
                u32x4* row = lds4 + (size_t)(p * nsq + lane) * LS4;
                f32x4 qd[8];
                tower_cb_board_quads(m, n, qd);
#pragma unroll
                for (int g8 = 0; g8 < 4; g8++) {  // 0 / 1 values: the lo halves are zero
                    u32x2 h0, l0, h1, l1;
                    split4(qd[2 * g8], h0, l0);
                    split4(qd[2 * g8 + 1], h1, l1);
                    row[g8] = u32x4{h0[0], h0[1], h1[0], h1[1]};
                    row[4 + g8] = u32x4{l0[0], l0[1], l1[0], l1[1]};
                }
            }
            tower_cb_table(ws, fcd, n, p, F >> 2, (const f32x4*)T.cplane_sums, (const f32x4*)T.b[0], pb4);
        };
        for (int p = wave; p < npos; p += 2 * NW) {
            const int p1 = p + NW;
            const WRaw r0 = ws_load_raw(states + (size_t)(pos0 + p) * geo.bytes, geo);
            const WRaw r1 = ws_load_raw(states + (size_t)(pos0 + (p1 < npos ? p1 : p)) * geo.bytes, geo);
            stage_one(p, r0);
            if (p1 < npos) stage_one(p1, r1);
        }
    } else if (FROM_STATES) {
        const Geom geo = make_geom(n);
        const uint8_t* states = (const uint8_t*)in;
        const int C = input_channels(n);
        for (int p = wave; p < npos; p += NW) {
            WState ws;
            ws_load(ws, states + (size_t)(pos0 + p) * geo.bytes, geo);
            const float fcd = fcd_value(ws, geo);
            const RowMask m = ws_row_mask(ws, geo);
            if (lane < nsq) {
                u32x4* row = lds4 + (size_t)(p * nsq + lane) * LS4;
                for (int g8 = 0; g8 < (CP0 >> 3); g8++) {
                    float4 a = row_mask_value(m, 2 * g8, C, fcd), b = row_mask_value(m, 2 * g8 + 1, C, fcd);
                    u32x2 h0, l0, h1, l1;
                    split4(f32x4{a.x, a.y, a.z, a.w}, h0, l0);
                    split4(f32x4{b.x, b.y, b.z, b.w}, h1, l1);
                    row[(g8 >> 2) * 8 + (g8 & 3)] = u32x4{h0[0], h0[1], h1[0], h1[1]};
                    row[(g8 >> 2) * 8 + 4 + (g8 & 3)] = u32x4{l0[0], l0[1], l1[0], l1[1]};
                }
            }
        }
    } else {
        const float* planes = (const float*)in;
        const int cin = T.cin_pad;
        const int groups = CP0 >> 3;
        for (int idx = tid; idx < rows * groups; idx += NW * 64) {
            int r = idx / groups, g8 = idx - r * groups;
            f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f}, b = a;
            const float* src = planes + ((size_t)pos0 * nsq + r) * cin + 8 * g8;
            if (8 * g8 < cin) a = *(const f32x4*)src;
            if (8 * g8 + 4 < cin) b = *(const f32x4*)(src + 4);
            u32x2 h0, l0, h1, l1;
            split4(a, h0, l0);
            split4(b, h1, l1);
            lds4[r * LS4 + (g8 >> 2) * 8 + (g8 & 3)] = u32x4{h0[0], h0[1], h1[0], h1[1]};
            lds4[r * LS4 + (g8 >> 2) * 8 + 4 + (g8 & 3)] = u32x4{l0[0], l0[1], l1[0], l1[1]};
        }
    }
    for (int idx = tid; idx < LS4; idx += NW * 64) lds4[rows * LS4 + idx] = u32x4{0u, 0u, 0u, 0u};
    __syncthreads();

    TG_S3_STAMP(0, 0);
    // row tiles dealt to the row groups as evenly as they go (k_tower_halo)
    const int NRG = NW / NCG;
    const int ntiles = (PW * nsq + 15) >> 4;
    const int tbase = ntiles / NRG, trem = ntiles - tbase * NRG;
    const int my_tiles = tbase + (rg < trem ? 1 : 0);
    const int tile0 = rg * tbase + min(rg, trem);
    const bool short_group = my_tiles < RTW;

    f32x4 acc[RTW][2];
#pragma unroll
    for (int j = 0; j < RTW; j++) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int t1 = 128, wstride = (F >> 4) * 128;

    const uint32_t wlane = (uint32_t)(((ch0 >> 4) * 128 + q * 16 + r16) * 16);  // this lane's 16 B inside a step of a layer's weights
    S3W w0, w1;  // the weight stream's two steps in flight between layers
    w0.h0 = w0.l0 = w0.h1 = w0.l1 = u32x4{0u, 0u, 0u, 0u};
    w1 = w0;

    // ---- layer 0 on the plain image: tile t = rows 16t … 16t + 15 ----
    {
        const int rho0 = tile0 * 16 + r16;
        int vmask[RTW];
        conv_tap_masks<RTW>(rows, n, nsq, rho0, vmask);
        if (short_group) vmask[RTW - 1] = 0;
        const u32x4* wp = (const u32x4*)(CB ? T.w0_board : T.w[0]) + (size_t)(ch0 >> 4) * 128 + q * 16 + r16;
        if (RTW > 1 && short_group) {
            f32x4 (&acs)[RTW - 1][2] = *reinterpret_cast<f32x4 (*)[RTW - 1][2]>(&acc[0][0]);
            s3_mainloop<RTW - 1, KC0>(lds4, wp, t1, wstride, LS4, rows, 0, n, rho0, q, vmask, acs);
        } else {
            s3_mainloop<RTW, KC0>(lds4, wp, t1, wstride, LS4, rows, 0, n, rho0, q, vmask, acc);
        }
        TG_S3_STAMP(0, 1);
        if (T.nlayers > 1) {  // in flight during the change of images
            w0 = s3_load_w(T.w[1], 9 * KC * wstride * 16, wlane, 0);
            w1 = s3_load_w(T.w[1], 9 * KC * wstride * 16, wlane, wstride * 16);
        }
#pragma unroll
        for (int t = 0; t < 2; t++) {
            const f32x4 bv = *(const f32x4*)&T.b[0][ch0 + 8 * q + 4 * t];
#pragma unroll
            for (int j = 0; j < RTW; j++) {
                acc[j][t] = relu4(acc[j][t] + (CB ? pb4[tower_cb_index(rho0 + j * 16, rows, n, nsq, F >> 2, (ch0 + 8 * q + 4 * t) >> 2)] : bv));
            }
        }
        TG_S3_STAMP(0, 2);
        __syncthreads();  // every wave has finished reading the input image
        TG_S3_STAMP(0, 3);
        const int cells = LEAD + PW * PS + 1;  // + the spare cell of the idle slots
        for (int idx = tid; idx < cells * P4; idx += NW * 64) {
            const int c = idx / P4 - LEAD;
            const int o = c < 0 || c >= PW * PS ? n * RS : c % PS;
            if (o >= n * RS || o % RS == n) lds4[idx] = u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int j = 0; j < RTW; j++) {
            const int rho = rho0 + j * 16;
            if (j < my_tiles && rho < PW * nsq) {
                const int p = rho / nsq, sq = rho - p * nsq, y = sq / n, x = sq - y * n;
                const int cell = LEAD + p * PS + y * RS + x;
                u32x2 h0, l0, h1, l1;
                split4(acc[j][0], h0, l0);
                split4(acc[j][1], h1, l1);
                u32x4* sp = lds4 + (size_t)cell * P4 + cg * 8 + q;
                sp[0] = u32x4{h0[0], h0[1], h1[0], h1[1]};
                sp[4] = u32x4{l0[0], l0[1], l1[0], l1[1]};
            }
            acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        TG_S3_STAMP(0, 4);
        __syncthreads();
        TG_S3_STAMP(0, 5);
    }
    if (T.nlayers == 1) return;  // (never: a tower has at least one block)

    // ---- layers 1 … : slot (tile, lane) → square through the slot table ----
    // idle slots (no square left for them) read the zero cell of position 0 and write a spare cell behind the image, so that
    // the epilogue needs no per-tile branches (each would wait out its own LDS round trip)
    int rowid[RTW], addr4[RTW], wb[RTW];  // wb: byte address of this lane's hi slot (its 8 output channels) in its cell
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        const uint32_t e = j < my_tiles ? T.slotmap[(tile0 + j) * 16 + r16] : 0xFFFF0000u;
        rowid[j] = (int)(e >> 16);
        const bool idle = rowid[j] == 0xFFFF;
        addr4[j] = ((idle ? LEAD + n * RS : (int)(e & 0xFFFFu)) - LEAD) * P4 + q;
        wb[j] = ((idle ? LEAD + PW * PS : (int)(e & 0xFFFFu)) * P4 + cg * 8 + q) * 16;
    }
    char* const ldsb = (char*)lds;
    for (int layer = 1; layer < T.nlayers; layer++) {
        TG_S3_STAMP(layer, 0);
#pragma unroll
        for (int j = 0; j < RTW; j++) asm volatile("" : "+v"(addr4[j]), "+v"(wb[j]));  // keep the compiler from hoisting address sums out of the layer loop
        const void* wnext = T.w[layer + 1 < T.nlayers ? layer + 1 : layer];
        f32x4 bv[2];  // requested here: the latency passes under the main loop
#pragma unroll
        for (int t = 0; t < 2; t++) bv[t] = *(const f32x4*)&T.b[layer][ch0 + 8 * q + 4 * t];
        if (RTW > 1 && short_group) {
            f32x4 (&acs)[RTW - 1][2] = *reinterpret_cast<f32x4 (*)[RTW - 1][2]>(&acc[0][0]);
            s3_mainloop_halo<RTW - 1, KC, NB>(lds4, T.w[layer], wnext, wlane, wstride * 16, addr4, acs, w0, w1);
        } else {
            s3_mainloop_halo<RTW, KC, NB>(lds4, T.w[layer], wnext, wlane, wstride * 16, addr4, acc, w0, w1);
        }
        TG_S3_STAMP(layer, 1);
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int j = 0; j < RTW; j++) {
                acc[j][t] = relu4(acc[j][t] + bv[t]);
            }
        }
        if (layer + 1 == T.nlayers && !OUT_SPLIT) {
#pragma unroll
            for (int j = 0; j < RTW; j++)
                if (rowid[j] < rows) {
                    float* o = out + ((size_t)pos0 * nsq + rowid[j]) * F + ch0 + 8 * q;
                    *(f32x4*)o = acc[j][0];
                    *(f32x4*)(o + 4) = acc[j][1];
                }
            break;
        }
        TG_S3_STAMP(layer, 2);
        __syncthreads();  // every wave has finished reading the previous image
        TG_S3_STAMP(layer, 3);
        const bool conv1 = (layer & 1) == 1;  // next layer is conv2 of the same block: it starts from the block input
        // the lane's 8 channels ch0 + 8q … + 7 (tile 0: the first four, tile 1: the others) are one hi slot and one lo slot of
        // its cell — the slots the main loop reads with the same lanes, so these accesses are conflict free as well
        f32x4 nxt[RTW][2];
#pragma unroll
        for (int j = 0; j < RTW; j++) nxt[j][0] = nxt[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (conv1) {
            u32x4 sh[RTW], sl[RTW];
#pragma unroll
            for (int j = 0; j < RTW; j++) {
                sh[j] = *(const u32x4*)(ldsb + wb[j]);
                sl[j] = *(const u32x4*)(ldsb + wb[j] + 64);
            }
#pragma unroll
            for (int j = 0; j < RTW; j++) {
                nxt[j][0] = join4(u32x2{sh[j][0], sh[j][1]}, u32x2{sl[j][0], sl[j][1]});
                nxt[j][1] = join4(u32x2{sh[j][2], sh[j][3]}, u32x2{sl[j][2], sl[j][3]});
            }
        }
#pragma unroll
        for (int j = 0; j < RTW; j++) {
            u32x2 h0, l0, h1, l1;
            split4(acc[j][0], h0, l0);
            split4(acc[j][1], h1, l1);
            *(u32x4*)(ldsb + wb[j]) = u32x4{h0[0], h0[1], h1[0], h1[1]};
            *(u32x4*)(ldsb + wb[j] + 64) = u32x4{l0[0], l0[1], l1[0], l1[1]};
        }
#pragma unroll
        for (int j = 0; j < RTW; j++) { acc[j][0] = nxt[j][0]; acc[j][1] = nxt[j][1]; }
        TG_S3_STAMP(layer, 4);
        __syncthreads();
        TG_S3_STAMP(layer, 5);
        if (OUT_SPLIT && layer + 1 == T.nlayers) {
            // the image holds the final activations in the split cell layout: copy the real cells out row by row, 16 B per lane
            const int spr = F >> 2;
            u32x4* o = (u32x4*)out + (size_t)pos0 * nsq * spr;
            for (int idx = tid; idx < rows * spr; idx += NW * 64) {
                const int r = idx / spr, v = idx - r * spr;
                const int p = r / nsq, sq = r - p * nsq, y = sq / n, x = sq - y * n;
                o[idx] = lds4[(size_t)(LEAD + p * PS + y * RS + x) * P4 + v];
            }
            if (T.head_w) {  // conv policy head as one more 3×3 convolution over the resident image (k_tower_s3)
                const int hstride = (T.head_cout >> 4) * 128;
                for (int hc0 = cg * 32; hc0 < T.head_cout; hc0 += NCG * 32) {
#pragma unroll
                    for (int j = 0; j < RTW; j++) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const uint32_t hlane = (uint32_t)(((hc0 >> 4) * 128 + q * 16 + r16) * 16);
#pragma unroll
                    for (int j = 0; j < RTW; j++) asm volatile("" : "+v"(addr4[j]));
                    w0 = s3_load_w(T.head_w, 9 * KC * hstride * 16, hlane, 0);
                    w1 = s3_load_w(T.head_w, 9 * KC * hstride * 16, hlane, hstride * 16);
                    if (RTW > 1 && short_group) {
                        f32x4 (&acs)[RTW - 1][2] = *reinterpret_cast<f32x4 (*)[RTW - 1][2]>(&acc[0][0]);
                        s3_mainloop_halo<RTW - 1, KC, NB>(lds4, T.head_w, T.head_w, hlane, hstride * 16, addr4, acs, w0, w1);
                    } else {
                        s3_mainloop_halo<RTW, KC, NB>(lds4, T.head_w, T.head_w, hlane, hstride * 16, addr4, acc, w0, w1);
                    }
#pragma unroll
                    for (int t = 0; t < 2; t++) {
                        const f32x4 bv = *(const f32x4*)&T.head_b[hc0 + 8 * q + 4 * t];
#pragma unroll
                        for (int j = 0; j < RTW; j++)
                            if (rowid[j] < rows)
                                *(f32x4*)&T.head_out[((size_t)pos0 * nsq + rowid[j]) * T.head_cout + hc0 + 8 * q + 4 * t] = acc[j][t] + bv;
                    }
                }
            }
            break;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Policy FC (net5.rs:56-61,108) on split operands: logits[M][N] = S[M][K]·W[K][N] + b with S in the split row
// layout the tower writes.  NW waves, each 2 position tiles × all CT output tiles (NW·32 positions × CT·16 outputs per
// workgroup): a wave's weight fragment (LDS) feeds 2 position tiles × 3 MFMAs.  Weights are staged global → LDS per
// K-step of 64, double buffered, in planes [chunk][q][hi|lo][CT·16] of 16-byte slots (a quarter-wave reads 16 consecutive
// slots: conflict free); the activations are the MFMA B operand straight from global.  CT = 7, NW = 4 needs 57 KB of LDS,
// so two workgroups share a CU and one's staging / barrier phases overlap the other's MFMAs; nothing is loaded twice by a
// workgroup.
// stats (optional): the block-wise softmax statistics of softmax.cuh over this workgroup's CT·16 columns, per row:
// stats[(row·blocks + block)·2] = {max, Σ exp(x − max)} of the columns < n_soft — what the tree backup and k_softmax_stats combine
template <int CT, int NW>
__global__ __launch_bounds__(NW * 64) void k_fc_s3b(const u32x4* __restrict__ A, const u32x4* __restrict__ Wp, const float* __restrict__ bias,
                                                    float* __restrict__ out, int M, int K, int NP, int out_stride, int n_valid,
                                                    float* __restrict__ stats, int n_soft) {
    constexpr int COLS = CT * 16, SLOTS = 2 * 4 * 2 * COLS, NT = NW * 64, PER = (SLOTS + NT - 1) / NT;
    __shared__ u32x4 wl[2][SLOTS];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const int r16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.y * COLS;
    const int rpitch = K >> 2;
    int row[2];
    bool row_ok[2];
    const u32x4* ap[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        row[p] = blockIdx.x * (NW * 32) + wave * 32 + p * 16 + r16;
        row_ok[p] = row[p] < M;
        ap[p] = A + (size_t)(row_ok[p] ? row[p] : M - 1) * rpitch + q;
    }
    const int nsteps = K / 64;
    const int ncb = NP / COLS;
    auto stage_load = [&](int step, u32x4 (&r)[PER]) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            int idx = u * NT + tid;
            idx = idx < SLOTS ? idx : SLOTS - 1;
            int c = idx / (COLS * 8), rem = idx - c * (COLS * 8);
            r[u] = Wp[((size_t)(step * 2 + c) * ncb + blockIdx.y) * (COLS * 8) + rem];
        }
    };
    auto stage_store = [&](int buf, const u32x4 (&r)[PER]) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            int idx = u * NT + tid;
            if (idx < SLOTS) wl[buf][idx] = r[u];
        }
    };
    f32x4 acc[2][CT];
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int j = 0; j < CT; j++) acc[p][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 stg[PER];
    stage_load(0, stg);
    stage_store(0, stg);
    u32x4 ac[2][2][2], an[2][2][2];
    auto load_a = [&](int step, u32x4 (&a)[2][2][2]) {
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int p = 0; p < 2; p++) {
                a[c][p][0] = ap[p][(step * 2 + c) * 8];
                a[c][p][1] = ap[p][(step * 2 + c) * 8 + 4];
            }
    };
    load_a(0, ac);
    __syncthreads();
    for (int step = 0; step < nsteps; step++) {
        const int buf = step & 1;
        const int nx = step + 1 < nsteps ? step + 1 : step;
        stage_load(nx, stg);
        load_a(nx, an);
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const u32x4* wh = &wl[buf][((c * 4 + q) * 2 + 0) * COLS + r16];
            const u32x4* wo = &wl[buf][((c * 4 + q) * 2 + 1) * COLS + r16];
            u32x4 w_h[CT], w_l[CT];
#pragma unroll
            for (int j = 0; j < CT; j++) { w_h[j] = wh[j * 16]; w_l[j] = wo[j * 16]; }
#pragma unroll
            for (int j = 0; j < CT; j++) {
#pragma unroll
                for (int p = 0; p < 2; p++) acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w_h[j]), as_bf(ac[c][p][0]), acc[p][j], 0, 0, 0);
#pragma unroll
                for (int p = 0; p < 2; p++) acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w_h[j]), as_bf(ac[c][p][1]), acc[p][j], 0, 0, 0);
#pragma unroll
                for (int p = 0; p < 2; p++) acc[p][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(w_l[j]), as_bf(ac[c][p][0]), acc[p][j], 0, 0, 0);
            }
        }
        stage_store(buf ^ 1, stg);
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int p = 0; p < 2; p++) { ac[c][p][0] = an[c][p][0]; ac[c][p][1] = an[c][p][1]; }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 2; p++) {
        f32x4 v[CT];
#pragma unroll
        for (int j = 0; j < CT; j++) v[j] = acc[p][j] + *(const f32x4*)&bias[n0 + j * 16 + 4 * q];  // (bias holds NP entries)
        if (row_ok[p]) {
#pragma unroll
            for (int j = 0; j < CT; j++) {
                const int nn = n0 + j * 16 + 4 * q;
                if (nn < n_valid) {
                    float* o = out + (size_t)row[p] * out_stride + nn;
                    if (nn + 3 < n_valid) *(f32x4*)o = v[j];
                    else for (int t = 0; t < 4; t++) if (nn + t < n_valid) o[t] = v[j][t];
                }
            }
        }
        if (stats) {
            float m, sm;
            fc_block_stats<CT>(v, n0 + 4 * q, n_soft, m, sm);
            if (row_ok[p] && q == 0) *(float2*)&stats[((size_t)row[p] * gridDim.y + blockIdx.y) * 2] = make_float2(m, sm);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// k_fc_s3_ring (round 4) — the policy FC on split operands with k_fc_ring's structure (fc_kernels.hip): 128 rows × (12 main + 1
// leftover) output tiles per workgroup, 32 × 8 workgroups, the 99 tiles and the statistics geometry of softmax.cuh, the weights
// of a K-step of 64 (2 chunks of 32 × 13 tile slots × hi | lo = 52 blocks of 1 KB) through a three-buffer LDS-DMA ring with flag
// counters, statistics + value pre-activation + logits rows or the children's logits from the epilogue.  What differs:
// `v_mfma_f32_16x16x32_bf16`, three per product, and ALL EIGHT waves (two per SIMD, one row tile each — the shipped TG_FSR_NW = 8:
// 62 – 66 µs) issue the refills: at the bf16 rate a K-step's MFMAs are no longer than a refill's 13 pieces, so leaving the refills to the
// younger wave of every SIMD, as k_fc_ring does, costs 90 µs.  (TG_FSR_NW = 4 builds the variant with FOUR waves of two row tiles each —
// a weight fragment pair then feeds 6 MFMAs and the LDS serves half the fragment reads per MFMA; measured no faster, r04_b §6.)
// Products in the order of k_fc_s3b (w_hi·a_hi, w_hi·a_lo, w_lo·a_hi per chunk, chunks ascending) → the same logits bits as k_fc_s3b, which keeps
// serving ≤ 512 rows (statistics behind it by k_fc_stats).  k_fc_s3b moved 737 MB per launch through the CUs' vector-memory ports
// (every 4-wave workgroup of 128 × 112 staged its weights through registers and read its activations straight from global: MFMA
// busy 0.36); here a CU takes in 1.33 MB of weights by LDS-DMA and 0.82 MB of activations.
// Weights: Wr[chunk of 32][tile 0 … 98][hi | lo][lane] 16-byte slots, lane = q·16 + column — a block is 1 KB in the reader's lane order.
// ------------------------------------------------------------------------------------------------------------------
#ifndef TG_FSR_NW
#define TG_FSR_NW 8
#endif
constexpr int FSR_NW = TG_FSR_NW;                           // waves per workgroup (4: one per SIMD, two row tiles each; 8: two per SIMD, one row tile each)
constexpr int FSR_RT = 8 / FSR_NW;                          // row tiles per wave
constexpr int FSR_CT = FC_MAIN_TILES + 1;                   // 13 tile slots
constexpr int FSR_BLOCKS = 2 * FSR_CT * 2;                  // 1 KB blocks per K-step: chunk × tile slot × hi|lo = 52
constexpr int FSR_SLOTS = FSR_BLOCKS * 64;                  // 3328 slots per buffer
constexpr int FSR_RING = 3;
constexpr size_t FSR_LDS = (size_t)FSR_RING * FSR_SLOTS * 16 + 2 * FSR_RING * sizeof(uint32_t);
constexpr int FSR_FILLERS = FSR_NW;                         // waves that issue the refills: all of them (see above)
constexpr int FSR_PER = (FSR_BLOCKS + FSR_FILLERS - 1) / FSR_FILLERS;  // blocks such a wave fills per K-step (13)

__global__ __launch_bounds__(FSR_NW * 64) void k_fc_s3_ring(const u32x4* __restrict__ A, const u32x4* __restrict__ Wr, const float* __restrict__ bias,
                                                            float* __restrict__ out, int M, int K, int out_stride, int n_valid,
                                                            float* __restrict__ stats, int n_soft, const FcGather gather) {
    static_assert(FSR_NW == 4 || FSR_NW == 8, "a wave's 128 / NW rows park in its share (64 / NW rows) of the two free ring buffers");
    extern __shared__ __attribute__((aligned(16))) uint32_t fsr_lds[];
    u32x4* wl = (u32x4*)fsr_lds;                                       // [FSR_RING][chunk][tile slot][hi|lo][lane]
    uint32_t* flags = (uint32_t*)(wl + FSR_RING * FSR_SLOTS);          // ready[3], done[3]
    const uint32_t ready0 = (uint32_t)(size_t)(__attribute__((address_space(3))) uint32_t*)flags;
    const uint32_t done0 = ready0 + FSR_RING * 4;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int r16 = lane & 15, q = lane >> 4;
    // (row block, column block) by XCD as in k_fc_ring (fc_kernels.hip): an XCD computes 4 column blocks × every fourth row block, so its
    // L2 fetches half of the weights and a quarter of the rows twice instead of all the weights and a quarter of the rows once
    int rbx = (int)blockIdx.x, cbx = (int)blockIdx.y;
    if ((gridDim.x & 7) == 0) {
        const int xcd = rbx & 7, j = (rbx >> 3) + (int)(gridDim.x >> 3) * cbx;
        cbx = 4 * (xcd & 1) + (j & 3);
        rbx = (xcd >> 1) + 4 * (j >> 2);
    }
    const int cb = cbx;
    const FcExtra X = fc_extra(cb);
    const bool has13 = wave < X.ne;                 // this wave also computes the leftover tile, for its row tile 0 (wave-uniform)
    const int n0 = cb * (FC_MAIN_TILES * 16);
    const int nx = (FC_MAIN_TILES * FC_MAIN_BLOCKS + X.l) * 16;
    const int rpitch = K >> 2;                      // slots per activation row: per chunk of 32, 4 hi slots then 4 lo slots
    int rt[FSR_RT], row[FSR_RT];
    bool row_ok[FSR_RT];
    const u32x4* ap[FSR_RT];
#pragma unroll
    for (int i = 0; i < FSR_RT; i++) {
        rt[i] = (wave + i * FSR_NW + X.s) & 7;      // row tile 0 of waves 0 … ne − 1 are the rows that need the leftover tile
        row[i] = rbx * 128 + rt[i] * 16 + r16;
        row_ok[i] = row[i] < M;
        ap[i] = A + (size_t)(row_ok[i] ? row[i] : M - 1) * rpitch + q;  // rows past the end load a valid row; never stored
    }
    const int nsteps = K / 64, nchunks = nsteps * 2;
    // LDS-DMA: block b = (chunk·13 + tile slot)·2 + hi|lo of a K-step goes to slots b·64 … b·64 + 63 of the buffer; wave w fills
    // blocks w, w + 4, …
    const int fwave = wave - (FSR_NW - FSR_FILLERS);  // ≥ 0: this wave issues refills (and signals ready[])
    const bool filler = fwave >= 0;
    uint32_t src0[FSR_PER];
#pragma unroll
    for (int u = 0; u < FSR_PER; u++) {
        int b = (filler ? fwave : 0) + FSR_FILLERS * u;
        b = b < FSR_BLOCKS ? b : FSR_BLOCKS - 1;
        const int h = b & 1, cj = b >> 1, c = cj / FSR_CT, j = cj - c * FSR_CT;
        const int tile = j < FC_MAIN_TILES ? cb * FC_MAIN_TILES + j : FC_MAIN_TILES * FC_MAIN_BLOCKS + X.l;
        src0[u] = (uint32_t)((((size_t)c * FC_TILES + tile) * 2 + h) * 64 + lane);
    }
    const uint32_t step_slots = 2u * FC_TILES * 2u * 64u;
    auto fill = [&](int step, int buf) {
#pragma unroll
        for (int u = 0; u < FSR_PER; u++)
            if (filler && fwave + FSR_FILLERS * u < FSR_BLOCKS)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(Wr + (size_t)step * step_slots + src0[u]),
                                                 (__attribute__((address_space(3))) void*)(wl + buf * FSR_SLOTS + (fwave + FSR_FILLERS * u) * 64), 16, 0, 0);
    };
    auto aload = [&](int i, int kc, int lo) { return ap[i][(size_t)(kc < nchunks ? kc : nchunks - 1) * 8 + 4 * lo]; };
    if (tid < 2 * FSR_RING) flags[tid] = 0u;
    __syncthreads();
    fill(0, 0);
    if (nsteps > 1) fill(1, 1);
    f32x4 acc[FSR_RT][FSR_CT];
#pragma unroll
    for (int i = 0; i < FSR_RT; i++)
#pragma unroll
        for (int j = 0; j < FSR_CT; j++) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // activations [row tile][hi, lo]: chunk 0 of the step in a0, chunk 1 in a1, chunk 0 of the next step in b0 (as k_fc_ring: requested
    // at the top of a step, forced complete before the refill is issued, so none queues behind a young LDS-DMA)
    u32x4 a0[FSR_RT][2], a1[FSR_RT][2], b0[FSR_RT][2];
#pragma unroll
    for (int i = 0; i < FSR_RT; i++) { a0[i][0] = aload(i, 0, 0); a0[i][1] = aload(i, 0, 1); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (filler) {
        fc_ring_signal(ready0);
        if (nsteps > 1) fc_ring_signal(ready0 + 4);
    }
    constexpr int H1 = 7;
    u32x4 wh[FSR_CT], wo[FSR_CT];
#define TG_FS_LOAD(C, J0, J1) _Pragma("unroll") for (int j = J0; j < J1; j++) { wh[j] = wb[(((C) * FSR_CT + j) * 2 + 0) * 64 + lane]; wo[j] = wb[(((C) * FSR_CT + j) * 2 + 1) * 64 + lane]; }
// (the three products of an accumulator — hi·hi, hi·lo, lo·hi, in that order — are issued a whole tile group apart, not back to
// back: with one row tile per wave consecutive MFMAs into the same accumulator waited out the matrix pipe's latency)
#define TG_FS_MFMA(AV, J0, J1)                                                                                                              \
    _Pragma("unroll") for (int j = J0; j < J1; j++)                                                                                         \
        _Pragma("unroll") for (int i = 0; i < FSR_RT; i++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh[j]), as_bf((AV)[i][0]), acc[i][j], 0, 0, 0); \
    _Pragma("unroll") for (int j = J0; j < J1; j++)                                                                                         \
        _Pragma("unroll") for (int i = 0; i < FSR_RT; i++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh[j]), as_bf((AV)[i][1]), acc[i][j], 0, 0, 0); \
    _Pragma("unroll") for (int j = J0; j < J1; j++)                                                                                         \
        _Pragma("unroll") for (int i = 0; i < FSR_RT; i++) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wo[j]), as_bf((AV)[i][0]), acc[i][j], 0, 0, 0);
#define TG_FS_XMFMA(AV)                                                                                                                     \
    acc[0][FC_MAIN_TILES] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh[FC_MAIN_TILES]), as_bf((AV)[0][0]), acc[0][FC_MAIN_TILES], 0, 0, 0); \
    acc[0][FC_MAIN_TILES] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wh[FC_MAIN_TILES]), as_bf((AV)[0][1]), acc[0][FC_MAIN_TILES], 0, 0, 0); \
    acc[0][FC_MAIN_TILES] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf(wo[FC_MAIN_TILES]), as_bf((AV)[0][0]), acc[0][FC_MAIN_TILES], 0, 0, 0);
#define TG_FS_CHUNK(C, AV, NEXT, EARLY)                                                                              \
    TG_FS_LOAD(C, H1, FSR_CT)                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    TG_FS_MFMA(AV, 0, H1)                                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    if (NEXT) { TG_FS_LOAD((C) + 1, 0, H1) }                                                                         \
    EARLY;                                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                                               \
    TG_FS_MFMA(AV, H1, FC_MAIN_TILES)                                                                                \
    if (has13) { TG_FS_XMFMA(AV) }                                                                                   \
    __builtin_amdgcn_sched_barrier(0);
    const volatile __attribute__((address_space(3))) uint32_t* flag_lds = (const volatile __attribute__((address_space(3))) uint32_t*)flags;
    uint32_t early_ready = 0u, early_done = 0u;
    uint32_t g_cnt[FSR_RT], g_pidx[FSR_RT][16];
#pragma unroll
    for (int i = 0; i < FSR_RT; i++) {
        g_cnt[i] = 0u;
#pragma unroll
        for (int r = 0; r < 16; r++) g_pidx[i][r] = 0u;
    }
    for (int step = 0; step < nsteps; step++) {
        const int buf = step % FSR_RING;
        const u32x4* wb = wl + buf * FSR_SLOTS;
        if ((int)__builtin_amdgcn_readfirstlane((int)early_ready) < FSR_FILLERS * (step / FSR_RING + 1))
            fc_ring_wait(ready0 + 4 * buf, (uint32_t)FSR_FILLERS * (uint32_t)(step / FSR_RING + 1));
        __builtin_amdgcn_sched_barrier(0);
        TG_FS_LOAD(0, 0, H1)
#pragma unroll
        for (int i = 0; i < FSR_RT; i++) {
            a1[i][0] = aload(i, step * 2 + 1, 0); a1[i][1] = aload(i, step * 2 + 1, 1);
            b0[i][0] = aload(i, step * 2 + 2, 0); b0[i][1] = aload(i, step * 2 + 2, 1);
        }
        if (gather.child_logit && step == nsteps - 1) {  // (no refill follows in the last step: these loads wait for nobody)
#pragma unroll
            for (int i = 0; i < FSR_RT; i++) {
                const int tile_row0 = rbx * 128 + rt[i] * 16;
                g_cnt[i] = gather.leaf_rec[2 * (size_t)min(tile_row0 + r16, M - 1) + 1];
#pragma unroll
                for (int r = 0; r < 16; r++)
                    g_pidx[i][r] = ((const uint32_t*)(gather.child_pidx + (size_t)min(tile_row0 + r, M - 1) * gather.stride))[lane];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        TG_FS_CHUNK(0, a0, true, early_done = flag_lds[FSR_RING + (step + 2) % FSR_RING])
        // the middle of the step: signal the step after this one, refill the buffer of the step before it
#pragma unroll
        for (int i = 0; i < FSR_RT; i++) asm volatile("" : "+v"(a1[i][0]), "+v"(a1[i][1]), "+v"(b0[i][0]), "+v"(b0[i][1]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (filler && step >= 1 && step + 1 < nsteps) fc_ring_signal(ready0 + 4 * ((step + 1) % FSR_RING));
        if (filler && step + 2 < nsteps) {
            if ((int)__builtin_amdgcn_readfirstlane((int)early_done) < FSR_NW * ((step + 2) / FSR_RING))
                fc_ring_wait(done0 + 4 * ((step + 2) % FSR_RING), (uint32_t)FSR_NW * (uint32_t)((step + 2) / FSR_RING));
            fill(step + 2, (step + 2) % FSR_RING);
        }
        __builtin_amdgcn_sched_barrier(0);
        TG_FS_CHUNK(1, a1, false, early_ready = flag_lds[(step + 1) % FSR_RING])
        fc_ring_signal(done0 + 4 * buf);
#pragma unroll
        for (int i = 0; i < FSR_RT; i++) { a0[i][0] = b0[i][0]; a0[i][1] = b0[i][1]; }
    }
#undef TG_FS_LOAD
#undef TG_FS_MFMA
#undef TG_FS_XMFMA
#undef TG_FS_CHUNK
    // ---- epilogue (per row tile): bias; the statistics of the wave's blocks; logits rows or the children's logits ----
    // gather: the wave's 128 / NW rows park in its share (64 / NW rows × 13 tiles) of each of the two ring buffers that hold nothing of
    // the last K-step, once every wave has read the steps that lived there (done[]; every LDS-DMA into them landed steps ago)
    constexpr int RP = FSR_CT * 16;        // floats per parked row (208)
    constexpr int SHARE = 64 / FSR_NW;     // rows per wave and buffer
    float* park[2] = {nullptr, nullptr};
    if (gather.child_logit) {
        const int bf[2] = {nsteps % FSR_RING, (nsteps + 1) % FSR_RING};
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int uses = bf[b] < nsteps ? (nsteps - bf[b] + FSR_RING - 1) / FSR_RING : 0;
            fc_ring_wait(done0 + 4 * bf[b], (uint32_t)FSR_NW * (uint32_t)uses);
            park[b] = (float*)(wl + bf[b] * FSR_SLOTS) + wave * (SHARE * RP);
        }
    }
    auto parked = [&](int i, int r) { const int rho = i * 16 + r; return park[rho / SHARE] + (rho % SHARE) * RP; };
#pragma unroll
    for (int i = 0; i < FSR_RT; i++) {
        const bool x13 = has13 && i == 0;
        f32x4 v[FSR_CT];
#pragma unroll
        for (int j = 0; j < FC_MAIN_TILES; j++) v[j] = acc[i][j] + *(const f32x4*)&bias[n0 + j * 16 + 4 * q];
        v[FC_MAIN_TILES] = acc[i][FC_MAIN_TILES] + *(const f32x4*)&bias[nx + 4 * q];
        if (stats) {
            float m, sm;
            float* srow = stats + (size_t)(row_ok[i] ? row[i] : 0) * (FC_STAT_STRIDE * 2);
            fc_block_stats<FC_MAIN_TILES>(*reinterpret_cast<const f32x4(*)[FC_MAIN_TILES]>(&v[0]), n0 + 4 * q, min(n_soft, n0 + FC_MAIN_TILES * 16), m, sm);
            if (row_ok[i] && q == 0) *(float2*)&srow[cb * 2] = make_float2(m, sm);
            if (x13) {
                fc_block_stats<1>(*reinterpret_cast<const f32x4(*)[1]>(&v[FC_MAIN_TILES]), nx + 4 * q, min(n_soft, nx + 16), m, sm);
                if (row_ok[i] && q == 0) *(float2*)&srow[(FC_MAIN_BLOCKS + X.l) * 2] = make_float2(m, sm);
                const int dv = n_soft - (nx + 4 * q);  // column n_soft (= P): the value head's pre-activation → pair FC_STAT_BLOCKS
                if (row_ok[i] && dv >= 0 && dv < 4)
                    *(float2*)&srow[FC_STAT_BLOCKS * 2] = make_float2(dv == 0 ? v[FC_MAIN_TILES][0] : dv == 1 ? v[FC_MAIN_TILES][1] : dv == 2 ? v[FC_MAIN_TILES][2] : v[FC_MAIN_TILES][3], 0.0f);
            }
        }
        if (out && row_ok[i]) {
#pragma unroll
            for (int j = 0; j < FSR_CT; j++) {
                const int nn = (j < FC_MAIN_TILES ? n0 + j * 16 : nx) + 4 * q;
                if (nn < n_valid && (j < FC_MAIN_TILES || x13)) {
                    float* o = out + (size_t)row[i] * out_stride + nn;
                    if (nn + 3 < n_valid) *(f32x4*)o = v[j];
                    else for (int t = 0; t < 4; t++) if (nn + t < n_valid) o[t] = v[j][t];
                }
            }
        }
        if (gather.child_logit) {
            {
                float* dst = parked(i, r16) + 4 * q;
#pragma unroll
                for (int j = 0; j < FSR_CT; j++) *(f32x4*)&dst[j * 16] = v[j];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the wave's own parked rows, now read by other lanes of the same wave
            const int tile_row0 = rbx * 128 + rt[i] * 16;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int grow = min(tile_row0 + r, M - 1);
                const uint32_t cnt = tile_row0 + r < M ? min((uint32_t)__builtin_amdgcn_readlane((int)g_cnt[i], r), (uint32_t)gather.stride) : 0u;
                const float* prow = parked(i, r);
                float* crow = gather.child_logit + (size_t)grow * gather.stride;
                const uint16_t* irow = gather.child_pidx + (size_t)grow * gather.stride;
                for (uint32_t c0 = 0; c0 < cnt; c0 += 128) {
                    const uint32_t pair = c0 == 0 ? g_pidx[i][r] : ((const uint32_t*)(irow + c0))[lane];
#pragma unroll
                    for (int hlf = 0; hlf < 2; hlf++) {
                        const uint32_t c = c0 + 2 * lane + hlf;
                        const uint32_t p = hlf ? pair >> 16 : pair & 0xFFFFu;
                        const uint32_t dm = p - (uint32_t)n0, dx = p - (uint32_t)nx;
                        const bool in_main = dm < (uint32_t)(FC_MAIN_TILES * 16), in_x = x13 && dx < 16u;
                        if (c < cnt && (in_main || in_x)) crow[c] = prow[in_main ? dm : FC_MAIN_TILES * 16 + dx];
                    }
                }
            }
        }
    }
}

// value head on the split activations: Linear(F·N² → 1) + tanh; wv in NHWC order (f32)
__global__ __launch_bounds__(256) void k_value_head_s3(const u32x4* __restrict__ act, const float* __restrict__ wv, float bv, int B, int len,
                                                       float* __restrict__ eval) {
    int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    int lane = threadIdx.x & 63;
    const u32x4* a = act + (size_t)b * (len >> 2);
    const f32x4* w = (const f32x4*)wv;
    float s = 0.0f;
    for (int g = lane; g < (len >> 3); g += 64) {
        const u32x4 hi = a[(g >> 2) * 8 + (g & 3)], lo = a[(g >> 2) * 8 + 4 + (g & 3)];
        const f32x4 w0 = w[2 * g], w1 = w[2 * g + 1];
        const f32x4 x0 = join4(u32x2{hi[0], hi[1]}, u32x2{lo[0], lo[1]}), x1 = join4(u32x2{hi[2], hi[3]}, u32x2{lo[2], lo[3]});
#pragma unroll
        for (int t = 0; t < 4; t++) s = fmaf(x0[t], w0[t], s);
#pragma unroll
        for (int t = 0; t < 4; t++) s = fmaf(x1[t], w1[t], s);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) eval[b] = tanhf(s + bv);
}

template <int RTW, int KC0, int KC, bool FROM_STATES, bool OUT_SPLIT, int NW, bool CB = false>
static hipError_t launch_s3_t(hipStream_t st, const void* in, const TowerS3Params& T, float* out, int B, int n, int PW, int NCG) {
    // rows of C·4 + 32 B are bank-conflict free; the 96-channel input image of the 16-position workgroup only fits with + 16 B
    const size_t rows = (size_t)PW * n * n;
    const size_t zrows = ((rows + n + 1 + 15) & ~(size_t)15) + 16 + n + 1;  // image + zero region (k_tower_s3)
    size_t lds = zrows * (T.F + 8) * sizeof(float);
    int pad0 = 2;
    const size_t budget = (size_t)160 * 1024 / (NW == 4 ? 2 : 1);        // two 4-wave workgroups per CU
    if (zrows * (32 * KC0 + 8) * sizeof(float) > budget) pad0 = 1;      // input image: + 16 B pitch and the single zero row
    lds = std::max(lds, (pad0 == 2 ? zrows : rows + 1) * (32 * KC0 + 4 * pad0) * sizeof(float));
    if (CB) lds = std::max(lds, zrows * (32 * KC0 + 4 * pad0) * sizeof(float) + (size_t)PW * 9 * T.F * sizeof(float));  // + PB behind the zero region
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_tower_s3<RTW, KC0, KC, FROM_STATES, OUT_SPLIT, NW, CB>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_tower_s3<RTW, KC0, KC, FROM_STATES, OUT_SPLIT, NW, CB>), dim3((B + PW - 1) / PW), dim3(NW * 64), lds, st, in, T, out, B, n, PW, NCG, pad0);
    return hipGetLastError();
}


template <int RTW, int KC0, int KC, int NB, bool FROM_STATES, bool OUT_SPLIT, int NW, bool CB = false>
static hipError_t launch_s3_halo_t(hipStream_t st, const void* in, const TowerS3Params& T, float* out, int B, int PW, int NCG) {
    const size_t plain = (size_t)(PW * NB * NB + 1) * (32 * KC0 + 4) * sizeof(float) + (CB ? (size_t)PW * 9 * (32 * KC) * sizeof(float) : 0);
    const size_t halo = (size_t)(NB + 2 + PW * T.halo_ps + 1) * (32 * KC + 4) * sizeof(float);  // + the spare cell
    const size_t lds = std::max(plain, halo);
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_tower_s3_halo<RTW, KC0, KC, NB, FROM_STATES, OUT_SPLIT, NW, CB>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_tower_s3_halo<RTW, KC0, KC, NB, FROM_STATES, OUT_SPLIT, NW, CB>), dim3((B + PW - 1) / PW), dim3(NW * 64), lds, st, in, T, out, B, PW, NCG);
    return hipGetLastError();
}

bool tower_s3_halo_geometry(int n, int F, int* pw, int* ps) {
    // positions per workgroup as in launch_s3; strides as tower_halo_geometry (same pitch of F/4 + 1 slots)
    if (n == 5 && F == 64) { *pw = 8; *ps = 36; return true; }    // 80 512 B with the spare cell: two workgroups per CU
    if (n == 5 && F == 128) { *pw = 8; *ps = 37; return true; }   // 160 512 B
    if (n == 6 && F == 128) { *pw = 4; *ps = 51; return true; }   // 112 464 B
    return false;
}
bool tower_s3_supported(int n, int F) { return (n == 5 && (F == 64 || F == 128)) || (n == 6 && F == 128); }

template <bool FROM_STATES, bool OUT_SPLIT>
static hipError_t launch_s3(hipStream_t st, const void* in, const TowerS3Params& T, float* out, int B, int n) {
    // (a tower without a residual block is layer 0 alone: the halo kernel's layer 0 writes halo cells that only a later layer reads — found
    // in round 6 by the batch-independence test on a 0-block network — so it stays on the plain image, whose loop ends behind layer 0)
    static const bool no_halo_env = env_on("TG_NO_HALO_TOWER");
    const bool no_halo = no_halo_env || T.nlayers < 2;
    if (FROM_STATES && T.cb) {  // layer 0 over one chunk of board planes, constant planes as a bias (KC0 = 1): the same tilings
        if (T.slotmap && !no_halo && B >= 256) {
            if (n == 5 && T.F == 64) return launch_s3_halo_t<7, 1, 2, 5, FROM_STATES, OUT_SPLIT, 4, FROM_STATES>(st, in, T, out, B, 8, 2);
            if (n == 5 && T.F == 128) return launch_s3_halo_t<7, 1, 4, 5, FROM_STATES, OUT_SPLIT, 8, FROM_STATES>(st, in, T, out, B, 8, 4);
            if (n == 6 && T.F == 128) return launch_s3_halo_t<5, 1, 4, 6, FROM_STATES, OUT_SPLIT, 8, FROM_STATES>(st, in, T, out, B, 4, 4);
        }
        if (n == 5 && T.F == 64) return launch_s3_t<7, 1, 2, FROM_STATES, OUT_SPLIT, 4, FROM_STATES>(st, in, T, out, B, n, 8, 2);
        if (n == 5 && T.F == 128) return launch_s3_t<7, 1, 4, FROM_STATES, OUT_SPLIT, 8, FROM_STATES>(st, in, T, out, B, n, 8, 4);
        if (n == 6 && T.F == 128) return launch_s3_t<5, 1, 4, FROM_STATES, OUT_SPLIT, 8, FROM_STATES>(st, in, T, out, B, n, 4, 4);
        return hipErrorInvalidValue;
    }
    if (T.slotmap && !no_halo && B >= 256) {  // the halo image (same workgroup shapes as below; identical bits)
        if (n == 5 && T.F == 64) return launch_s3_halo_t<7, 3, 2, 5, FROM_STATES, OUT_SPLIT, 4>(st, in, T, out, B, 8, 2);
        if (n == 5 && T.F == 128) return launch_s3_halo_t<7, 3, 4, 5, FROM_STATES, OUT_SPLIT, 8>(st, in, T, out, B, 8, 4);
        if (n == 6 && T.F == 128) return launch_s3_halo_t<5, 3, 4, 6, FROM_STATES, OUT_SPLIT, 8>(st, in, T, out, B, 4, 4);
    }
    // 5×5, F = 64: 8 positions = 13 row tiles = 2 row groups (7,6) × 2 channel groups, 4 waves, two workgroups per CU
    if (n == 5 && T.F == 64) return launch_s3_t<7, 3, 2, FROM_STATES, OUT_SPLIT, 4>(st, in, T, out, B, n, 8, 2);
    // 5×5, F = 128: 8 positions = 13 row tiles = 2 row groups (7,6) × 4 channel groups
    if (n == 5 && T.F == 128) return launch_s3_t<7, 3, 4, FROM_STATES, OUT_SPLIT, 8>(st, in, T, out, B, n, 8, 4);
    // 6×6, F = 128: 4 positions = 9 row tiles = 2 row groups (5,4) × 4 channel groups
    if (n == 6 && T.F == 128) return launch_s3_t<5, 3, 4, FROM_STATES, OUT_SPLIT, 8>(st, in, T, out, B, n, 4, 4);
    return hipErrorInvalidValue;
}
hipError_t launch_tower_s3(hipStream_t st, const float* planes, const TowerS3Params& T, float* out, int B, int n, bool out_split) {
    return out_split ? launch_s3<false, true>(st, planes, T, out, B, n) : launch_s3<false, false>(st, planes, T, out, B, n);
}
hipError_t launch_tower_s3_states(hipStream_t st, const uint8_t* states, const TowerS3Params& T, float* out, int B, int n, bool out_split) {
    return out_split ? launch_s3<true, true>(st, states, T, out, B, n) : launch_s3<true, false>(st, states, T, out, B, n);
}
bool fc_s3_supported(int K, int NP) { return K % 64 == 0 && NP % FC_S3_COLS == 0; }
bool fc_s3_ring_supported(int M, int K, int n_valid) { return K % 64 == 0 && n_valid <= FC_TILES * 16 && M > 512; }
// Wp: the [chunk][column block][q][hi|lo][column] layout of k_fc_s3b (≤ 512 rows); Wr (optional): the ring layout of
// k_fc_s3_ring (full batches).  stats: the block statistics of softmax.cuh's geometry (the exact-f32 FC's), from the ring's epilogue
// or by k_fc_stats behind k_fc_s3b — the same bits.  gather: as launch_gemm's (needs Wr and > 512 rows).
hipError_t launch_fc_s3(hipStream_t st, const float* act_split, const void* Wp, const void* Wr, const float* bias, float* out, int M, int K, int NP,
                        int out_stride, int n_valid, float* stats, int n_soft, const FcGatherArgs* gather) {
    if (stats && (n_valid > FC_TILES * 16 || out_stride < FC_TILES * 16)) return hipErrorInvalidValue;
    static const bool no_ring = env_on("TG_S3_NO_FC_RING");  // A/B: k_fc_s3b at every batch (same bits)
    if (Wr && !no_ring && fc_s3_ring_supported(M, K, n_valid)) {
        static LdsAttr lds_attr;
        if (hipError_t e = lds_attr.ensure((const void*)k_fc_s3_ring, FSR_LDS); e != hipSuccess) return e;
        FcGather g{nullptr, nullptr, nullptr, 0};
        if (gather) g = FcGather{gather->child_pidx, gather->leaf_rec, gather->child_logit, gather->stride};
        hipLaunchKernelGGL(k_fc_s3_ring, dim3((M + 127) / 128, FC_MAIN_BLOCKS), dim3(FSR_NW * 64), FSR_LDS, st, (const u32x4*)act_split, (const u32x4*)Wr, bias,
                           gather ? nullptr : out, M, K, out_stride, n_valid, stats, n_soft, g);
        return hipGetLastError();
    }
    if (gather || NP % FC_S3_COLS) return hipErrorInvalidValue;
    dim3 grid((M + 127) / 128, NP / FC_S3_COLS);
    hipLaunchKernelGGL((k_fc_s3b<FC_S3_COLS / 16, 4>), grid, dim3(256), 0, st, (const u32x4*)act_split, (const u32x4*)Wp, bias, out, M, K, NP, out_stride, n_valid,
                       nullptr, n_soft);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return stats ? launch_fc_stats(st, out, out_stride, M, n_soft, stats) : hipSuccess;
}
hipError_t launch_value_head_s3(hipStream_t st, const float* act_split, const float* wv, float bv, int B, int len, float* eval) {
    hipLaunchKernelGGL(k_value_head_s3, dim3((B + 3) / 4), dim3(256), 0, st, (const u32x4*)act_split, wv, bv, B, len, eval);
    return hipGetLastError();
}

}  // namespace tg
