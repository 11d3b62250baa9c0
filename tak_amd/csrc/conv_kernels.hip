// conv_kernels.hip — one 3×3 convolution layer per launch on CDNA4 matrix cores, exact f32.
//
// With tower_kernels.hip (the fused towers) and fc_kernels.hip (policy FC, softmax, value head) this replaces the libtorch ops behind
// reference alpha-tak/src/model/{net5,net6,res_block}.rs (conv2d 3×3 pad 1 + batch_norm(eval) + relu + residual add, linear, softmax,
// tanh).
//
// Layout: activations are NHWC — row m = (position b, square sq), F contiguous channels — so a 3×3 convolution is an
// implicit GEMM  out[m][o] = Σ_{tap,c} X[nbr(m,tap)][c] · W[tap,c][o]  with M = B·N² rows, K = 9·C.  Halos never cross
// positions, so a workgroup keeps whole positions in LDS and a tap is an LDS offset: im2col lives in address arithmetic.
// Arithmetic: v_mfma_f32_16x16x4_f32 in the fused towers and the policy FC, v_mfma_f32_32x32x2_f32 in the generic per-layer
// kernels — f32 in, f32 accumulate, bit-exact fmaf chains (the parity path; 157.3 TFLOP/s peak).  BatchNorm (eval) is
// folded into weights / bias at load time; bias, residual and ReLU are fused into the accumulator epilogue.
//
// Kernels, in the order of the file:
//   k_conv3x3, k_conv_pos   one 3×3 layer (shapes the fused towers do not cover; the conv policy head of Net6)
//   k_conv_halo             one 3×3 layer on the halo image of k_tower_halo: the training step's convolutions at full batches
//   k_conv_split            one 3×3 layer for small batches: workgroup = (position, 16-channel tile)
// Every variant of a layer type performs the same products in the same order: a position's outputs are the same bits
// whatever batch (and therefore kernel) evaluates it (tests/test_gpu_net.py, tests/test_gpu_variants.py).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "conv_mainloop.cuh"
#include "pos_tiling.h"
#include "tower_stage.cuh"
#include "tower_stamps.cuh"
#include "kernels.h"

namespace tg {

// Workgroup = 4 waves as 2 (rows) × 2 (cols); each wave owns RT×CT tiles of 32×32.
template <int RT, int CT>
__global__ __launch_bounds__(256) void k_conv3x3(const float* __restrict__ in, const float* __restrict__ Wp,
                                                 const float* __restrict__ bias, const float* __restrict__ res,
                                                 float* __restrict__ out, int M, int n, int Cpad, int CoutP,
                                                 int out_stride, int cout_valid, int relu) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int TM = 64 * RT;
    const int tid = threadIdx.x;
    const int nsq = n * n;
    const int LS = Cpad + LDS_PAD;
    const int m0 = blockIdx.x * TM;
    const int mlast = min(m0 + TM, M) - 1;
    const int pos0 = m0 / nsq;
    const int npos = mlast / nsq - pos0 + 1;
    const int rows = npos * nsq;

    // ---- stage the touched positions (contiguous in global) into padded LDS rows ----
    {
        const int vpr = Cpad >> 2;  // float4 per row
        const float4* src = (const float4*)(in + (size_t)pos0 * nsq * Cpad);
        const int total = rows * vpr;
        for (int idx = tid; idx < total; idx += 256) {
            int r = idx / vpr, v = idx - r * vpr;
            float4 x = src[idx];
            *(float4*)&lds[r * LS + v * 4] = x;
        }
        for (int idx = tid; idx < LS; idx += 256) lds[rows * LS + idx] = 0.0f;  // the zero row
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int wr = wave & 1, wc = wave >> 1;
    const int i = lane & 31, h = lane >> 5;
    const int zero_off = rows * LS + 4 * h;

    int base_off[RT], py[RT], px[RT];
    bool valid[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        int m = m0 + (wr * RT + rt) * 32 + i;
        valid[rt] = m < M;
        int mm = valid[rt] ? m : m0;
        int p = mm / nsq;
        int sq = mm - p * nsq;
        py[rt] = sq / n;
        px[rt] = sq - py[rt] * n;
        base_off[rt] = ((p - pos0) * nsq + sq) * LS + 4 * h;
    }

    f32x16 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[rt][ct][r] = 0.0f;

    const int col0 = blockIdx.y * (64 * CT) + wc * (32 * CT);
    const int chunks = Cpad >> 3;
    // B fragment base: Wp[k/16][col][16]; 8-wide sub-chunk c8 lives at [c8>>1][col][8*(c8&1) ..]; this lane:
    // column col0 + ct*32 + i, k sub-offset 4h
    const float* wlane = Wp + ((size_t)(col0 + i) * 16 + 4 * h);
    const size_t wchunk_stride = (size_t)CoutP * 16;

    for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        int aoff[RT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            int yy = py[rt] + dy, xx = px[rt] + dx;
            bool ok = valid[rt] && yy >= 0 && yy < n && xx >= 0 && xx < n;
            aoff[rt] = ok ? base_off[rt] + (dy * n + dx) * LS : zero_off;
        }
        const float* wtap = wlane + (size_t)tap * (chunks >> 1) * wchunk_stride;
        for (int c8 = 0; c8 < chunks; c8++) {
            f32x4 a[RT], b[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
                b[ct] = *(const f32x4*)(wtap + (size_t)(c8 >> 1) * wchunk_stride + (size_t)ct * 32 * 16 + 8 * (c8 & 1));
#pragma unroll
            for (int rt = 0; rt < RT; rt++) a[rt] = *(const f32x4*)&lds[aoff[rt] + c8 * 8];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int ct = 0; ct < CT; ct++)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[rt][t], b[ct][t], acc[rt][ct], 0, 0, 0);
        }
    }

    // ---- epilogue: bias (+ residual) (+ ReLU); C/D map: col = lane&31, row = (r&3) + 8(r>>2) + 4(lane>>5) ----
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const int col = col0 + ct * 32 + i;
            const float bv = bias[col];
#pragma unroll
            for (int r = 0; r < 16; r++) {
                int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                int m = m0 + (wr * RT + rt) * 32 + row;
                if (m < M && col < cout_valid) {
                    float v = acc[rt][ct][r] + bv;
                    size_t o = (size_t)m * out_stride + col;
                    if (res) v += res[o];
                    if (relu) v = fmaxf(v, 0.0f);
                    out[o] = v;
                }
            }
        }
    }
}



// ------------------------------------------------------------------------------------------------
// Whole-positions variant: a workgroup owns PW complete positions (PW·N² rows, e.g. 16 positions = 400
// rows = 25 row tiles on 5×5; 4 positions = 144 rows = 9 tiles on 6×6) and CTW 16-wide channel tiles, so
// the grid is an exact multiple of the 256 CUs (no tail wave) and no position is staged twice.
// v_mfma_f32_16x16x4_f32 with the WEIGHTS as the A operand and the activations as B: the accumulator then
// holds, per lane, 4 consecutive output channels of one row → 16-byte epilogue loads/stores.
// Waves: wave = (row group rg, channel tile ct); each wave owns RTW row tiles × 1 channel tile.
// ------------------------------------------------------------------------------------------------
template <int RTW, int NWAVES>
__global__ __launch_bounds__(NWAVES * 64) void k_conv_pos(const float* __restrict__ in, const float* __restrict__ Wp,
                                                          const float* __restrict__ bias, const float* __restrict__ res,
                                                          float* __restrict__ out, int B, int n, int Cpad, int CoutP,
                                                          int out_stride, int cout_valid, int relu, int PW, int CTW) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;  // every access below is a whole 16-byte slot → ds_read_b128 / ds_write_b128
    const int tid = threadIdx.x;
    const int nsq = n * n;
    const int LS4 = (Cpad + LDS_PAD16) >> 2;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int rows = npos * nsq;
    {
        const int vpr = Cpad >> 2;
        const f32x4* src = (const f32x4*)(in + (size_t)pos0 * nsq * Cpad);
        const int total = rows * vpr;
        // all of a thread's loads are issued before the first LDS write (8 in flight per lane)
        constexpr int UNR = 8;
        for (int base = 0; base < total; base += NWAVES * 64 * UNR) {
            f32x4 tmp[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                int idx = base + u * NWAVES * 64 + tid;
                tmp[u] = idx < total ? src[idx] : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                int idx = base + u * NWAVES * 64 + tid;
                if (idx < total) {
                    int r = idx / vpr, v = idx - r * vpr;
                    lds4[r * LS4 + v] = tmp[u];
                }
            }
        }
        for (int idx = tid; idx < LS4; idx += NWAVES * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __syncthreads();

    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW, rg = wave / CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int zero4 = rows * LS4 + q;

    int base4[RTW], pyx[RTW];
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        int rho = (rg * RTW + j) * 16 + r16;
        bool valid = rho < rows;
        int rr = valid ? rho : 0;
        int p = rr / nsq;
        int sq = rr - p * nsq;
        int y = sq / n, x = sq - y * n;
        pyx[j] = valid ? (y | (x << 8)) : 0x7f7f;  // invalid rows: every tap falls off the board
        base4[j] = rr * LS4 + q;
    }

    f32x4 acc[RTW];
#pragma unroll
    for (int j = 0; j < RTW; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int ch0 = (blockIdx.y * CTW + ct) * 16;
    const int chunks = Cpad >> 4;
    const int total_chunks = 9 * chunks;
    // weights: Wp[k/16][ch][16] = 4 slots of 16 B per (chunk, channel); this lane reads slot q of channel ch0 + r16
    const f32x4* wp = (const f32x4*)Wp + ((size_t)(ch0 + r16) * 4 + q);
    const size_t wstride4 = (size_t)CoutP * 4;

    f32x4 w_cur = wp[0];
    int kk = 0;
    for (int tap = 0; tap < 9; tap++) {
        const int dy = tap / 3 - 1, dx = tap % 3 - 1;
        int aoff[RTW];
#pragma unroll
        for (int j = 0; j < RTW; j++) {
            int yy = (pyx[j] & 0xff) + dy, xx = (pyx[j] >> 8) + dx;
            bool ok = yy >= 0 && yy < n && xx >= 0 && xx < n;
            aoff[j] = ok ? base4[j] + (dy * n + dx) * LS4 : zero4;
        }
        f32x4 a_cur[RTW];
#pragma unroll
        for (int j = 0; j < RTW; j++) a_cur[j] = lds4[aoff[j]];
        // every tap's products in a chain of their own, added to acc when the tap is complete (conv_mainloop_halo's SPLIT: the same
        // chains in the same order → the same bits as k_conv_halo)
        f32x4 part[RTW];
#pragma unroll
        for (int j = 0; j < RTW; j++) part[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        for (int kc = 0; kc < chunks; kc++) {
            // software pipeline: the next chunk's weights (L2) and activations (LDS) are in flight while
            // this chunk's 4·RTW MFMAs issue
            const int kkn = kk + 1 < total_chunks ? kk + 1 : kk;
            const f32x4 w_nxt = wp[(size_t)kkn * wstride4];
            const int kn = kc + 1 < chunks ? kc + 1 : kc;
            f32x4 a_nxt[RTW];
#pragma unroll
            for (int j = 0; j < RTW; j++) a_nxt[j] = lds4[aoff[j] + kn * 4];
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int j = 0; j < RTW; j++) part[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(w_cur[t], a_cur[j][t], part[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < RTW; j++) a_cur[j] = a_nxt[j];
            w_cur = w_nxt;
            kk++;
        }
#pragma unroll
        for (int j = 0; j < RTW; j++) acc[j] += part[j];
    }

    // epilogue: lane holds out[row = tile*16 + (lane&15)][ch0 + 4q .. 4q+3]
    const int ch = ch0 + 4 * q;
    const f32x4 bv = *(const f32x4*)&bias[ch];
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        int rho = (rg * RTW + j) * 16 + r16;
        if (rho < rows && ch < cout_valid) {
            size_t o = ((size_t)pos0 * nsq + rho) * out_stride + ch;
            f32x4 v = acc[j] + bv;
            if (res) v += *(const f32x4*)&res[o];
            if (relu) v = relu4(v);
            if (ch + 3 < cout_valid) *(f32x4*)&out[o] = v;
            else for (int t = 0; t < 4; t++) if (ch + t < cout_valid) out[o + t] = v[t];
        }
    }
}


// ------------------------------------------------------------------------------------------------
// ONE 3×3 layer on the halo image (the main loop of k_tower_halo for a layer that stands alone): the convolutions of the
// training step — forward in training mode and the data gradient, F → F, activations in HBM between them because
// BatchNorm's batch statistics sit between two layers — and the conv policy head of Net6 (F → 251 in 256).  The input rows
// of the workgroup's PW positions are staged from global straight into halo cells; taps are ds_read immediates, the
// weights stream through a buffer descriptor two chunks ahead, slots come from the same slot table as the tower's.
// Epilogue: + bias, + res (optional), ReLU (optional).  COT = CoutP / 16; blockIdx.y picks a group of CTW channel tiles.
// ------------------------------------------------------------------------------------------------
// PSC: the position stride of the halo image (tower_halo_geometry) as a constant — the zero-cell fill divides by it 19 000 times
template <int RTW, int NWAVES, int CH, int NB, int COT, int PSC>
__global__ __launch_bounds__(NWAVES * 64) void k_conv_halo(const float* __restrict__ in, const float* __restrict__ Wp,
                                                           const float* __restrict__ bias, const float* __restrict__ res,
                                                           float* __restrict__ out, const uint32_t* __restrict__ slotmap, int B, int PW,
                                                           int PS, int CTW, int out_stride, int cout_valid, int relu,
                                                           double* __restrict__ stats_part, const ConvBnBwdIn bnb) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;
    constexpr int n = NB, nsq = NB * NB, RS = NB + 1, LEAD = NB + 2, F4 = 4 * CH, P4 = 4 * CH + 1;
    PS = PSC;
    const int tid = threadIdx.x;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int rows = npos * nsq;
    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW, rg = wave / CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = (blockIdx.y * CTW + ct) * 16;
    const uint32_t wlane = (uint32_t)(((ch0 + r16) * 4 + q) * 16);
    f32x4 w0, w1;
    TG_STAMP(0, 0);
#ifdef TG_TOWER_STAMPS  // wall-clock (100 MHz) start and end of every workgroup: dispatch skew and tail of a launch
    if (g_tower_stamps && tid == 0) g_tower_stamps[128 + 2 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
    conv_halo_first_weights<CH, COT>(Wp, wlane, w0, w1);  // in flight while the image is staged
    // zero cells (behind every board row, the zero row behind every position, lead and tail) …
    const int cells = LEAD + PW * PS + 1;
    for (int idx = tid; idx < cells * P4; idx += NWAVES * 64) {
        const int c = idx / P4 - LEAD;
        const int o = c < 0 || c >= PW * PS ? n * RS : c % PS;
        if (o >= n * RS || o % RS == n) lds4[idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    // … and the squares' rows from global (row-major [row][16·CH]), 8 loads in flight per lane
    auto halo_cell = [&](int idx) {
        const int r = idx / F4, v = idx - r * F4;
        const int p = r / nsq, sq = r - p * nsq, y = sq / n, x = sq - y * n;
        return (LEAD + p * PS + y * RS + x) * P4 + v;
    };
    const f32x4* src = (const f32x4*)(in + (size_t)pos0 * nsq * (16 * CH));
    const int total = rows * F4;
    {
        constexpr int UNR = 8;
        for (int base = 0; base < total; base += NWAVES * 64 * UNR) {
            f32x4 tmp[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int idx = base + u * NWAVES * 64 + tid;
                tmp[u] = src[idx < total ? idx : total - 1];
            }
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int idx = base + u * NWAVES * 64 + tid;
                if (idx < total) lds4[halo_cell(idx)] = tmp[u];
            }
        }
    }
    __syncthreads();
    TG_STAMP(0, 1);

    const int NRG = NWAVES / CTW;
    const int ntiles = (PW * nsq + 15) >> 4;
    const int tbase = ntiles / NRG, trem = ntiles - tbase * NRG;
    const int my_tiles = tbase + (rg < trem ? 1 : 0);
    const int tile0 = rg * tbase + min(rg, trem);
    const bool short_group = my_tiles < RTW;
    f32x4 acc[RTW];
    int addr4[RTW];
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const uint32_t e = j < my_tiles ? slotmap[(tile0 + j) * 16 + r16] : 0xFFFF0000u;
        const bool idle = (e >> 16) == 0xFFFFu;  // a slot without a square reads around a zero cell and stores nothing
        addr4[j] = ((idle ? LEAD + n * RS : (int)(e & 0xFFFFu)) - LEAD) * P4 + q;
    }
    const int turn = (wave >> 2) & 1;
    TG_STAMP(0, 2);
    if (RTW > 1 && short_group) {
        f32x4 (&acs)[RTW - 1] = *reinterpret_cast<f32x4 (*)[RTW - 1]>(&acc[0]);
        conv_mainloop_halo<RTW - 1, CH, NB, RTW, COT, true>(lds4, Wp, Wp, wlane, addr4, acs, turn, w0, w1);
    } else {
        conv_mainloop_halo<RTW, CH, NB, RTW, COT, true>(lds4, Wp, Wp, wlane, addr4, acc, turn, w0, w1);
    }
    TG_STAMP(0, 3);
    const int ch = ch0 + 4 * q;
    const f32x4 bv = *(const f32x4*)&bias[ch];
    // (the tiles' rows are looked up again here rather than kept in 13 registers across the main loop, whose two accumulator sets
    // leave none to spare)
    int rowid[RTW];
#pragma unroll
    for (int j = 0; j < RTW; j++) rowid[j] = j < my_tiles ? (int)(slotmap[(tile0 + j) * 16 + r16] >> 16) : 0xFFFF;
    // stats_part: Σ and Σ² of this lane's outputs, per channel — in double from the first add on: var = E[z²] − E[z]² loses
    // (mean/σ)² of the sums' relative accuracy, and f32 partials over up to 208 rows left 1e-4 of the variance at |mean| = 10σ.
    // With bnb.y set (round 4; the data-gradient convolution of the training step): the output IS dy of the layer below, and the
    // same two slots collect that layer's BatchNorm-backward sums Σg and Σg·x̂ (g = dy·[y > 0], x̂ = (z − mean)·invstd) while dy is
    // in registers — k_col_reduce<RED_BNBWD>'s pass over dy, y and z (27 µs per layer) is gone
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 bn_mu = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, bn_is = bn_mu;
    if (bnb.y && ch0 + 4 * q < cout_valid) { bn_mu = *(const f32x4*)&bnb.mean[ch0 + 4 * q]; bn_is = *(const f32x4*)&bnb.invstd[ch0 + 4 * q]; }
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        if (rowid[j] < rows && ch < cout_valid) {
            const size_t o = ((size_t)pos0 * nsq + rowid[j]) * out_stride + ch;
            f32x4 v = acc[j] + bv;
            if (res) v += *(const f32x4*)&res[o];
            if (relu) v = relu4(v);
            if (ch + 3 < cout_valid) *(f32x4*)&out[o] = v;
            else for (int t = 0; t < 4; t++) if (ch + t < cout_valid) out[o + t] = v[t];
            if (stats_part && !bnb.y) {
#pragma unroll
                for (int t = 0; t < 4; t++) { const double d = (double)v[t]; s1[t] += d; s2[t] = fma(d, d, s2[t]); }
            } else if (stats_part) {
                const f32x4 yy = *(const f32x4*)&bnb.y[o], zz = *(const f32x4*)&bnb.z[o];
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const float g = yy[t] > 0.0f ? v[t] : 0.0f;
                    s1[t] += (double)g;
                    s2[t] += (double)(g * ((zz[t] - bn_mu[t]) * bn_is[t]));
                }
            }
        }
    }
    if (stats_part) {
        // BatchNorm's batch statistics from the accumulators (training forward): the column sums of this wave's rows — 16
        // lanes of a q-group hold 16 rows of the same 4 channels — leave the kernel as doubles, one partial row per (workgroup,
        // row group): part[((blockIdx.x·NRG + rg)·2 + {Σ, Σ²})·CoutP + channel], k_col_reduce's layout, summed in fixed order later
#pragma unroll
        for (int d = 1; d < 16; d <<= 1)
#pragma unroll
            for (int t = 0; t < 4; t++) { s1[t] += __shfl_xor(s1[t], d); s2[t] += __shfl_xor(s2[t], d); }
        if (r16 == 0) {
            const int CoutP = 16 * COT;
            double* dst = stats_part + ((size_t)(blockIdx.x * NRG + rg) * 2) * CoutP + ch;
#pragma unroll
            for (int t = 0; t < 4; t++) { dst[t] = s1[t]; dst[CoutP + t] = s2[t]; }
        }
    }
    TG_STAMP(0, 4);
#ifdef TG_TOWER_STAMPS
    if (g_tower_stamps && tid == NWAVES * 64 - 64) g_tower_stamps[128 + 2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
#endif
}

// ONE 3×3 layer for SMALL batches (round 6; the conv policy head of Net6 at the reference's 32 leaves: k_conv_pos gave a position to
// one workgroup — 32 busy CUs — with 3 row tiles per wave and the weights one chunk ahead): workgroup = (position, 16-channel tile),
// wave = row tile, ONE chain per wave with the weights a tap ahead (conv_mainloop_tile).  k_conv_pos's sums — a chain per tap, added in
// tap order — so the same bits.  No residual, no statistics: the head and plain layers.
template <int NRT, int CH>
__global__ __launch_bounds__(NRT * 64) void k_conv_split(const float* __restrict__ in, const float* __restrict__ Wp, const float* __restrict__ bias,
                                                         float* __restrict__ out, int n, int CoutP, int out_stride, int cout_valid, int relu) {
    constexpr int F = 16 * CH, F4 = F / 4, LS4 = (F + LDS_PAD16) >> 2;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;
    const int tid = threadIdx.x, nsq = n * n, rows = nsq;
    const int p = blockIdx.x, ch0 = blockIdx.y * 16;
    const int rt = tid >> 6, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
    const int rho = rt * 16 + r16;
    const f32x4* wp = (const f32x4*)Wp + ((size_t)(ch0 + r16) * 4 + q);
    const size_t wstride4 = (size_t)CoutP * 4;
    f32x4 wf[CH];
    conv_tile_first_weights<CH>(wp, wstride4, wf);  // in flight while the image is staged
    {
        const f32x4* src = (const f32x4*)(in + (size_t)p * nsq * F);
        const int total = nsq * F4;
        constexpr int UNR = 8;
        for (int base = 0; base < total; base += NRT * 64 * UNR) {
            f32x4 tmp[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int idx = base + u * NRT * 64 + tid;
                tmp[u] = src[idx < total ? idx : total - 1];
            }
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int idx = base + u * NRT * 64 + tid;
                if (idx < total) lds4[(idx / F4) * LS4 + idx % F4] = tmp[u];
            }
        }
        for (int idx = tid; idx < LS4; idx += NRT * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __syncthreads();
    int vmask[1];
    conv_tap_masks<1>(rows, n, nsq, rho, vmask);
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    conv_mainloop_tile<CH, 4, true>(lds4, wp, wstride4, LS4, rows, n, rho, q, vmask[0], acc, wf);
    const int ch = ch0 + 4 * q;
    if (rho < rows && ch < cout_valid) {
        f32x4 v = acc + *(const f32x4*)&bias[ch];
        if (relu) v = relu4(v);
        const size_t o = ((size_t)p * nsq + rho) * out_stride + ch;
        if (ch + 3 < cout_valid) *(f32x4*)&out[o] = v;
        else for (int t = 0; t < 4; t++) if (ch + t < cout_valid) out[o + t] = v[t];
    }
}

// ---- launchers --------------------------------------------------------------------------------
size_t conv_lds_bytes(int rt, int n, int Cpad) {
    int TM = 64 * rt, nsq = n * n;
    int max_pos = (TM - 1) / nsq + 2;
    return (size_t)(max_pos * nsq + 1) * (Cpad + LDS_PAD) * sizeof(float);
}

template <int RT, int CT>
static hipError_t launch_conv_t(hipStream_t st, const float* in, const float* Wp, const float* bias, const float* res,
                                float* out, int M, int n, int Cpad, int CoutP, int out_stride, int cout_valid, bool relu) {
    size_t lds = conv_lds_bytes(RT, n, Cpad);
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_conv3x3<RT, CT>, lds); e != hipSuccess) return e;
    dim3 grid((M + 64 * RT - 1) / (64 * RT), CoutP / (64 * CT));
    hipLaunchKernelGGL((k_conv3x3<RT, CT>), grid, dim3(256), lds, st, in, Wp, bias, res, out, M, n, Cpad, CoutP, out_stride,
                       cout_valid, relu ? 1 : 0);
    return hipGetLastError();
}

template <int RTW, int NWAVES>
static hipError_t launch_conv_pos_t(hipStream_t st, const float* in, const float* Wp, const float* bias, const float* res,
                                    float* out, int B, int n, int Cpad, int CoutP, int out_stride, int cout_valid, bool relu,
                                    int PW, int CTW) {
    size_t lds = (size_t)(PW * n * n + 1) * (Cpad + LDS_PAD16) * sizeof(float);
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_conv_pos<RTW, NWAVES>, lds); e != hipSuccess) return e;
    dim3 grid((B + PW - 1) / PW, CoutP / (CTW * 16));
    hipLaunchKernelGGL((k_conv_pos<RTW, NWAVES>), grid, dim3(NWAVES * 64), lds, st, in, Wp, bias, res, out, B, n, Cpad, CoutP,
                       out_stride, cout_valid, relu ? 1 : 0, PW, CTW);
    return hipGetLastError();
}

// slot table of the halo image for (n, F) on the current device, built on first use (launch_conv3x3's halo path; the fused
// tower carries its own copy in TowerParams)
static const uint32_t* conv_halo_slotmap(int n, int F, int pw, int ps) {
    struct Entry { int dev, n, F, pw, ps; uint32_t* d; };
    static std::vector<Entry> cache;
    static std::mutex guard;  // trainers of several engines may run on several host threads (data-parallel tests)
    std::lock_guard<std::mutex> lock(guard);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    for (const Entry& e : cache) if (e.dev == dev && e.n == n && e.F == F && e.pw == pw && e.ps == ps) return e.d;
    std::vector<uint32_t> map((size_t)((pw * n * n + 15) / 16) * 16);
    tower_halo_slotmap(n, pw, ps, map.data());
    uint32_t* d = nullptr;
    if (hipMalloc((void**)&d, map.size() * 4) != hipSuccess) return nullptr;
    if (hipMemcpy(d, map.data(), map.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    cache.push_back({dev, n, F, pw, ps, d});
    return d;
}

template <int RTW, int NWAVES, int CH, int NB, int COT, int PSC>
static hipError_t launch_conv_halo_t(hipStream_t st, const float* in, const float* Wp, const float* bias, const float* res, float* out,
                                     const uint32_t* slotmap, int B, int PW, int PS, int CTW, int out_stride, int cout_valid, bool relu,
                                     double* stats_part, int* stats_blocks, const ConvBnBwdIn* bnb) {
    if (PS != PSC) return hipErrorInvalidValue;
    const size_t lds = (size_t)(NB + 2 + PW * PS + 1) * (16 * CH + 4) * sizeof(float);
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_conv_halo<RTW, NWAVES, CH, NB, COT, PSC>, lds); e != hipSuccess) return e;
    dim3 grid((B + PW - 1) / PW, COT / CTW);
    if (grid.y != 1) stats_part = nullptr;  // (statistics only for layers whose channels one workgroup column covers)
    ConvBnBwdIn bn{nullptr, nullptr, nullptr, nullptr};
    if (bnb && stats_part && out_stride == 16 * COT) bn = *bnb;  // (y and z share the output's row layout)
    else if (bnb) stats_part = nullptr;
    hipLaunchKernelGGL((k_conv_halo<RTW, NWAVES, CH, NB, COT, PSC>), grid, dim3(NWAVES * 64), lds, st, in, Wp, bias, res, out, slotmap, B, PW, PS,
                       CTW, out_stride, cout_valid, relu ? 1 : 0, stats_part, bn);
    if (stats_blocks) *stats_blocks = stats_part ? (int)grid.x * (NWAVES / CTW) : 0;
    return hipGetLastError();
}

hipError_t launch_conv3x3(hipStream_t st, const float* in, const float* Wp, const float* bias, const float* res, float* out,
                          int M, int n, int Cpad, int CoutP, int out_stride, int cout_valid, bool relu, double* stats_part,
                          int* stats_blocks, const ConvBnBwdIn* bnb) {
    const int B = M / (n * n);
    if (stats_blocks) *stats_blocks = 0;
    {   // F → F (and F → 2F) layers of the BASELINE topologies at full batches: the halo image (k_conv_halo), same bits as k_conv_pos
        static const bool off = env_on("TG_NO_HALO_CONV");
        int pw, ps;
        if (!off && B >= 1024 && tower_halo_geometry(n, Cpad, &pw, &ps)) {
            const uint32_t* map = conv_halo_slotmap(n, Cpad, pw, ps);
            if (map) {
                if (n == 5 && Cpad == 64 && CoutP == 64) return launch_conv_halo_t<13, 8, 4, 5, 4, 36>(st, in, Wp, bias, res, out, map, B, pw, ps, 4, out_stride, cout_valid, relu, stats_part, stats_blocks, bnb);
                if (n == 5 && Cpad == 128 && CoutP == 128) return launch_conv_halo_t<13, 8, 8, 5, 8, 37>(st, in, Wp, bias, res, out, map, B, pw, ps, 8, out_stride, cout_valid, relu, stats_part, stats_blocks, bnb);
                if (n == 6 && Cpad == 128 && CoutP == 128) return launch_conv_halo_t<9, 8, 8, 6, 8, 51>(st, in, Wp, bias, res, out, map, B, pw, ps, 8, out_stride, cout_valid, relu, stats_part, stats_blocks, bnb);
                if (n == 6 && Cpad == 128 && CoutP == 256) return launch_conv_halo_t<9, 8, 8, 6, 16, 51>(st, in, Wp, bias, res, out, map, B, pw, ps, 8, out_stride, cout_valid, relu, stats_part, stats_blocks, bnb);
            }
        }
    }
    {   // small batches of a layer without residual and statistics (the conv policy head): (position, channel tile) workgroups
        static const bool off = env_on("TG_NO_SPLIT_TOWER");
        if (!off && !res && !stats_part && !bnb && B >= 1 && B <= TOWER_SPLIT_MAX_BATCH && Cpad == 128 && CoutP % 16 == 0 && (n == 5 || n == 6)) {
            const size_t lds = (size_t)(n * n + 1) * (128 + LDS_PAD16) * sizeof(float);
            const dim3 grid(B, CoutP / 16);
            if (n == 6) hipLaunchKernelGGL((k_conv_split<3, 8>), grid, dim3(192), lds, st, in, Wp, bias, out, n, CoutP, out_stride, cout_valid, relu ? 1 : 0);
            else hipLaunchKernelGGL((k_conv_split<2, 8>), grid, dim3(128), lds, st, in, Wp, bias, out, n, CoutP, out_stride, cout_valid, relu ? 1 : 0);
            return hipGetLastError();
        }
    }
    // whole-positions kernel where the shape divides evenly (the BASELINE configs; on 6×6 also layers of 256 output channels, two
    // workgroup columns); generic tiles otherwise
    const int pos_F = (n == 5 && CoutP == 64 && Cpad <= 80) ? 64 : ((n == 5 || n == 6) && CoutP % 128 == 0 && Cpad <= 128) ? 128 : 0;
    if (pos_F)
        return launch_pos_tiled(n, pos_F, B, [&](auto t) {
            using Tl = decltype(t);
            return launch_conv_pos_t<Tl::RTW, Tl::NWAVES>(st, in, Wp, bias, res, out, B, n, Cpad, CoutP, out_stride, cout_valid, relu, Tl::PW, Tl::CTW);
        });
    if (conv_lds_bytes(2, n, Cpad) > 160 * 1024) {  // wide inputs (data gradient of the 6×6 policy head): 64-row tiles
        if (CoutP % 128 == 0) return launch_conv_t<1, 2>(st, in, Wp, bias, res, out, M, n, Cpad, CoutP, out_stride, cout_valid, relu);
        return launch_conv_t<1, 1>(st, in, Wp, bias, res, out, M, n, Cpad, CoutP, out_stride, cout_valid, relu);
    }
    if (CoutP % 128 == 0) return launch_conv_t<2, 2>(st, in, Wp, bias, res, out, M, n, Cpad, CoutP, out_stride, cout_valid, relu);
    return launch_conv_t<2, 1>(st, in, Wp, bias, res, out, M, n, Cpad, CoutP, out_stride, cout_valid, relu);
}

}  // namespace tg
