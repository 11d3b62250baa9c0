// tower_stage.cuh — what the fused towers share around their main loops: the exact-f32 towers (tower_kernels.hip: k_tower, k_tower_halo,
// k_tower_sq, k_tower_split) and the split-bf16 towers (net_s3_kernels.hip: k_tower_s3, k_tower_s3_halo) differ in their LDS image and
// their main loop.  Here: the constant planes of game_repr as a per-position bias of layer 0 (TowerParams.cb / TowerS3Params.cb),
// layer 0 of the exact-f32 towers as a sum of weight rows (tower_cb_layer0), and the ReLU on a quad of every epilogue.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "board.cuh"
#include "conv_mainloop.cuh"

namespace tg {

// PB[position p][border class][F] = bias + Σ_{constant planes that are set} S[plane][class] + fcd · S[fcd plane][class], summed in
// exactly this order by every kernel that uses it (a position's result must not depend on the kernel that evaluates it).
// class = 3·(y = 0 ? 0 : y = n − 1 ? 2 : 1) + (x = 0 ? 0 : x = n − 1 ? 2 : 1): which of the 9 taps stay on the board.
// Called by the whole wave that holds position p's state; F4 = F / 4; S4 = S as float4; B4 = the layer's bias as float4.
__device__ __forceinline__ void tower_cb_table(const WState& ws, float fcd, int n, int p, int F4, const f32x4* __restrict__ S4,
                                               const f32x4* __restrict__ B4, f32x4* pb4) {
    const int lane = threadIdx.x & 63;
    int st0, cp0;
    starting_stones(n, st0, cp0);
    // the constant planes that are set (ws_row_mask's rules), as indices into S
    const bool w = ws.to_move == 0;
    const int my_st = w ? ws.ws : ws.bs, en_st = w ? ws.bs : ws.ws, my_cp = w ? ws.wc : ws.bc, en_cp = w ? ws.bc : ws.wc;
    int pl[5];
    pl[0] = (my_st > 0 && my_st <= st0) ? my_st - 1 : -1;
    pl[1] = (en_st > 0 && en_st <= st0) ? st0 + en_st - 1 : -1;
    pl[2] = (my_cp > 0 && my_cp <= cp0) ? 2 * st0 + my_cp - 1 : -1;
    pl[3] = (en_cp > 0 && en_cp <= cp0) ? 2 * st0 + cp0 + en_cp - 1 : -1;
    pl[4] = w ? 2 * st0 + 2 * cp0 : -1;
    const int fplane = 2 * st0 + 2 * cp0 + 1;
    for (int idx0 = 0; idx0 < 9 * F4; idx0 += 64) {  // idx = class·F/4 + channel quad
        const int idx = min(idx0 + lane, 9 * F4 - 1);
        const int cls = idx / F4;
        // all seven rows are requested before the first add (a row behind `if (plane is set)` was a load the next one waited
        // for: six L2 round trips in a row, per round and position); an unset plane reads row 0 and is not added — the sum
        // and its order are those of the conditional form, bit for bit
        f32x4 v = B4[idx - cls * F4];
        f32x4 t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) t[k] = S4[(size_t)(pl[k] >= 0 ? pl[k] : 0) * 9 * F4 + idx];
        const f32x4 sf = S4[(size_t)fplane * 9 * F4 + idx];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const f32x4 u = v + t[k];
            v = pl[k] >= 0 ? u : v;
        }
        v += f32x4{fcd * sf[0], fcd * sf[1], fcd * sf[2], fcd * sf[3]};
        if (idx0 + lane < 9 * F4) pb4[(size_t)p * 9 * F4 + idx] = v;
    }
}
// the 32 board-plane values of this lane's square as eight float quads (planes ≥ board_channels(n) are zero)
__device__ __forceinline__ void tower_cb_board_quads(const RowMask& m, int n, f32x4 (&qd)[8]) {
    const uint32_t bits = m.w[0] & ((1u << board_channels(n)) - 1u);  // board_channels ≤ 28
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t nib = (bits >> (4 * k)) & 15u;
        qd[k] = f32x4{(nib & 1u) ? 1.0f : 0.0f, (nib & 2u) ? 1.0f : 0.0f, (nib & 4u) ? 1.0f : 0.0f, (nib & 8u) ? 1.0f : 0.0f};
    }
}
// index (in f32x4) of a row's entry of PB for channel quad chq
__device__ __forceinline__ int tower_cb_index(int rho, int rows, int n, int nsq, int F4, int chq) {
    if (rho >= rows) return chq;
    const int p = rho / nsq, sq = rho - p * nsq, y = sq / n, x = sq - y * n;
    const int cls = (y == 0 ? 0 : y == n - 1 ? 2 : 1) * 3 + (x == 0 ? 0 : x == n - 1 ? 2 : 1);
    return (p * 9 + cls) * F4 + chq;
}

// ---- layer 0 of the exact-f32 states-entry towers: a sum of weight rows, no MFMA ----
// A board plane holds 0 or 1, 1.0·w = w and x + 0·w = x: the output of layer 0 at square o, channel f is the per-position
// constant-plane bias plus the folded conv0 weights of the planes that are SET on o's neighbours.  tower_cb_layer0 is the only
// place where k_tower, k_tower_halo, k_tower_sq and k_tower_split (tower_kernels.hip, TowerParams.cb) compute it, in this order:
//
//   y[p][o][f] = relu( (…((PB[p][class(o)][f] + R[c₁][t₁][f]) + R[c₂][t₁][f]) + … ) )
//
//   · taps t = 3·ky + kx ascending, over the taps of o that stay on the board (neighbour (y + ky − 1, x + kx − 1));
//   · within a tap the set planes c of the neighbour in ascending plane index (its top one-hot, planes 0 – 5, then its buried
//     stones, planes ≥ 6); a neighbour without a stone adds the row R[bc] of −0.0f, which changes no bit of any sum;
//   · PB as tower_cb_table defines it: bias, the set constant planes' S in that order, fcd · S[fcd plane] last.
// That order is the contract that keeps a position's bits independent of the kernel (and batch size) that evaluates it.
//
// R = TowerParams.w0_rows (net_pack.h pack_board_rows): [plane ≤ bc][tap][F].  Mapping: one wave per position, lanes are
// CHANNELS (lane → channel ch; a tower of 128 filters makes two passes), the n² sums are registers.  Ascending taps of o are
// ascending neighbour squares, so the wave walks the INPUT squares s in ascending order and adds each set plane's nine rows
// R[c][t] to the nine outputs o = s − offset(t): per output exactly the order above, and the nine loads of a plane are
// independent of each other.  A square's planes arrive as a scalar (v_readlane of the lane-per-square RowMask): the top one-hot
// is branch-free, its rows requested one board row ahead; the buried stones, rarer, take a scalar loop.
// sink(o, y) receives every output of channel ch, o static.  (The scheduling barriers bound what is in flight: without them the
// compiler requests every row of the position at once and spills.)  AHEAD = false requests a board row's rows when its turn
// comes, not one row ahead: NB·9 registers less (k_tower_split, whose workgroups must stay co-resident); same sums.
template <int NB, int F, bool AHEAD, class Sink>
__device__ __forceinline__ void tower_cb_layer0(const WState& ws, float fcd, const RowMask& m, const float* __restrict__ S,
                                                const float* __restrict__ B, const float* __restrict__ R, int ch, Sink&& sink) {
    constexpr int n = NB, nsq = NB * NB, bc = (NB + 8) * 2;  // bc = board_channels(NB)
    // ---- PB[class][ch]: tower_cb_table's sum, element for element ----
    int st0, cp0;
    starting_stones(n, st0, cp0);
    const bool w = ws.to_move == 0;
    const int my_st = w ? ws.ws : ws.bs, en_st = w ? ws.bs : ws.ws, my_cp = w ? ws.wc : ws.bc, en_cp = w ? ws.bc : ws.wc;
    int pl[5];
    pl[0] = (my_st > 0 && my_st <= st0) ? my_st - 1 : -1;
    pl[1] = (en_st > 0 && en_st <= st0) ? st0 + en_st - 1 : -1;
    pl[2] = (my_cp > 0 && my_cp <= cp0) ? 2 * st0 + my_cp - 1 : -1;
    pl[3] = (en_cp > 0 && en_cp <= cp0) ? 2 * st0 + cp0 + en_cp - 1 : -1;
    pl[4] = w ? 2 * st0 + 2 * cp0 : -1;
    const int fplane = 2 * st0 + 2 * cp0 + 1;
    const unsigned uch = (unsigned)ch;  // every row is addressed as (wave-uniform base)[lane's channel]: scalar base, 32-bit lane offset
    const float b0 = B[uch];
    float pb[9];
#pragma unroll
    for (int cls = 0; cls < 9; cls++) {
        float v = b0, t[5];
#pragma unroll
        for (int k = 0; k < 5; k++) t[k] = (S + ((size_t)(pl[k] >= 0 ? pl[k] : 0) * 9 + cls) * F)[uch];
        const float sf = (S + ((size_t)fplane * 9 + cls) * F)[uch];
#pragma unroll
        for (int k = 0; k < 5; k++) {
            const float u = v + t[k];
            v = pl[k] >= 0 ? u : v;
        }
        pb[cls] = v + fcd * sf;
        if (cls % 3 == 2) __builtin_amdgcn_sched_barrier(0);
    }
    // ---- the board planes of every square as scalars; the sums start from PB of the square's border class ----
    const uint32_t bm = m.w[0] & ((1u << bc) - 1u);
    uint32_t bits[nsq];
    float acc[nsq];
#pragma unroll
    for (int o = 0; o < nsq; o++) {
        bits[o] = (uint32_t)__builtin_amdgcn_readlane((int)bm, o);
        const int y = o / n, x = o % n;
        acc[o] = pb[(y == 0 ? 0 : y == n - 1 ? 2 : 1) * 3 + (x == 0 ? 0 : x == n - 1 ? 2 : 1)];
    }
    // the rows of input square (y, x)'s top plane (or the −0.0f row), for the taps whose output stays on the board
    float top[AHEAD ? 2 : 1][NB][9];
    auto fetch_row = [&](int y, float (&buf)[NB][9]) {
#pragma unroll
        for (int x = 0; x < n; x++) {
            const uint32_t t6 = bits[y * n + x] & 63u;
            const float* rw = R + (size_t)(t6 ? __builtin_ctz(t6) : bc) * 9 * F;
#pragma unroll
            for (int t = 0; t < 9; t++) {
                const int oy = y - (t / 3 - 1), ox = x - (t % 3 - 1);
                if (oy >= 0 && oy < n && ox >= 0 && ox < n) buf[x][t] = (rw + t * F)[uch];
            }
        }
    };
    if (AHEAD) fetch_row(0, top[0]);
#pragma unroll
    for (int y = 0; y < n; y++) {
        if (!AHEAD) fetch_row(y, top[0]);
        else if (y + 1 < n) fetch_row(y + 1, top[(y + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int x = 0; x < n; x++) {
#pragma unroll
            for (int t = 0; t < 9; t++) {
                const int oy = y - (t / 3 - 1), ox = x - (t % 3 - 1);
                if (oy >= 0 && oy < n && ox >= 0 && ox < n) acc[oy * n + ox] += top[AHEAD ? y & 1 : 0][x][t];
            }
            uint32_t bur = bits[y * n + x] >> 6;  // wave-uniform: a scalar loop
            while (bur) {
                const float* rw = R + (size_t)(6 + __builtin_ctz(bur)) * 9 * F;
                bur &= bur - 1u;
                float r9[9];
#pragma unroll
                for (int t = 0; t < 9; t++) {
                    const int oy = y - (t / 3 - 1), ox = x - (t % 3 - 1);
                    if (oy >= 0 && oy < n && ox >= 0 && ox < n) r9[t] = (rw + t * F)[uch];
                }
#pragma unroll
                for (int t = 0; t < 9; t++) {
                    const int oy = y - (t / 3 - 1), ox = x - (t % 3 - 1);
                    if (oy >= 0 && oy < n && ox >= 0 && ox < n) acc[oy * n + ox] += r9[t];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int o = 0; o < nsq; o++) sink(o, fmaxf(acc[o], 0.0f));
}
// float index of (position p, square sq, channel ch) in the towers' output: plain NHWC, or the policy FC's fragment order
// (TowerParams.frag_out: per tile of 16 positions and 16-channel chunk one KB, lane (position, q))
__device__ __forceinline__ size_t tower_out_index(int frag_out, int p, int sq, int ch, int nsq, int F) {
    if (frag_out) return ((((size_t)(p >> 4) * (nsq * (F >> 4)) + sq * (F >> 4) + (ch >> 4)) * 64 + (p & 15) * 4 + ((ch & 15) >> 2)) << 2) + (ch & 3);
    return ((size_t)p * nsq + sq) * F + ch;
}

// ---- epilogue: ReLU on a quad ----
__device__ __forceinline__ f32x4 relu4(f32x4 v) {
    v[0] = fmaxf(v[0], 0.0f); v[1] = fmaxf(v[1], 0.0f); v[2] = fmaxf(v[2], 0.0f); v[3] = fmaxf(v[3], 0.0f);
    return v;
}
}  // namespace tg
