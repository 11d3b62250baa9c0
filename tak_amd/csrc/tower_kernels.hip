// tower_kernels.hip — the fused residual towers of the policy/value resnet, exact f32 (layout and arithmetic: conv_kernels.hip).
//
// Kernels, in the order of the file:
//   k_tower                 conv0 + the whole residual tower in ONE launch on the plain LDS image (one zero row for
//                           off-board taps, per-tap masks): batches below 2048 / 1024 / 512 positions
//   k_tower_split           small batches of wide networks: a position split over F / 16 workgroups by output channel tile
//   k_tower_halo            the same tower on the HALO image (zero cells between board rows and positions, taps as
//                           ds_read immediates, conflict-free slot table): full batches, 89 – 94 % of the MFMA peak
//   k_tower_sq              5×5 with 64 filters at full batches: square tiles (tile = board square, column = position), only
//                           the MFMAs of on-board taps issued (169 of 225); same bits
// Every variant performs the same products in the same order: a position's outputs are the same bits whatever batch (and
// therefore kernel) evaluates it (tests/test_gpu_net.py, tests/test_gpu_variants.py).
// Layer 0 of the states entry (TowerParams.cb) issues no MFMA in any of the four: a board plane holds 0 or 1 and a position sets
// few of them, so a square's output is the constant-plane bias plus the weight rows of its neighbours' set planes, summed by
// the one function tower_cb_layer0 (tower_stage.cuh) and stored straight into the image layer 1 reads.  The planes entry
// (arbitrary input data) and TG_NO_CONST_BIAS keep the dense layer 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "board.cuh"
#include "conv_mainloop.cuh"
#include "pos_tiling.h"
#include "tower_stage.cuh"
#include "tower_stamps.cuh"
#include "kernels.h"

namespace tg {

// ------------------------------------------------------------------------------------------------
// Fused residual tower: conv0 + R × (conv1, conv2 + skip) in ONE launch.  A workgroup keeps its PW
// positions in LDS for the whole tower: each layer's MFMA loop reads the padded NHWC image of the
// previous layer from LDS, the epilogue (bias, ReLU, skip) runs on the accumulators, and — behind a
// barrier — the wave writes its 16-channel slice straight back into the same LDS image for the next
// layer.  The skip connection never leaves registers (each wave keeps the block input of exactly the
// tiles it produces).  Only the input planes are read from HBM and only the final activations are
// written (for the policy / value heads); per layer the only global traffic is the L2-resident weights.
// ------------------------------------------------------------------------------------------------
// ---- layer 0 of the states entry (TowerParams.cb; tower_stage.cuh) ----
// The positions of one workgroup, one wave per position at a time: the wave unpacks the state (lane = square) and sums layer 0's
// weight rows with its lanes as channels (tower_cb_layer0: the constant planes as the bias PB, the set board planes' rows of
// TowerParams.w0_rows; F = 128: two passes).  put(p, o, ch, y) receives the output of this lane's channel ch at square o of the
// workgroup's position p, bias and ReLU applied: every kernel stores it where its layer 1 reads it.
template <int NWAVES, int NB, int F, class Put>
__device__ __forceinline__ void tower_stage_layer0(const uint8_t* states, int pos0, int npos, const TowerParams& T, Put&& put) {
    static_assert(F == 64 || F == 128, "lanes are channels");
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Geom geo = make_geom(NB);
    auto stage_one = [&](int p, const WRaw& raw) {
        WState ws;
        ws_unpack(ws, raw, geo);
        const float fcd = fcd_value(ws, geo);
        const RowMask m = ws_row_mask(ws, geo);
#pragma unroll 1
        for (int ch = lane; ch < F; ch += 64)
            tower_cb_layer0<NB, F, true>(ws, fcd, m, T.cplane_sums, T.b[0], T.w0_rows, ch, [&](int o, float y) { put(p, o, ch, y); });
    };
    // a wave's positions are requested two at a time (C2: 16 positions, 8 waves — one memory round trip instead of two)
    for (int p = wave; p < npos; p += 2 * NWAVES) {
        const int p1 = p + NWAVES;
        const WRaw r0 = ws_load_raw(states + (size_t)(pos0 + p) * geo.bytes, geo);
        const WRaw r1 = ws_load_raw(states + (size_t)(pos0 + (p1 < npos ? p1 : p)) * geo.bytes, geo);
        stage_one(p, r0);
        if (p1 < npos) stage_one(p1, r1);
    }
}
// the same when layer 0 is the whole tower (no residual block): straight into `out`
template <int NWAVES, int NB, int F>
__device__ __forceinline__ void tower_layer0_to_out(const uint8_t* states, int pos0, int npos, const TowerParams& T, float* __restrict__ out) {
    tower_stage_layer0<NWAVES, NB, F>(states, pos0, npos, T, [&](int p, int o, int ch, float y) {
        out[tower_out_index(T.frag_out, pos0 + p, o, ch, NB * NB, F)] = y;
    });
}

// FROM_STATES: `in` points at packed game states and the planes are encoded straight into the LDS image
// (game_repr fused into the tower: the f32 planes never touch HBM).
// CB (with FROM_STATES): layer 0 is a sum of weight rows (tower_stage_layer0) written straight into the image layer 1 reads;
// the MFMA loops start at layer 1 — CH0 = 0 and NB = the board size then.
template <int RTW, int NWAVES, int CH0, int CH, bool FROM_STATES, bool CB = false, int NB = 0>
__global__ __launch_bounds__(NWAVES * 64) void k_tower(const float* __restrict__ in, TowerParams T, float* __restrict__ out,
                                                       int B, int n, int PW, int CTW) {
    static_assert(!CB || FROM_STATES, "the constant-plane bias needs the packed states");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;
    const int tid = threadIdx.x;
    const int nsq = n * n;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int rows = npos * nsq;
    const int F = T.F;
    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW, rg = wave / CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = ct * 16;

    // ---- stage the input planes (row pitch cin_pad + 4) ----
    int Cpad = CB ? F : T.cin_pad;
    int LS4 = (Cpad + LDS_PAD16) >> 2;
    if constexpr (CB) {  // layer 0's outputs, the image of layer 1 (row pitch F + 8)
        static_assert(NB * NB > 0 && CH0 == 0, "layer 0 as a sum of rows: no main loop");
        if (T.nlayers == 1) {  // no residual block: layer 0 is the tower's output
            tower_layer0_to_out<NWAVES, NB, 16 * CH>((const uint8_t*)in, pos0, npos, T, out);
            return;
        }
        const int LS = LS4 * 4;
        tower_stage_layer0<NWAVES, NB, 16 * CH>((const uint8_t*)in, pos0, npos, T, [&](int p, int o, int ch, float y) {
            lds[(p * (NB * NB) + o) * LS + ch] = y;
        });
        for (int idx = tid; idx < LS4; idx += NWAVES * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else if (FROM_STATES) {
        const Geom geo = make_geom(n);
        const uint8_t* states = (const uint8_t*)in;
        const int C = input_channels(n);
        for (int p = wave; p < npos; p += NWAVES) {  // one wave encodes one position at a time, lane = square
            WState ws;
            ws_load(ws, states + (size_t)(pos0 + p) * geo.bytes, geo);
            const float fcd = fcd_value(ws, geo);
            const RowMask m = ws_row_mask(ws, geo);
            if (lane < nsq) {
                f32x4* row = lds4 + (size_t)(p * nsq + lane) * LS4;
                const int kl = (Cpad >> 2) - 4;  // first quad of the last 16-channel chunk
                for (int k = 0; k < kl; k++) {
                    float4 v = row_mask_value(m, k, C, fcd);
                    row[k] = f32x4{v.x, v.y, v.z, v.w};
                }
                f32x4 lc[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float4 v = row_mask_value(m, kl + k, C, fcd);
                    lc[k] = f32x4{v.x, v.y, v.z, v.w};
                }
                conv_last_chunk_store(row + kl, lc, T.cin_last_t);
            }
        }
        for (int idx = tid; idx < LS4; idx += NWAVES * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
        const int vpr = Cpad >> 2;
        const f32x4* src = (const f32x4*)(in + (size_t)pos0 * nsq * Cpad);
        const int total = rows * vpr;
        for (int idx = tid; idx < total; idx += NWAVES * 64) {
            int r = idx / vpr, v = idx - r * vpr;
            if (v < vpr - 4) lds4[r * LS4 + v] = src[idx];
        }
        for (int r = tid; r < rows; r += NWAVES * 64) {  // the last chunk of every row, permuted like the weights
            f32x4 lc[4];
#pragma unroll
            for (int k = 0; k < 4; k++) lc[k] = src[(size_t)r * vpr + vpr - 4 + k];
            conv_last_chunk_store(lds4 + (size_t)r * LS4 + vpr - 4, lc, T.cin_last_t);
        }
        for (int idx = tid; idx < LS4; idx += NWAVES * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    __syncthreads();

    // Row tiles of a full workgroup are dealt to the NWAVES / CTW row groups as evenly as they go (25 = 13 + 12 with two
    // groups, 7 + 6 + 6 + 6 with four): the first `rem` groups own RTW tiles, the others RTW - 1 and run the loop
    // specialised for that count instead of issuing a whole tile of zero MFMAs (wave-uniform branch).  The waves of one
    // channel tile (wave % CTW) land on one SIMD, so every SIMD carries all the row tiles whatever the split.
    const int NRG = NWAVES / CTW;
    const int ntiles = (PW * nsq + 15) >> 4;
    const int tbase = ntiles / NRG, trem = ntiles - tbase * NRG;
    const int my_tiles = tbase + (rg < trem ? 1 : 0);
    const int rho0 = (rg * tbase + min(rg, trem)) * 16 + r16;
    const bool short_group = my_tiles < RTW;

    // Skip connection without any storage of its own: after conv1 of a block every wave reads the block input X
    // of exactly the tiles it owns back from the LDS image (just before it overwrites them with conv1's output)
    // and uses it as the initial value of conv2's accumulators.
    f32x4 acc[RTW];
#pragma unroll
    for (int j = 0; j < RTW; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    int vmask[RTW];  // board geometry is the same for every layer
    conv_tap_masks<RTW>(rows, n, nsq, rho0, vmask);
    if (short_group) vmask[RTW - 1] = 0;  // that tile belongs to the next row group

    for (int layer = CB ? 1 : 0; layer < T.nlayers; layer++) {
        const f32x4* wp = (const f32x4*)T.w[layer] + ((size_t)(ch0 + r16) * 4 + q);
        TG_STAMP(layer, 0);
        if (RTW > 1 && short_group) {
            f32x4 (&acs)[RTW - 1] = *reinterpret_cast<f32x4 (*)[RTW - 1]>(&acc[0]);
            if constexpr (!CB) {
                if (layer == 0) conv_mainloop<RTW - 1, CH0>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho0, q, vmask, acs, T.cin_last_t);
            }
            if (CB || layer > 0) conv_mainloop<RTW - 1, CH>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho0, q, vmask, acs);
        } else {
            if constexpr (!CB) {
                if (layer == 0) conv_mainloop<RTW, CH0>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho0, q, vmask, acc, T.cin_last_t);
            }
            if (CB || layer > 0) conv_mainloop<RTW, CH>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho0, q, vmask, acc);
        }
        TG_STAMP(layer, 1);
        // ---- epilogue on the accumulators: lane holds out[row][ch0 + 4q .. 4q+3] ----
        const f32x4 bv = *(const f32x4*)&T.b[layer][ch0 + 4 * q];
#pragma unroll
        for (int j = 0; j < RTW; j++) acc[j] = relu4(acc[j] + bv);
        if (layer + 1 == T.nlayers) {
#pragma unroll
            for (int j = 0; j < RTW; j++)
                if (j < my_tiles && rho0 + j * 16 < rows) {
                    const int rho = rho0 + j * 16;
                    if (T.frag_out) {  // (tile of 16 positions, chunk = square·F/16 + channel tile) → one KB, lane (position, q)
                        const int p = pos0 + rho / nsq, sq = rho % nsq;
                        ((f32x4*)out)[((size_t)(p >> 4) * (nsq * (F >> 4)) + sq * (F >> 4) + ct) * 64 + (p & 15) * 4 + q] = acc[j];
                    } else *(f32x4*)&out[((size_t)pos0 * nsq + rho) * F + ch0 + 4 * q] = acc[j];
                }
            break;
        }
        TG_STAMP(layer, 2);
        __syncthreads();  // every wave has finished reading the previous image
        TG_STAMP(layer, 3);
        const int LS4n = (F + LDS_PAD16) >> 2;
        const bool conv1 = (layer & 1) == 1;  // next layer is conv2 of the same block: it starts from the block input
        Cpad = F;
        LS4 = LS4n;
        // tile by tile: read the own tile of X (the initial value of conv2's accumulator), overwrite it with this layer's
        // output — no second register set (at layer 0 the pitch changes: conv1 is false there, nothing is read back)
#pragma unroll
        for (int j = 0; j < RTW; j++) {
            f32x4 x0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (j < my_tiles && rho0 + j * 16 < rows) {
                const int at = (rho0 + j * 16) * LS4 + (ch0 >> 2) + q;
                if (conv1) x0 = lds4[at];
                lds4[at] = acc[j];
            }
            acc[j] = x0;
        }
        if (layer == 0)
            for (int idx = tid; idx < LS4; idx += NWAVES * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        TG_STAMP(layer, 4);
        __syncthreads();
        TG_STAMP(layer, 5);
    }
}

// ------------------------------------------------------------------------------------------------
// The fused tower for SMALL batches of wide networks (round 6): k_tower gives every position to one workgroup — at the reference's
// own constants (32 lock-step games → 32 leaves per forward, Net6 = 16 blocks × 128 filters; train/src/self_play.rs:94,
// alpha-tak/src/model/net6.rs:16-17) that is 32 busy CUs of 256, each issuing 8 channel tiles × 3 row tiles × 288 MFMAs per layer
// (23 µs per layer, 882 µs per forward).  Here a position is SPLIT over G = F / 16 workgroups by output channel tile (G = 8 at
// F = 128, G = 4 at F = 64: the two that launch_tower_split instantiates): workgroup
// (position p, group g) holds the whole input image of p in LDS and computes CTW channel tiles × NRT row tiles, one (row tile, channel
// tile) pair per wave = ONE chain of 9·16·CH/4 MFMAs — the shortest critical path the arithmetic allows (a chain cannot be cut: every
// output element is accumulated over k in k_tower's order, so the results are bit-identical).  Between two layers the G workgroups of a
// position exchange their 16·CTW-channel slices through global memory (two buffers used in turn; L2-resident: n²·F floats per
// position) and meet at a counter per position: slice stored → release → flag += 1; wait for flag = G·(layer + 1) → acquire → stage the
// next image.  Workgroup ids come in blocks of 8 positions × G groups with the position's low bits in the id's low bits, so the siblings
// of a position sit on one XCD (id mod 8) and the exchange stays in that XCD's L2 (SAME_L2, below; without that guarantee agent-scope
// fences make it correct wherever they sit).  Weights: a wave with one tile issues 4 MFMAs per 16-k chunk — far less than an L2 round
// trip — so they are fetched a whole TAP ahead (CH quads per lane, two sets) instead of two chunks ahead.  What bounds a layer is the
// chain itself: 288 DEPENDENT MFMAs at 46 cycles each (6.0 µs of a layer's 8.2; scripts/probes/split_stamps.hip).
// A workgroup never waits for more than its own G − 1 siblings, all of one launch whose grid (≤ 512 three-wave workgroups on 6×6, ≤ 1024
// two-wave ones on 5×5) is co-resident, and whose ids put a position's siblings within 8·G of each other in the dispatch order; the wait
// is bounded all the same: after SPLIT_SPIN_LIMIT polls it raises T.split_err (→ TG_ERR_HIP on the host) and the waits stop.
// ------------------------------------------------------------------------------------------------
constexpr unsigned SPLIT_SPIN_LIMIT = 1u << 21;
constexpr int SPLIT_FLAG_STRIDE = 32;  // u32 words between two positions' counters (kernels.h: TOWER_SPLIT_CTL_WORDS)

// SAME_L2: the launcher has verified on this device that workgroup id i runs on XCD i mod 8 (k_xcc_probe), so a position's siblings
// share one L2 and the exchange needs no agent-scope fences — those write back and INVALIDATE the XCD's whole L2 (buffer_wbl2 sc1 /
// buffer_inv sc1: 256 workgroups × every layer), after which every weight load of the next layer misses it (tower 359 against 252 µs).
// What it needs instead: the slice's stores complete (the vector L1 writes through: s_waitcnt vmcnt(0) = in L2), the counter as an L2
// atomic polled at device scope, and the image staged with device-scope loads (sc1: past this CU's L1).  Without the guarantee: the
// agent-scope fences, correct wherever the siblings sit.  (Measured and not kept, profiles/r06_k_split_exchange_variants.txt: the data as
// its own flag — three sentinel-filled buffers polled directly, no counter: 242 µs, i.e. the exchange is the siblings' skew, not the
// protocol's round trips.)
template <int NRT, int CTW, int CH, bool SAME_L2>
__global__ __launch_bounds__(NRT * CTW * 64) void k_tower_split(const uint8_t* __restrict__ states, TowerParams T, float* __restrict__ out,
                                                                float* __restrict__ scratch, int B, int n) {
    constexpr int NW = NRT * CTW, F = 16 * CH, F4 = F / 4;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;
    const int tid = threadIdx.x, nsq = n * n, rows = nsq;
    // workgroup id → (position, channel group): ids come in blocks of 8·G — 8 consecutive positions × their G groups — with the
    // position's low three bits in the id's low three bits: the G siblings of a position are dispatched within 8·G consecutive ids
    // (they never wait for a workgroup far behind them in the dispatch order) and land on one XCD (id mod 8), so their exchange
    // stays in that XCD's L2
    constexpr int G = (CH / CTW);
    const int blk = blockIdx.x / (8 * G), rem = blockIdx.x - blk * (8 * G);
    const int p = blk * 8 + (rem & 7), g = rem >> 3;
    if (p >= B) return;
    // the guarantee the fast exchange rests on — a position's siblings on ONE XCD — is checked by every workgroup of every launch:
    // group 0 posts its XCD in the position's counter line, the others compare at the first meeting (the dispatcher's round robin may
    // start anywhere, so the id alone does not name the XCD; ids that agree mod 8 share one — k_xcc_probe)
    unsigned my_xcc = 0;
    if (SAME_L2 && tid == 0) {
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(my_xcc));
        my_xcc = (my_xcc & 15u) + 1u;
    }
    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW, rt = wave / CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = (g * CTW + ct) * 16;
    const int rho = rt * 16 + r16;  // this lane's row (square) of the position; ≥ rows: padding of the last row tile
    unsigned* flag = T.split_flags + (size_t)p * SPLIT_FLAG_STRIDE;  // a 128-byte line per position: its 8 pollers contend with nobody else

    int LS4 = (F + LDS_PAD16) >> 2;
    int vmask[1];
    conv_tap_masks<1>(rows, n, nsq, rho, vmask);
    f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    bool failed = false;  // (thread 0) a wait ran into its bound: no further waits
    const size_t wlane = (size_t)(ch0 + r16) * 4 + q;
    f32x4 wf[CH];  // the first tap's weights of the NEXT layer: requested before the wait for the siblings, there when it ends
    for (int layer = 0; layer < T.nlayers; layer++) {
        // two exchange buffers used in turn (`out` is written by the last layer only: in the FC's fragment order a position's output
        // lies across the rows of 15 others)
        float* xbuf = scratch + (size_t)(layer & 1) * TOWER_SPLIT_MAX_BATCH * nsq * F;
        TG_STAMP(layer, 0);
        if (layer == 0) {
            // layer 0 is a sum of weight rows (tower_cb_layer0, the one function every tower calls; lanes are channels): wave 0 sums
            // this workgroup's slice of 16·CTW channels of position p and stores it into the exchange buffer like every other
            // layer's, or into `out` when it is the tower's output
            const bool last = T.nlayers == 1;
            if (wave == 0) {
                static_assert(CTW * 16 <= 64, "the workgroup's channels in one pass");
                const int ch = g * CTW * 16 + (lane & (CTW * 16 - 1));  // (the lanes beyond the slice repeat it and store nothing)
                float* dst = last ? out + tower_out_index(T.frag_out, p, 0, ch, nsq, F) : xbuf + (size_t)p * nsq * F + ch;
                const int ostep = last && T.frag_out ? CH * 256 : F;  // floats between two squares of a position in `out` / xbuf
                auto put = [&](int o, float y) {
                    if (lane < CTW * 16) dst[o * ostep] = y;
                };
                WState ws;
                const Geom geo = make_geom(n);
                ws_load(ws, states + (size_t)p * geo.bytes, geo);
                const float fcd = fcd_value(ws, geo);
                const RowMask m = ws_row_mask(ws, geo);
                // (opaque to the compiler: this branch does not change from layer to layer, and it would compute every row address
                // before the layer loop and keep a hundred registers of them through all layers)
                const float *S = T.cplane_sums, *R = T.w0_rows;
                asm volatile("" : "+s"(S), "+s"(R));
                if (n == 5) tower_cb_layer0<5, F, false>(ws, fcd, m, S, T.b[0], R, ch, put);
                else tower_cb_layer0<6, F, false>(ws, fcd, m, S, T.b[0], R, ch, put);
            }
            TG_STAMP(layer, 1);
            if (last) break;
        } else {
            const f32x4* wp = (const f32x4*)T.w[layer] + wlane;
            const f32x4 bv = *(const f32x4*)&T.b[layer][ch0 + 4 * q];
            conv_mainloop_tile<CH>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho, q, vmask[0], acc, wf);
            TG_STAMP(layer, 1);
            const f32x4 v = relu4(acc + bv);
            if (layer + 1 == T.nlayers) {
                if (rho < rows) {
                    if (T.frag_out) ((f32x4*)out)[((size_t)(p >> 4) * (nsq * CH) + rho * CH + (ch0 >> 4)) * 64 + (p & 15) * 4 + q] = v;
                    else *(f32x4*)&out[((size_t)p * nsq + rho) * F + ch0 + 4 * q] = v;
                }
                break;
            }
            // the block input of conv2's accumulator: this wave's own slice of the image conv1 has just read (k_tower's skip path)
            f32x4 x0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if ((layer & 1) == 1 && rho < rows) x0 = lds4[rho * LS4 + (ch0 >> 2) + q];
            acc = x0;
            if (rho < rows) *(f32x4*)&xbuf[((size_t)p * nsq + rho) * F + ch0 + 4 * q] = v;
        }
        if (SAME_L2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __syncthreads();  // every wave's slice is in L2 (SAME_L2) / on its way and every wave has finished reading the image
        TG_STAMP(layer, 2);
        conv_tile_first_weights<CH>((const f32x4*)T.w[layer + 1] + wlane, (size_t)F * 4, wf);
        if (tid == 0) {
            if (!SAME_L2) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            if (SAME_L2 && layer == 0 && g == 0) __hip_atomic_store(flag + 1, my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned target = (unsigned)G * (unsigned)(layer + 1);
            unsigned spins = 0;
            // (device scope: a group-scope load — sc0 — may hit this CU's L1 and then never sees the siblings' atomics: measured, the
            // bounded wait fired)
            auto poll = [&]() -> unsigned { return __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
            while (!failed && poll() < target) {
                __builtin_amdgcn_s_sleep(2);
                if (++spins > SPLIT_SPIN_LIMIT) { __hip_atomic_store(T.split_err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); failed = true; }
                else if ((spins & 4095u) == 0 && __hip_atomic_load(T.split_err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) failed = true;
            }
            if (!SAME_L2) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            if (SAME_L2 && layer == 0 && !failed && __hip_atomic_load(flag + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != my_xcc)
                __hip_atomic_store(T.split_err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        TG_STAMP(layer, 3);
        // ---- the next layer's image: all F channels of position p, pitch F + 8 floats ----
        // SAME_L2: DEVICE-scope loads (sc1) — past this CU's L1, which may hold the buffer's lines of two layers ago, to the L2 the siblings'
        // stores went to.  (`buffer_inv sc0` + plain loads was 5 % faster and passed every test, but a counter polled that way saw the
        // siblings' atomics only after a long delay: the L1 was being emptied by the weight stream, not by the invalidate.)
        const f32x4* src = (const f32x4*)(xbuf + (size_t)p * nsq * F);
        const int total = nsq * F4;
        constexpr int UNR = 8;
        for (int base = 0; base < total; base += NW * 64 * UNR) {
            f32x4 tmp[UNR];
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int idx = base + u * NW * 64 + tid;
                const f32x4* a = src + (idx < total ? idx : total - 1);
                if (SAME_L2) asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=v"(tmp[u]) : "v"(a) : "memory");
                else tmp[u] = *a;
            }
            if (SAME_L2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
            for (int u = 0; u < UNR; u++) {
                const int idx = base + u * NW * 64 + tid;
                if (idx < total) lds4[(idx / F4) * LS4 + idx % F4] = tmp[u];
            }
        }
        if (layer == 0)
            for (int idx = tid; idx < LS4; idx += NW * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        __syncthreads();
        TG_STAMP(layer, 4);
    }
    // the counter returns to zero with the launch: the last of the position's G workgroups to finish resets it
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u == (unsigned)G * (unsigned)T.nlayers) {
            __hip_atomic_store(flag + 1, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(flag, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The fused tower for full batches: as k_tower, but from layer 1 on the resident image is the HALO image of
// conv_mainloop.cuh (zero cells between board rows and between positions), so the 3×3 taps are immediates and the main
// loop is nothing but ds_read_b128 / MFMA / one weight load per chunk.  Layer 0 (other pitch, once per launch) runs
// the masked loop on the plain image and writes its output straight into halo cells; with CB (the states entry) it is a
// sum of weight rows (tower_stage_layer0) written straight into the halo cells, no plain image at all.  From layer 1 on the squares
// are dealt to (row tile, lane) slots by T.slotmap (tower_halo_slotmap): a permutation of the GEMM's M dimension,
// invisible in the results, that keeps every ds_read_b128 of the loop off its neighbours' banks.
// Per-element arithmetic (taps, chunks, k-steps, bias, ReLU, skip) in k_tower's order → identical bits.
// ------------------------------------------------------------------------------------------------
// Staging of the input planes and layer 0 on the plain image (tile t = rows 16t … 16t + 15), shared by the full-batch towers
// k_tower_halo and k_tower_sq where layer 0 is dense (planes entry, TG_NO_CONST_BIAS): leaves this wave's layer-0 outputs (bias and ReLU applied) of rows rho0 + 16j, j < my_tiles, in acc
// and requests layer 1's first two chunks of weights into w0 / w1.  The caller synchronises before it overwrites the image.
template <int RTW, int NWAVES, int CH0, int CH, int NB, bool FROM_STATES>
__device__ __forceinline__ void tower_plain_layer0(const float* __restrict__ in, const TowerParams& T, f32x4* lds4, int PW, int pos0,
                                                   int npos, int CTW, uint32_t wlane, f32x4 (&acc)[RTW], int& rho0_out,
                                                   int& my_tiles_out, f32x4& w0, f32x4& w1) {
    constexpr int n = NB, nsq = NB * NB, F = 16 * CH;
    const int tid = threadIdx.x;
    const int rows = npos * nsq;
    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW, rg = wave / CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = ct * 16;

    // ---- stage the input planes: plain image, row pitch cin_pad + 8 floats, one zero row behind it ----
    const int Cpad = T.cin_pad;
    const int LS4 = (Cpad + LDS_PAD16) >> 2;
    if (FROM_STATES) {
        const Geom geo = make_geom(n);
        const uint8_t* states = (const uint8_t*)in;
        const int C = input_channels(n);
        for (int p = wave; p < npos; p += NWAVES) {  // one wave encodes one position at a time, lane = square
            WState ws;
            ws_load(ws, states + (size_t)(pos0 + p) * geo.bytes, geo);
            const float fcd = fcd_value(ws, geo);
            const RowMask m = ws_row_mask(ws, geo);
            if (lane < nsq) {
                f32x4* row = lds4 + (size_t)(p * nsq + lane) * LS4;
                const int kl = (Cpad >> 2) - 4;  // first quad of the last 16-channel chunk
                for (int k = 0; k < kl; k++) {
                    float4 v = row_mask_value(m, k, C, fcd);
                    row[k] = f32x4{v.x, v.y, v.z, v.w};
                }
                f32x4 lc[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float4 v = row_mask_value(m, kl + k, C, fcd);
                    lc[k] = f32x4{v.x, v.y, v.z, v.w};
                }
                conv_last_chunk_store(row + kl, lc, T.cin_last_t);
            }
        }
    } else {
        const int vpr = Cpad >> 2;
        const f32x4* src = (const f32x4*)(in + (size_t)pos0 * nsq * Cpad);
        const int total = rows * vpr;
        for (int idx = tid; idx < total; idx += NWAVES * 64) {
            int r = idx / vpr, v = idx - r * vpr;
            if (v < vpr - 4) lds4[r * LS4 + v] = src[idx];
        }
        for (int r = tid; r < rows; r += NWAVES * 64) {  // the last chunk of every row, permuted like the weights
            f32x4 lc[4];
#pragma unroll
            for (int k = 0; k < 4; k++) lc[k] = src[(size_t)r * vpr + vpr - 4 + k];
            conv_last_chunk_store(lds4 + (size_t)r * LS4 + vpr - 4, lc, T.cin_last_t);
        }
    }
    for (int idx = tid; idx < LS4; idx += NWAVES * 64) lds4[rows * LS4 + idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();

    // row tiles dealt to the row groups as in k_tower
    const int NRG = NWAVES / CTW;
    const int ntiles = (PW * nsq + 15) >> 4;
    const int tbase = ntiles / NRG, trem = ntiles - tbase * NRG;
    const int my_tiles = tbase + (rg < trem ? 1 : 0);
    const int tile0 = rg * tbase + min(rg, trem);
    const bool short_group = my_tiles < RTW;

#pragma unroll
    for (int j = 0; j < RTW; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // ---- layer 0 ----
    const int rho0 = tile0 * 16 + r16;
    int vmask[RTW];
    conv_tap_masks<RTW>(rows, n, nsq, rho0, vmask);
    if (short_group) vmask[RTW - 1] = 0;
    const f32x4* wp = (const f32x4*)T.w[0] + ((size_t)(ch0 + r16) * 4 + q);
    const int last_t0 = T.cin_last_t;
    TG_STAMP(0, 0);
    if (RTW > 1 && short_group) {
        f32x4 (&acs)[RTW - 1] = *reinterpret_cast<f32x4 (*)[RTW - 1]>(&acc[0]);
        conv_mainloop<RTW - 1, CH0>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho0, q, vmask, acs, last_t0);
    } else {
        conv_mainloop<RTW, CH0>(lds4, wp, (size_t)F * 4, LS4, rows, n, rho0, q, vmask, acc, last_t0);
    }
    TG_STAMP(0, 1);
    if (T.nlayers > 1) conv_halo_first_weights<CH>(T.w[1], wlane, w0, w1);  // in flight during the change of images
    const f32x4 bv = *(const f32x4*)&T.b[0][ch0 + 4 * q];
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        acc[j] = relu4(acc[j] + bv);
    }
    rho0_out = rho0;
    my_tiles_out = my_tiles;
}

template <int RTW, int NWAVES, int CH0, int CH, int NB, bool FROM_STATES, bool CB = false>
__global__ __launch_bounds__(NWAVES * 64) void k_tower_halo(const float* __restrict__ in, TowerParams T, float* __restrict__ out,
                                                            int B, int PW, int CTW) {
    static_assert(!CB || FROM_STATES, "the constant-plane bias needs the packed states");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;
    TG_STAMP(0, 6);  // kernel start (diagnostic build only)
    constexpr int n = NB, nsq = NB * NB, RS = NB + 1, LEAD = NB + 2, F = 16 * CH, P4 = 4 * CH + 1;
    const int PS = T.halo_ps;
    const int tid = threadIdx.x;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int rows = npos * nsq;
    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = ct * 16;
    const uint32_t wlane = (uint32_t)(((ch0 + r16) * 4 + q) * 16);  // this lane's 16 B inside a chunk of weights
    f32x4 w0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, w1 = w0;                // the weight stream's two chunks in flight between layers
    f32x4 acc[RTW];
    int rho0, my_tiles;
    if constexpr (CB) {
        // ---- layer 0 as a sum of weight rows, straight into the halo image ----
        static_assert(CH0 == 0, "layer 0 as a sum of rows: no main loop");
        if (T.nlayers == 1) {  // no residual block: layer 0 is the tower's output
            tower_layer0_to_out<NWAVES, NB, F>((const uint8_t*)in, pos0, npos, T, out);
            return;
        }
        conv_halo_first_weights<CH>(T.w[1], wlane, w0, w1);  // in flight while layer 0 is summed
        // row tiles dealt to the row groups as in k_tower
        const int NRG = NWAVES / CTW, rg = wave / CTW;
        const int ntiles = (PW * nsq + 15) >> 4;
        const int tbase = ntiles / NRG, trem = ntiles - tbase * NRG;
        my_tiles = tbase + (rg < trem ? 1 : 0);
        rho0 = (rg * tbase + min(rg, trem)) * 16 + r16;
        // the zero cells of the image (they are never written again), and the cells of the positions a ragged workgroup lacks (their
        // slots are computed and never stored; what they read must be finite)
        const int cells = LEAD + PW * PS + 1;  // + the spare cell of the idle slots
        for (int idx = tid; idx < cells * P4; idx += NWAVES * 64) {
            const int c = idx / P4 - LEAD;
            const int o = c < 0 || c >= PW * PS ? n * RS : c % PS;  // offset inside the position block; rows of RS cells, then the zero row
            if (o >= n * RS || o % RS == n || c / PS >= npos) lds4[idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        tower_stage_layer0<NWAVES, NB, F>((const uint8_t*)in, pos0, npos, T, [&](int p, int o, int ch, float y) {
            lds[(LEAD + p * PS + (o / n) * RS + o % n) * (P4 * 4) + ch] = y;
        });
#pragma unroll
        for (int j = 0; j < RTW; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        TG_STAMP(0, 0); TG_STAMP(0, 1); TG_STAMP(0, 2);  // (no main loop, no epilogue: layer 0 is part of the staging)
        __syncthreads();
        TG_STAMP(0, 3); TG_STAMP(0, 4); TG_STAMP(0, 5);
    } else tower_plain_layer0<RTW, NWAVES, CH0, CH, NB, FROM_STATES>(in, T, lds4, PW, pos0, npos, CTW, wlane, acc, rho0, my_tiles, w0, w1);
    const bool short_group = my_tiles < RTW;
    const int tile0 = (rho0 - r16) >> 4;
    if constexpr (!CB) {
        TG_STAMP(0, 2);
        __syncthreads();  // every wave has finished reading the input planes
        TG_STAMP(0, 3);
        // the halo image replaces them: zero cells first (they are never written again), then this layer's output
        const int cells = LEAD + PW * PS + 1;  // + the spare cell of the idle slots
        for (int idx = tid; idx < cells * P4; idx += NWAVES * 64) {
            const int c = idx / P4 - LEAD;
            const int o = c < 0 || c >= PW * PS ? n * RS : c % PS;  // offset inside the position block; rows of RS cells, then the zero row
            if (o >= n * RS || o % RS == n) lds4[idx] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < RTW; j++) {
            const int rho = rho0 + j * 16;
            if (j < my_tiles && rho < PW * nsq) {
                const int p = rho / nsq, sq = rho - p * nsq, y = sq / n, x = sq - y * n;
                lds4[(LEAD + p * PS + y * RS + x) * P4 + (ch0 >> 2) + q] = acc[j];
            }
            acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        TG_STAMP(0, 4);
        __syncthreads();
        TG_STAMP(0, 5);
    }

    // ---- layers 1 … : slot (tile, lane) → square through the slot table ----
    int cell4[RTW], rowid[RTW], addr4[RTW];
#pragma unroll
    for (int j = 0; j < RTW; j++) {
        const uint32_t e = j < my_tiles ? T.slotmap[(tile0 + j) * 16 + r16] : 0xFFFF0000u;
        rowid[j] = (int)(e >> 16);                                      // 0xFFFF: slot without a square
        const bool idle = rowid[j] == 0xFFFF;  // such a slot reads around a zero cell and writes the spare cell behind the image
        cell4[j] = (idle ? LEAD + PW * PS : (int)(e & 0xFFFFu)) * P4 + (ch0 >> 2) + q;  // this lane's 4 output channels of the square
        addr4[j] = ((idle ? LEAD + n * RS : (int)(e & 0xFFFFu)) - LEAD) * P4 + q;       // B-operand base: tap (-1,-1), chunk 0
    }
    const int turn = (wave >> 2) & 1;  // waves w and w + 4 share a SIMD
    for (int layer = 1; layer < T.nlayers; layer++) {
        // the addresses are the same in every layer, but the compiler must not know: it would hoist all 9·RTW
        // (address + tap offset) sums out of the layer loop and spill them instead of using ds_read immediates
#pragma unroll
        for (int j = 0; j < RTW; j++) asm volatile("" : "+v"(addr4[j]));
        TG_STAMP(layer, 0);
        const float* wnext = T.w[layer + 1 < T.nlayers ? layer + 1 : layer];
        const f32x4 bv = *(const f32x4*)&T.b[layer][ch0 + 4 * q];  // requested here: its latency passes under the main loop
        if (RTW > 1 && short_group) {
            f32x4 (&acs)[RTW - 1] = *reinterpret_cast<f32x4 (*)[RTW - 1]>(&acc[0]);
            conv_mainloop_halo<RTW - 1, CH, NB>(lds4, T.w[layer], wnext, wlane, addr4, acs, turn, w0, w1);
        } else {
            conv_mainloop_halo<RTW, CH, NB>(lds4, T.w[layer], wnext, wlane, addr4, acc, turn, w0, w1);
        }
        TG_STAMP(layer, 1);
#pragma unroll
        for (int j = 0; j < RTW; j++) acc[j] = relu4(acc[j] + bv);
        if (layer + 1 == T.nlayers) {
#pragma unroll
            for (int j = 0; j < RTW; j++)
                if (rowid[j] < rows) {
                    if (T.frag_out) {
                        const int p = pos0 + rowid[j] / nsq, sq = rowid[j] % nsq;
                        ((f32x4*)out)[((size_t)(p >> 4) * (nsq * CH) + sq * CH + ct) * 64 + (p & 15) * 4 + q] = acc[j];
                    } else *(f32x4*)&out[((size_t)pos0 * nsq + rowid[j]) * F + ch0 + 4 * q] = acc[j];
                }
            break;
        }
        TG_STAMP(layer, 2);
        __syncthreads();  // every wave has finished reading the previous image
        TG_STAMP(layer, 3);
        const bool conv1 = (layer & 1) == 1;  // next layer is conv2 of the same block: it starts from the block input
#pragma unroll
        for (int j = 0; j < RTW; j++) {  // no per-tile branches: idle slots have their own cell
            f32x4 x0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (conv1) x0 = lds4[cell4[j]];
            lds4[cell4[j]] = acc[j];
            acc[j] = x0;
        }
        TG_STAMP(layer, 4);
        __syncthreads();
        TG_STAMP(layer, 5);
    }
}

// ------------------------------------------------------------------------------------------------
// The fused tower of 5×5 boards with 64 filters at full batches (16 positions per workgroup) on the square-tile image of
// conv_mainloop_sq — row tile = board square, tile column = position of the workgroup — whose main loop issues the MFMAs
// of the on-board taps only: 169 of the 225 (square, tap) pairs.
// Layer 0 with the constant planes as a bias (CB, the states entry) is a sum of weight rows (tower_stage_layer0): the wave that
// unpacks a position writes its 25 × 64 outputs straight into the position's cells, no main loop, no image of the planes.
// Without CB (planes entry, 80 input channels) layer 0 stays on the plain image as in k_tower_halo.
// Waves w = 4·rg + ct: channel tile ct, row group rg (its squares: sq_tile); waves w and w + 4 share a SIMD.
// Per-element arithmetic in k_tower's order, minus additions of exact zeros → identical bits.
// ------------------------------------------------------------------------------------------------
// the last layer's outputs of this lane's position p (one contiguous KB per tile in the FC's fragment order)
template <int RG, int CH>
__device__ __forceinline__ void tower_sq_store(const f32x4 (&acc)[13], const TowerParams& T, float* __restrict__ out, int p, int q, int ct) {
    constexpr int nsq = SQ_NB * SQ_NB;
#pragma unroll
    for (int j = 0; j < sq_tiles(RG); j++) {
        const int sq = sq_tile(RG, j);
        if (T.frag_out) ((f32x4*)out)[((size_t)(p >> 4) * (nsq * CH) + sq * CH + ct) * 64 + (p & 15) * 4 + q] = acc[j];
        else *(f32x4*)&out[((size_t)p * nsq + sq) * (16 * CH) + ct * 16 + 4 * q] = acc[j];
    }
}
// a layer's outputs into the image; conv1 → acc = the block input the next layer (conv2) starts from
template <int RG, int CH>
__device__ __forceinline__ void tower_sq_writeback(f32x4* cell4, f32x4 (&acc)[13], bool conv1) {
#pragma unroll
    for (int j = 0; j < sq_tiles(RG); j++) {
        const int o = sq_tile(RG, j) * sq_image_cell4<CH>();
        f32x4 x0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (conv1) x0 = cell4[o];
        cell4[o] = acc[j];
        acc[j] = x0;
    }
}

template <int CH0, bool FROM_STATES, bool CB = false>
__global__ __launch_bounds__(512) void k_tower_sq(const float* __restrict__ in, TowerParams T, float* __restrict__ out, int B) {
    static_assert(!CB || FROM_STATES, "the constant-plane bias needs the packed states");
    constexpr int RTW = 13, NWAVES = 8, CTW = 4, CH = 4, NB = SQ_NB, nsq = NB * NB, PW = 16;
    constexpr int PP4 = sq_image_pitch4<CH>(), CP4 = sq_image_cell4<CH>();  // position / cell pitch of the image in 16 B
    extern __shared__ __attribute__((aligned(16))) float lds[];
    f32x4* lds4 = (f32x4*)lds;
    TG_STAMP(0, 6);  // kernel start (diagnostic build only)
    const int tid = threadIdx.x;
    const int pos0 = blockIdx.x * PW;
    const int npos = min(PW, B - pos0);
    const int wave = tid >> 6, lane = tid & 63;
    const int ct = wave % CTW, rg = wave / CTW;
    const int r16 = lane & 15, q = lane >> 4;
    const int ch0 = ct * 16;
    const uint32_t wlane = (uint32_t)(((ch0 + r16) * 4 + q) * 16);  // this lane's 16 B inside a chunk of weights
    f32x4 w0 = f32x4{0.0f, 0.0f, 0.0f, 0.0f}, w1 = w0;                // the weight stream's two chunks in flight between layers
    f32x4 acc[RTW];
    int ad = r16 * PP4 + q;  // this lane's tile column is position r16
    const int turn = rg;     // waves w and w + 4 share a SIMD
    if constexpr (CB) {
        // ---- layer 0 as a sum of weight rows, straight into the square-tile image ----
        static_assert(CH0 == 0, "layer 0 as a sum of rows: no main loop");
        if (T.nlayers == 1) {  // no residual block: layer 0 is the tower's output
            tower_layer0_to_out<NWAVES, NB, 16 * CH>((const uint8_t*)in, pos0, npos, T, out);
            return;
        }
        conv_halo_first_weights<CH>(T.w[1], wlane, w0, w1);  // in flight while layer 0 is summed
        tower_stage_layer0<NWAVES, NB, 16 * CH>((const uint8_t*)in, pos0, npos, T, [&](int p, int o, int ch, float y) {
            lds[(p * PP4 + o * CP4) * 4 + ch] = y;
        });
        // the positions a ragged workgroup lacks get zero cells (their columns are computed and never stored; what they read must be
        // finite)
        for (int idx = tid; idx < (PW - npos) * nsq * 4 * CH; idx += NWAVES * 64) {
            const int c = idx / (4 * CH);
            lds4[(npos + c / nsq) * PP4 + (c % nsq) * CP4 + idx % (4 * CH)] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < RTW; j++) acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        TG_STAMP(0, 0); TG_STAMP(0, 1); TG_STAMP(0, 2);  // (no main loop, no epilogue: layer 0 is part of the staging)
        __syncthreads();
        TG_STAMP(0, 3); TG_STAMP(0, 4); TG_STAMP(0, 5);
    } else {  // layer 0 on the plain image (tile = 16 consecutive rows), then the change of images
        int rho0, my_tiles;
        tower_plain_layer0<RTW, NWAVES, CH0, CH, NB, FROM_STATES>(in, T, lds4, PW, pos0, npos, CTW, wlane, acc, rho0, my_tiles, w0, w1);
        if (T.nlayers == 1) {  // no residual block: layer 0 is the tower's output
#pragma unroll
            for (int j = 0; j < RTW; j++) {
                const int rho = rho0 + j * 16;
                if (j < my_tiles && rho < npos * nsq) {
                    const int p = pos0 + rho / nsq, sq = rho % nsq;
                    if (T.frag_out) ((f32x4*)out)[((size_t)(p >> 4) * (nsq * CH) + sq * CH + ct) * 64 + (p & 15) * 4 + q] = acc[j];
                    else *(f32x4*)&out[((size_t)pos0 * nsq + rho) * (16 * CH) + ch0 + 4 * q] = acc[j];
                }
            }
            return;
        }
        TG_STAMP(0, 2);
        __syncthreads();  // every wave has finished reading the input planes
        TG_STAMP(0, 3);
        // the square-tile image replaces them.  Every cell of all PW positions is written: the rows of a ragged workgroup's missing
        // positions read the zero row in layer 0, so their cells hold finite values (bias, ReLU) that later layers read and never store
#pragma unroll
        for (int j = 0; j < RTW; j++) {
            const int rho = rho0 + j * 16;
            if (j < my_tiles) {
                const int p = rho / nsq, sq = rho - p * nsq;
                lds4[p * PP4 + sq * CP4 + (ch0 >> 2) + q] = acc[j];
            }
            acc[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        TG_STAMP(0, 4);
        __syncthreads();
        TG_STAMP(0, 5);
    }

    // ---- layers 1 … ----
    for (int layer = 1; layer < T.nlayers; layer++) {
        // (the address is the same in every layer, but the compiler must not know: it would hoist the (address + offset) sums of
        // the main loop out of the layer loop and spill them instead of using ds_read immediates)
        asm volatile("" : "+v"(ad));
        const f32x4* img4 = lds4 + ad;
        TG_STAMP(layer, 0);
        const float* wnext = T.w[layer + 1 < T.nlayers ? layer + 1 : layer];
        const f32x4 bv = *(const f32x4*)&T.b[layer][ch0 + 4 * q];  // requested here: its latency passes under the main loop
        if (rg == 0) conv_mainloop_sq<0, CH>(img4, T.w[layer], wnext, wlane, acc, turn, w0, w1);
        else conv_mainloop_sq<1, CH>(img4, T.w[layer], wnext, wlane, acc, turn, w0, w1);
        TG_STAMP(layer, 1);
#pragma unroll
        for (int j = 0; j < RTW; j++) acc[j] = relu4(acc[j] + bv);
        if (layer + 1 == T.nlayers) {
            if (r16 < npos) {
                // (opaque to the compiler, like the image address: it would otherwise compute all 2 × 13 64-bit store addresses
                // before the layer loop and keep them in scratch)
                int p = pos0 + r16;
                asm volatile("" : "+v"(p));
                if (rg == 0) tower_sq_store<0, CH>(acc, T, out, p, q, ct);
                else tower_sq_store<1, CH>(acc, T, out, p, q, ct);
            }
            break;
        }
        TG_STAMP(layer, 2);
        __syncthreads();  // every wave has finished reading the previous image
        TG_STAMP(layer, 3);
        const bool conv1 = (layer & 1) == 1;  // next layer is conv2 of the same block: it starts from the block input
        f32x4* cell4 = lds4 + ad + (ch0 >> 2);
        if (rg == 0) tower_sq_writeback<0, CH>(cell4, acc, conv1);
        else tower_sq_writeback<1, CH>(cell4, acc, conv1);
        TG_STAMP(layer, 4);
        __syncthreads();
        TG_STAMP(layer, 5);
    }
}

// (CB: layer 0 needs no image of its own — its sums go straight into the image of layer 1)
template <int RTW, int NWAVES, int CH0, int CH, bool FROM_STATES, bool CB = false, int NB = 0>
static hipError_t launch_tower_t(hipStream_t st, const float* in, const TowerParams& T, float* out, int B, int n, int PW, int CTW) {
    const size_t rows1 = (size_t)(PW * n * n + 1);
    const size_t first = CB ? 0 : rows1 * (T.cin_pad + LDS_PAD16) * sizeof(float);
    const size_t later = rows1 * (T.F + LDS_PAD16) * sizeof(float);
    const size_t lds = first > later ? first : later;
    if (CB && (n != NB || !T.w0_rows)) return hipErrorInvalidValue;
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_tower<RTW, NWAVES, CH0, CH, FROM_STATES, CB, NB>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_tower<RTW, NWAVES, CH0, CH, FROM_STATES, CB, NB>), dim3((B + PW - 1) / PW), dim3(NWAVES * 64), lds, st, in, T, out, B, n, PW, CTW);
    return hipGetLastError();
}


// ---- halo image (k_tower_halo): geometry and the square → tile-slot table -------------------------
bool tower_halo_geometry(int n, int F, int* pw, int* ps) {
    // position strides found by simulating the ds_read_b128 bank groups over all tiles / taps (conflict factor ≤ 1.11)
    if (n == 5 && F == 64) { *pw = 16; *ps = 36; return true; }   // 158 848 B of LDS (with the spare cell)
    if (n == 5 && F == 128) { *pw = 8; *ps = 37; return true; }   // 160 512 B
    if (n == 6 && F == 128) { *pw = 4; *ps = 51; return true; }   // 112 464 B
    return false;
}

void tower_halo_slotmap(int n, int pw, int ps, uint32_t* out) {
    // ds_read_b128 serves lanes {0-3, 12-15} of one 16-byte slot q together with lanes {4-11} of slot q + 1 (and vice
    // versa).  With a pitch of F + 4 floats the bank quad of a read is (cell + q + 4·chunk) mod 16, so a tile whose 8
    // "outer" lanes and 8 "inner" lanes each hold 8 cells with distinct residues of ONE parity is conflict free for every
    // tap and chunk (a tap shifts all cells alike).  Greedy: per tile take one square per residue of the richer parity.
    const int nsq = n * n, RS = n + 1, LEAD = n + 2, rows = pw * nsq, tiles = (rows + 15) / 16;
    std::vector<std::vector<int>> bucket(16);
    std::vector<int> cell(rows);
    for (int r = rows - 1; r >= 0; r--) {
        const int p = r / nsq, sq = r % nsq;
        cell[r] = LEAD + p * ps + (sq / n) * RS + sq % n;
        bucket[cell[r] % 16].push_back(r);
    }
    static const int outer[8] = {0, 1, 2, 3, 12, 13, 14, 15}, inner[8] = {4, 5, 6, 7, 8, 9, 10, 11};
    for (int t = 0; t < tiles; t++) {
        size_t left[2] = {0, 0};
        for (int r = 0; r < 16; r++) left[r & 1] += bucket[r].size();
        const int par = left[0] >= left[1] ? 0 : 1;
        for (const int* slots : {outer, inner}) {
            int missing[8], nm = 0;
            for (int k = 0; k < 8; k++) {
                std::vector<int>& b = bucket[2 * k + par];
                if (!b.empty()) { out[t * 16 + slots[k]] = (uint32_t)cell[b.back()] | ((uint32_t)b.back() << 16); b.pop_back(); }
                else missing[nm++] = slots[k];
            }
            for (int m = 0; m < nm; m++) {
                int big = 0;
                for (int r = 1; r < 16; r++) if (bucket[r].size() > bucket[big].size()) big = r;
                if (!bucket[big].empty()) {
                    out[t * 16 + missing[m]] = (uint32_t)cell[bucket[big].back()] | ((uint32_t)bucket[big].back() << 16);
                    bucket[big].pop_back();
                } else out[t * 16 + missing[m]] = 0xFFFF0000u;  // no square left: the slot idles
            }
        }
    }
}

template <int RTW, int NWAVES, int CH0, int CH, int NB, bool FROM_STATES, bool CB = false>
static hipError_t launch_tower_halo_t(hipStream_t st, const float* in, const TowerParams& T, float* out, int B, int CTW) {
    const int PW = T.halo_pw;
    const size_t plain = CB ? 0 : (size_t)(PW * NB * NB + 1) * (T.cin_pad + LDS_PAD16) * sizeof(float);
    const size_t halo = (size_t)(NB + 2 + PW * T.halo_ps + 1) * (16 * CH + 4) * sizeof(float);  // + the spare cell
    const size_t lds = plain > halo ? plain : halo;
    if (CB && !T.w0_rows) return hipErrorInvalidValue;
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_tower_halo<RTW, NWAVES, CH0, CH, NB, FROM_STATES, CB>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_tower_halo<RTW, NWAVES, CH0, CH, NB, FROM_STATES, CB>), dim3((B + PW - 1) / PW), dim3(NWAVES * 64), lds, st, in, T, out, B, PW, CTW);
    return hipGetLastError();
}

template <int CH0, bool FROM_STATES, bool CB = false>
static hipError_t launch_tower_sq_t(hipStream_t st, const float* in, const TowerParams& T, float* out, int B) {
    constexpr int PW = 16, NB = SQ_NB, CH = 4;
    const size_t plain = (size_t)(PW * NB * NB + 1) * (T.cin_pad + LDS_PAD16) * sizeof(float);
    const size_t image = (size_t)PW * sq_image_pitch4<CH>() * 16;  // 115 200 B
    // CB: layer 0's sums go straight into the square-tile image
    if (CB && !T.w0_rows) return hipErrorInvalidValue;
    const size_t lds = CB ? image : plain > image ? plain : image;
    static LdsAttr lds_attr;
    if (hipError_t e = lds_attr.ensure((const void*)k_tower_sq<CH0, FROM_STATES, CB>, lds); e != hipSuccess) return e;
    hipLaunchKernelGGL((k_tower_sq<CH0, FROM_STATES, CB>), dim3((B + PW - 1) / PW), dim3(512), lds, st, in, T, out, B);
    return hipGetLastError();
}

bool tower_square_tiles(int n, int F, int B) {
    static const bool off = env_on("TG_NO_HALO_TOWER");
    return !off && n == SQ_NB && F == 64 && B > 2048;
}

// full batches of the three BASELINE topologies run on the halo image (identical bits, see k_tower_halo); 5×5 with 64 filters
// on the square-tile image (k_tower_sq)
template <bool FROM_STATES>
static bool launch_tower_halo(hipStream_t st, const float* in, const TowerParams& T, float* out, int B, int n, hipError_t* err) {
    static const bool off = env_on("TG_NO_HALO_TOWER");
    if (off || !T.slotmap) return false;
    if (FROM_STATES && T.cb) {  // layer 0 as a sum of weight rows, constant planes as a bias (no layer-0 loop: CH0 = 0)
        if (tower_square_tiles(n, T.F, B)) { *err = launch_tower_sq_t<0, FROM_STATES, FROM_STATES>(st, in, T, out, B); return true; }
        if (n == 6 && T.F == 128 && B > 512) { *err = launch_tower_halo_t<9, 8, 0, 8, 6, FROM_STATES, FROM_STATES>(st, in, T, out, B, 8); return true; }
        if (n == 5 && T.F == 128 && B > 1024) { *err = launch_tower_halo_t<13, 8, 0, 8, 5, FROM_STATES, FROM_STATES>(st, in, T, out, B, 8); return true; }
        return false;
    }
    if (tower_square_tiles(n, T.F, B) && T.cin_pad == 80) { *err = launch_tower_sq_t<5, FROM_STATES>(st, in, T, out, B); return true; }
    if (n == 6 && T.F == 128 && T.cin_pad == 96 && B > 512) { *err = launch_tower_halo_t<9, 8, 6, 8, 6, FROM_STATES>(st, in, T, out, B, 8); return true; }
    if (n == 5 && T.F == 128 && T.cin_pad == 80 && B > 1024) { *err = launch_tower_halo_t<13, 8, 5, 8, 5, FROM_STATES>(st, in, T, out, B, 8); return true; }
    return false;
}

bool tower_supported(int n, int F, int cin_pad) {
    if (n == 5 && F == 64 && cin_pad == 80) return true;   // config C2
    if (n == 6 && F == 128 && cin_pad == 96) return true;  // config C3
    if (n == 5 && F == 128 && cin_pad == 80) return true;  // config C5 network
    return false;
}

// Does workgroup id i of a 1-D grid run on XCD i mod 8 on this device (every XCD its own L2)?  64 workgroups report HW_REG_XCC_ID.
__global__ void k_xcc_probe(unsigned* __restrict__ out) {
    unsigned x;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
    if (threadIdx.x == 0) out[blockIdx.x] = x & 15u;
}
static bool workgroups_round_robin_over_xcds() {
    static std::mutex guard;
    static int verdict[16] = {};  // per device: 0 unknown, 1 yes, 2 no
    std::lock_guard<std::mutex> lock(guard);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return false;
    if (verdict[dev]) return verdict[dev] == 1;
    verdict[dev] = 2;
    unsigned* d = nullptr;
    unsigned h[64];
    if (hipMalloc((void**)&d, sizeof(h)) != hipSuccess) return false;
    bool ok = true;
    for (int rep = 0; rep < 4 && ok; rep++) {  // (a fresh launch every time: the mapping must not depend on what ran before)
        hipLaunchKernelGGL(k_xcc_probe, dim3(64), dim3(64), 0, nullptr, d);
        ok = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
        for (int i = 8; i < 64 && ok; i++) ok = h[i] == h[i & 7];
    }
    (void)hipFree(d);
    if (ok) verdict[dev] = 1;
    return ok;
}

template <int NRT, int CTW, int CH>
static hipError_t launch_tower_split_t(hipStream_t st, const uint8_t* states, const TowerParams& T, float* out, float* scratch, int B, int n) {
    const int nsq = n * n, F = 16 * CH;
    const size_t lds = (size_t)(nsq + 1) * (F + LDS_PAD16) * sizeof(float);
    constexpr int G = CH / CTW;
    const dim3 grid((B + 7) / 8 * 8 * G), block(NRT * CTW * 64);
    static const bool agent_fences = env_on("TG_SPLIT_AGENT_FENCES");  // A/B: the exchange with agent-scope fences wherever the siblings sit (same bits)
    if (!agent_fences && workgroups_round_robin_over_xcds()) {
        static LdsAttr lds_attr;
        if (hipError_t e = lds_attr.ensure((const void*)k_tower_split<NRT, CTW, CH, true>, lds); e != hipSuccess) return e;
        hipLaunchKernelGGL((k_tower_split<NRT, CTW, CH, true>), grid, block, lds, st, states, T, out, scratch, B, n);
    } else {
        static LdsAttr lds_attr;
        if (hipError_t e = lds_attr.ensure((const void*)k_tower_split<NRT, CTW, CH, false>, lds); e != hipSuccess) return e;
        hipLaunchKernelGGL((k_tower_split<NRT, CTW, CH, false>), grid, block, lds, st, states, T, out, scratch, B, n);
    }
    return hipGetLastError();
}

// small batches of wide networks: a position split over G workgroups by channel tile — G = 8 at 128 filters, G = 4 at 64 on 5×5, the
// only two that exist (k_tower_split; identical bits);
// scratch = TowerParams.split_buf's two exchange buffers
static bool launch_tower_split(hipStream_t st, const uint8_t* states, const TowerParams& T, float* out, float* scratch, int B, int n,
                               hipError_t* err) {
    static const bool off = env_on("TG_NO_SPLIT_TOWER");
    if (off || !scratch || !T.cb || !T.w0_rows || !T.split_flags || B > TOWER_SPLIT_MAX_BATCH || (T.nlayers & 1) == 0)
        return false;
    if (n == 5 && T.F == 64) { *err = launch_tower_split_t<2, 1, 4>(st, states, T, out, scratch, B, n); return true; }  // G = 4
    if (T.F != 128) return false;
    // one (row tile, channel tile) pair per wave, G = 8 workgroups per position: 3-wave workgroups (6×6) fit twice on a CU at their
    // 200 registers, 2-wave ones (5×5) four times — 512 / 1024 resident workgroups.  (2 and 4 channel tiles per workgroup — G = 4, 2 —
    // were measured for the batches in between: a 12-wave workgroup per position pair gains nothing over k_tower.)
    if (n == 6 && B <= TOWER_SPLIT_MAX_BATCH / 2) { *err = launch_tower_split_t<3, 1, 8>(st, states, T, out, scratch, B, n); return true; }
    if (n == 5) { *err = launch_tower_split_t<2, 1, 8>(st, states, T, out, scratch, B, n); return true; }
    return false;
}

// The fused tower: full batches on the halo / square-tile image, small batches of wide networks split by channel tile (states entry
// with a scratch buffer), everything else on k_tower with the whole-position tilings.  FROM_STATES: `in` holds packed game states,
// encoded in-kernel; with T.cb layer 0 is the sum of the set board planes' weight rows (identical bits for every batch size).
template <bool FROM_STATES>
static hipError_t launch_tower_impl(hipStream_t st, const float* in, const TowerParams& T, float* out, int B, int n, float* scratch) {
    hipError_t herr;
    if (launch_tower_halo<FROM_STATES>(st, in, T, out, B, n, &herr)) return herr;
    if (FROM_STATES && launch_tower_split(st, (const uint8_t*)in, T, out, scratch, B, n, &herr)) return herr;
    if (!(FROM_STATES && T.cb) && !tower_supported(n, T.F, T.cin_pad)) return hipErrorInvalidValue;
    return launch_pos_tiled(n, T.F, B, [&](auto t) {
        using Tl = decltype(t);
        constexpr int CH = Tl::F / 16, CH0 = Tl::N == 5 ? 5 : 6;  // layer 0 over the 80 / 96 channels of the input planes
        if constexpr (FROM_STATES)
            if (T.cb) return launch_tower_t<Tl::RTW, Tl::NWAVES, 0, CH, true, true, Tl::N>(st, in, T, out, B, n, Tl::PW, Tl::CTW);
        return launch_tower_t<Tl::RTW, Tl::NWAVES, CH0, CH, FROM_STATES>(st, in, T, out, B, n, Tl::PW, Tl::CTW);
    });
}

hipError_t launch_tower(hipStream_t st, const float* in, const TowerParams& T, float* out, int B, int n) {
    return launch_tower_impl<false>(st, in, T, out, B, n, nullptr);
}

// same, with the input planes encoded in-kernel from packed game states.  scratch (optional): a second activation buffer of the
// batch's size — with it small batches of wide networks run split by channel tile (k_tower_split)
hipError_t launch_tower_states(hipStream_t st, const uint8_t* states, const TowerParams& T, float* out, int B, int n, float* scratch) {
    return launch_tower_impl<true>(st, (const float*)states, T, out, B, n, scratch);
}

}  // namespace tg
