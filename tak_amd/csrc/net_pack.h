// net_pack.h — every weight layout of the engine as a plain host function: tensor lookup, BatchNorm folding, the f32 and
// split-bf16 layouts of the convolutions, of the policy FC and of the value head.  Nothing from HIP: net.hip uploads what
// these return, train.hip shares the padding rules, tests/net_pack_host.cpp runs them on the CPU.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace tg {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// Outputs of the f32 policy FC, padded: to 1664 columns at P = 1575 (the FC kernels use the first 99 tiles = 1584 of them,
// softmax.cuh; the generic k_gemm and k_fc_small want multiples of 64 / 32); shapes with K % 64 != 0 go through k_gemm
inline int fc_padded_cols(size_t K, int P) { return (K % 64 == 0) ? round_up(P, 208) : round_up(P, 64); }

using TensorMap = std::map<std::string, std::vector<float>>;  // as given (tch layouts)

struct Folded {
    std::vector<float> w, b;  // OIHW weights scaled per output channel, bias
};

inline const std::vector<float>* find(const TensorMap& t, const std::string& name, size_t want, std::string& err) {
    auto it = t.find(name);
    if (it == t.end()) { err = "missing tensor " + name; return nullptr; }
    if (it->second.size() != want) {
        err = "tensor " + name + " has " + std::to_string(it->second.size()) + " elements, expected " + std::to_string(want);
        return nullptr;
    }
    return &it->second;
}

// conv (O,I,3,3)+bias followed by BatchNorm in eval mode (running stats, eps = 1e-5, tch default):
// y = (conv(x) + b - mean) * gamma / sqrt(var + eps) + beta  →  w' = w*s, b' = (b - mean)*s + beta
inline bool fold_conv_bn(const TensorMap& t, const std::string& conv, const std::string& bn, int O, int I, Folded& out, std::string& err) {
    auto w = find(t, conv + ".weight", (size_t)O * I * 9, err);
    auto b = w ? find(t, conv + ".bias", O, err) : nullptr;
    if (!w || !b) return false;
    out.w = *w;
    out.b = *b;
    if (bn.empty()) return true;
    auto g = find(t, bn + ".weight", O, err);
    auto be = g ? find(t, bn + ".bias", O, err) : nullptr;
    auto mu = be ? find(t, bn + ".running_mean", O, err) : nullptr;
    auto var = mu ? find(t, bn + ".running_var", O, err) : nullptr;
    if (!var) return false;
    for (int o = 0; o < O; o++) {
        float s = (*g)[o] / std::sqrt((*var)[o] + 1e-5f);
        for (int k = 0; k < I * 9; k++) out.w[(size_t)o * I * 9 + k] *= s;
        out.b[o] = ((*b)[o] - (*mu)[o]) * s + (*be)[o];
    }
    return true;
}

inline uint16_t f32_to_bf16(float x) {  // round to nearest even, as v_cvt_pk_bf16_f32
    uint32_t u;
    std::memcpy(&u, &x, 4);
    if ((u & 0x7f800000u) == 0x7f800000u) return (uint16_t)(u >> 16);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}
inline void split_bf16(float v, uint16_t& hi, uint16_t& lo) {  // v ≈ hi + lo
    hi = f32_to_bf16(v);
    lo = f32_to_bf16(v - bf16_to_f32(hi));
}

// OIHW → Wp[(tap*Ipad + c)/16][CoutP][(tap*Ipad + c)%16], tap = ky*3 + kx, zero padded; bias[CoutP], CoutP = round_up(O, 64)
// last_t = 2 / 3: the real channels of the last 16-channel chunk go to positions 4·(i / last_t) + i % last_t
// (conv_mainloop.cuh conv_last_chunk_perm: layer 0 of the fused towers); 4 = channel order
inline void pack_conv(const Folded& f, int O, int I, int Ipad, int last_t, std::vector<float>& wp, std::vector<float>& bp) {
    const int OP = round_up(O, 64);
    wp.assign((size_t)9 * Ipad * OP, 0.0f);
    bp.assign(OP, 0.0f);
    for (int o = 0; o < O; o++) {
        bp[o] = f.b[o];
        for (int c = 0; c < I; c++)
            for (int tap = 0; tap < 9; tap++) {
                int pos = c & 15;
                if (last_t < 4 && c >= Ipad - 16) { const int i = c - (Ipad - 16); pos = 4 * (i / last_t) + i % last_t; }
                size_t k = (size_t)tap * Ipad + (c & ~15) + pos;
                wp[((k >> 4) * OP + o) * 16 + (k & 15)] = f.w[((size_t)o * I + c) * 9 + tap];
            }
    }
}

// OIHW (BN folded) → [chunk = tap·KC + kc][cout tile][hi|lo][q][cout][8 bf16], channel = 32·kc + 8q + j, zero padded
// OP: output channels of the fragment layout (multiple of 16; 0 = O), O of them real — the conv head inside the split tower
inline std::vector<uint16_t> pack_conv_s3(const Folded& f, int O, int I, int KC, int OP = 0) {
    if (!OP) OP = O;
    std::vector<uint16_t> w((size_t)9 * KC * OP * 64, 0);
    for (int tap = 0; tap < 9; tap++)
        for (int kc = 0; kc < KC; kc++)
            for (int o = 0; o < O; o++)
                for (int q = 0; q < 4; q++)
                    for (int j = 0; j < 8; j++) {
                        int c = 32 * kc + 8 * q + j;
                        if (c >= I) continue;
                        // [chunk][tile of 16 couts][hi|lo][q][cout in tile][8 bf16].  A wave computes two tiles = 32 output channels;
                        // the MFMA leaves rows 4q' … 4q' + 3 of a tile in lane group q', so channel 8q' + 4t + i of the 32 goes to
                        // row 4q' + i of tile t: lane group q' then holds channels 8q' … 8q' + 7 — one 16-byte slot of the split image
                        const int o32 = o & 31, tile = (o >> 5) * 2 + ((o32 >> 2) & 1), row = (o32 >> 3) * 4 + (o32 & 3);
                        size_t slot = (((((size_t)tap * KC + kc) * (OP / 16) + tile) * 2) * 4 + q) * 16 + row;
                        split_bf16(f.w[((size_t)o * I + c) * 9 + tap], w[slot * 8 + j], w[(slot + 64) * 8 + j]);
                    }
    return w;
}

// Constant planes as a bias (kernels.h TowerParams.cb; states entry): a folded conv0 (O, I, 3, 3) over its first bc planes, the
// board planes, …
inline Folded restrict_to_board(const Folded& f0, int O, int I, int bc) {
    Folded fb;
    fb.b = f0.b;
    fb.w.resize((size_t)O * bc * 9);
    for (int o = 0; o < O; o++)
        for (int c = 0; c < bc; c++)
            for (int tap = 0; tap < 9; tap++) fb.w[((size_t)o * bc + c) * 9 + tap] = f0.w[((size_t)o * I + c) * 9 + tap];
    return fb;
}
// … and S[constant plane][border class][O]: per plane ≥ bc and border class the sum of its folded weights over the taps that
// stay on the board (tap order, f32)
inline std::vector<float> pack_cplane_sums(const Folded& f0, int O, int I, int bc) {
    const int nconst = I - bc;
    std::vector<float> S((size_t)nconst * 9 * O, 0.0f);
    for (int pl = 0; pl < nconst; pl++)
        for (int cls = 0; cls < 9; cls++) {
            const int cy = cls / 3, cx = cls % 3;  // 0: first row / column, 1: interior, 2: last
            for (int o = 0; o < O; o++) {
                float sum = 0.0f;
                for (int tap = 0; tap < 9; tap++) {
                    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
                    if ((cy == 0 && dy < 0) || (cy == 2 && dy > 0) || (cx == 0 && dx < 0) || (cx == 2 && dx > 0)) continue;
                    sum += f0.w[((size_t)o * I + bc + pl) * 9 + tap];
                }
                S[((size_t)pl * 9 + cls) * O + o] = sum;
            }
        }
    return S;
}

// Layer 0 of the exact states-entry towers as a sum of rows (tower_stage.cuh tower_cb_layer0): R[plane][tap][O] — for the bc
// board planes the folded conv0 weight of (output channel, plane, tap), channels contiguous, the nine taps of a plane side by
// side; then one more block R[bc][tap][O] of −0.0f, the row a square without a stone adds: x + (−0.0f) = x, bit for bit, for
// every x (+0.0f would turn a sum of −0.0f into +0.0f)
inline std::vector<float> pack_board_rows(const Folded& f0, int O, int I, int bc) {
    std::vector<float> R((size_t)(bc + 1) * 9 * O, -0.0f);
    for (int c = 0; c < bc; c++)
        for (int tap = 0; tap < 9; tap++)
            for (int o = 0; o < O; o++) R[((size_t)c * 9 + tap) * O + o] = f0.w[((size_t)o * I + c) * 9 + tap];
    return R;
}

// element k = sq·F + c (the order of the activations) of a row of Linear [*, F·nsq] over the NCHW flattening c·nsq + sq
// (net5.rs:86 view)
inline float nhwc_at(const float* row, int F, int nsq, size_t k) { return row[(k % F) * nsq + k / F]; }

// The columns of the policy FC: P rows of policy.weight [P, F·nsq], and — where the padding leaves room (`wv` set) — the value
// head (Linear(F·nsq → 1), net5.rs:62) as column P, so the value costs no kernel of its own: the softmax kernel applies the
// tanh.  Every FC layout below is a loop over at(column, k).
struct FcColumns {
    const float* w;   // policy.weight
    const float* b;   // policy.bias
    const float* wv;  // value.weight, or nullptr: no value column
    float bv;         // value.bias
    int P, F, nsq;
    size_t K() const { return (size_t)F * nsq; }
    int cols() const { return P + (wv ? 1 : 0); }
    float at(int o, size_t k) const { return nhwc_at(o < P ? w + (size_t)o * K() : wv, F, nsq, k); }
    std::vector<float> bias(int NP) const {  // padded to NP
        std::vector<float> bp(NP, 0.0f);
        for (int o = 0; o < cols(); o++) bp[o] = o < P ? b[o] : bv;
        return bp;
    }
};

// f32: Wp[K/16][NP][16], zero padded (whole chunks of 16 k)
inline std::vector<float> pack_fc(const FcColumns& c, int NP) {
    const size_t K = c.K();
    std::vector<float> wp((K + 15) / 16 * 16 * NP, 0.0f);
    for (int o = 0; o < c.cols(); o++)
        for (size_t k = 0; k < K; k++) wp[((k >> 4) * NP + o) * 16 + (k & 15)] = c.at(o, k);
    return wp;
}
// the same, every (chunk, tile) block of 16 columns in the MFMA fragment's lane order (k_fc_ring's LDS-DMA source):
// block (chunk, tile): slot q·16 + r holds the 4 floats (k = 16·chunk + 4q … 4q + 3) of column 16·tile + r
inline std::vector<float> pack_fc_lanes(const std::vector<float>& wp, int NP) {
    std::vector<float> wl(wp.size());
    const size_t tiles = (size_t)NP / 16, chunks = wp.size() / ((size_t)NP * 16);
    for (size_t c = 0; c < chunks; c++)
        for (size_t t = 0; t < tiles; t++)
            for (size_t r = 0; r < 16; r++)
                for (size_t qq = 0; qq < 4; qq++)
                    for (size_t u = 0; u < 4; u++)
                        wl[((c * tiles + t) * 64 + qq * 16 + r) * 4 + u] = wp[((c * NP + t * 16 + r) * 4 + qq) * 4 + u];
    return wl;
}
// split bf16: [chunk of 32 k][NP / CB column blocks][q][hi|lo][column][8 bf16], the LDS plane layout of k_fc_s3b
inline std::vector<uint16_t> pack_fc_s3(const FcColumns& c, int NP, int CB) {
    const size_t K = c.K();
    std::vector<uint16_t> ws((size_t)(K / 32) * NP * 64, 0);
    for (int o = 0; o < c.cols(); o++)
        for (size_t k = 0; k < K; k++) {
            const size_t cb = (size_t)o / CB, col = (size_t)o % CB, q = (k & 31) >> 3;
            size_t slot = ((((k >> 5) * (size_t)(NP / CB) + cb) * 4 + q) * 2) * CB + col;
            split_bf16(c.at(o, k), ws[slot * 8 + (k & 7)], ws[(slot + CB) * 8 + (k & 7)]);
        }
    return ws;
}
// the ring kernel's copy (k_fc_s3_ring): [chunk][tile 0 … tiles − 1][hi|lo][lane = q·16 + column within the tile][8 bf16]: a
// (chunk, tile, half) block is one KB in the reader's lane order = one LDS-DMA instruction
inline std::vector<uint16_t> pack_fc_s3_ring(const FcColumns& c, int tiles) {
    const size_t K = c.K();
    std::vector<uint16_t> wr((size_t)(K / 32) * tiles * 2 * 64 * 8, 0);
    for (int o = 0; o < c.cols(); o++)
        for (size_t k = 0; k < K; k++) {
            const size_t lane = ((k & 31) >> 3) * 16 + (o & 15);
            const size_t slot = (((k >> 5) * tiles + (o >> 4)) * 2) * 64 + lane;
            split_bf16(c.at(o, k), wr[slot * 8 + (k & 7)], wr[(slot + 64) * 8 + (k & 7)]);
        }
    return wr;
}

// value.weight [1, F·nsq] in NHWC order (k_value_head)
inline std::vector<float> pack_value(const float* wv, int F, int nsq) {
    std::vector<float> v((size_t)F * nsq);
    for (size_t k = 0; k < v.size(); k++) v[k] = nhwc_at(wv, F, nsq, k);
    return v;
}

}  // namespace tg
