// net.hip — host side of the network: tensor intake in tch/libtorch layout, upload of the folded and
// re-laid-out weights (the packers are net_pack.h), the head plan, and the forward schedule (one kernel per conv layer, heads,
// softmax) on the engine stream.  Replaces Network<N> of reference alpha-tak/src/model/network.rs:26-35
// and the concrete Net5 / Net6 (model/net5.rs, net6.rs, res_block.rs) without any tch type.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "engine.h"
#include "kernels.h"
#include "net_pack.h"
#include "softmax.cuh"
#include "rng.cuh"

namespace tg {

struct ConvLayer {
    DevBuf w, b;      // Wp [K/16][CoutP][16], bias [CoutP]
    int cin_pad = 0;  // channels per input row (multiple of 16)
    int cout = 0, cout_pad = 0;
};

// What the head of a forward does for this (topology, precision): decided once, at the end of net_finalize
enum HeadKind { HEAD_CONV_F32, HEAD_FC_F32, HEAD_FC_SPLIT };
struct HeadPlan {
    HeadKind kind = HEAD_CONV_F32;  // conv head / exact-f32 FC (k_fc_ring, k_fc_small, k_gemm) / split-bf16 FC (k_fc_s3b, k_fc_s3_ring)
    bool conv_in_tower = false;     // the conv head is computed inside the split tower (TowerS3Params.head_*)
    bool split_act = false;         // the split tower writes split activations (its FC or conv head is in use): the value head reads them so
    bool frag_act = false;          // the exact tower writes the FC's fragment order (TowerParams.frag_out)
    int ld = 0;                     // logits row stride: the FC's padded outputs, nsq · CoutP of the conv head
    bool value_col = false;         // the value head rides in padding column P of the policy FC (logit P = value pre-activation)
    bool search_logits = false;     // logits-only forwards are offered to the search (net_fc_logits); not on split tower + f32 FC
    bool stats = false;             // the FC emits block-wise softmax statistics (softmax.cuh) into Net.fc_stats
    int stat_blocks = 0;            // FC_STAT_BLOCKS (11) with stats, else 0
    int stat_stride = 0;            // pairs per row of fc_stats: the blocks, then {value pre-activation, 0}
    const void* w = nullptr;        // FC weights: Wp [K/16][ld][16] f32 / k_fc_s3b's split layout
    const float* b = nullptr;       // FC bias padded to ld
    const void* w_ring = nullptr;   // the ring kernels' copy (k_fc_ring's lane order / k_fc_s3_ring's layout, nullptr: it has none)
};

struct Net {
    TensorMap tensors;  // as given (tch layouts)
    bool ready = false;
    int F = 0, R = 0, cin = 0, cin_pad = 0;
    ConvLayer conv0;
    std::vector<ConvLayer> res1, res2;
    ConvLayer policy_conv;            // TG_HEAD_CONV
    DevBuf policy_w, policy_b;        // TG_HEAD_FC5: Wp [K/16][NP][16]
    DevBuf policy_w_lin;              // the same, every (chunk, tile) block of 16 columns in the MFMA fragment's lane order (k_fc_ring's LDS-DMA source)
    DevBuf value_w;                   // [nsq*F] in NHWC order
    float value_b = 0.0f;
    HeadPlan head;
    // activations (max_batch positions)
    DevBuf x, y, logits, planes_nhwc, planes_nchw;
    DevBuf fc_stats;                  // [max_batch][head.stat_stride][2]: block-wise softmax statistics of the policy FC (softmax.cuh)
    FcGatherArgs gather{};            // set by the search (net_set_gather): logits-only forwards of the exact FC write the
    bool gather_on = false;           // children's logits of every leaf instead of the logits rows
    bool fused = false;  // whole tower in one launch (k_tower)
    TowerParams tower;
    ConvLayer conv0_tower;             // conv0 with the last input chunk permuted (layer 0 of the fused towers)
    DevBuf board_rows;                 // R[board plane, −0.0f block][tap][F]: layer 0 as a sum of rows (TowerParams.cb)
    DevBuf cplane_sums;                // S[constant plane][border class][F] (TowerParams.cb)
    int64_t conv_flops_exec = 0;       // MFMA FLOPs the timed launch actually issues (≤ conv_flops when constant planes are a bias)
    DevBuf halo_map;                   // tile slot → square table of the halo tower (k_tower_halo)
    DevBuf split_ctl;                  // k_tower_split: a counter line per position, then the error word a bounded wait raises (TOWER_SPLIT_CTL_WORDS)
    DevBuf split_buf;                  // k_tower_split: two exchange buffers of TOWER_SPLIT_MAX_BATCH positions × n² × F floats
    DevBuf s3_halo_map;                // the same for the split tower's workgroup (k_tower_s3_halo)
    int precision = TG_PRECISION_F32;  // tg_net_set_precision
    bool s3 = false;                   // split-bf16 tower in use
    TowerS3Params tower_s3;
    std::vector<DevBuf> s3_w;
    DevBuf s3_w0_board;    // conv0 over the board planes only, split fragments with one 32-channel chunk (TowerS3Params.cb)
    DevBuf s3_head;        // conv policy head weights, split (computed inside k_tower_s3)
    DevBuf s3_fc, s3_fc_b; // policy FC weights (split) and bias padded to round_up(P, FC_S3_COLS)
    DevBuf s3_fc_ring;     // the same weights in k_fc_s3_ring's layout [chunk of 32][tile 0 … 98][hi|lo][lane] (full batches)
    // tg_eval_examples: a slice's examples (states, {offset, n_moves, result} records, packed move / visit lists), its rows and
    // target entropies, and the call's sums ({Σ loss_p, Σ loss_z, Σ entropy} f64, {top1, sign_ok, decided} u64)
    DevBuf ev_states, ev_rec, ev_moves, ev_visits, ev_rows, ev_ent, ev_acc;
    // measurement hooks (tg_profile_*)
    int prof_every = 0;
    uint64_t prof_counter = 0;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::vector<hipEvent_t>> ev_chains;  // per sampled forward: [start, after conv0, after each tower conv…, end]
    double conv_ms = 0.0, fwd_ms = 0.0;
    uint64_t conv_n = 0, fwd_n = 0;
    int64_t conv_rows = 0, conv_flops = 0;
    ~Net() {
        for (auto& c : ev_chains) for (auto ev : c) (void)hipEventDestroy(ev);
        for (auto ev : ev_pool) (void)hipEventDestroy(ev);
    }
};

static hipEvent_t prof_event(Net* n, hipStream_t st) {
    hipEvent_t ev = nullptr;
    if (!n->ev_pool.empty()) { ev = n->ev_pool.back(); n->ev_pool.pop_back(); }
    else if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    (void)hipEventRecord(ev, st);
    return ev;
}

static void prof_collect(Net* n) {  // the stream must be idle
    for (auto& c : n->ev_chains) {
        float ms = 0.0f;
        if (c.size() >= 2 && hipEventElapsedTime(&ms, c.front(), c.back()) == hipSuccess) { n->fwd_ms += ms; n->fwd_n++; }
        for (size_t i = 1; i + 2 < c.size(); i++)  // intervals [after conv0 … after last tower conv]
            if (hipEventElapsedTime(&ms, c[i], c[i + 1]) == hipSuccess) { n->conv_ms += ms; n->conv_n++; }
        for (auto ev : c) n->ev_pool.push_back(ev);
    }
    n->ev_chains.clear();
}

void net_destroy(Net* n) { delete n; }

int net_create(TgEngine* e) {
    Net* n = new Net();
    e->net = n;
    n->F = e->cfg.filters;
    n->R = e->cfg.res_blocks;
    n->cin = e->cin;
    n->cin_pad = e->cin_pad;
    return TG_OK;
}

int net_set_tensor(TgEngine* e, const char* name, const float* data, size_t count) {
    if (!e || !e->net) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    if (!name || (!data && count)) return fail(TG_ERR_INVALID_ARG, "tg_net_set_tensor: null argument");
    e->net->tensors[name] = std::vector<float>(data, data + count);
    e->net->ready = false;
    return TG_OK;
}

bool net_ready(const TgEngine* e) { return e && e->net && e->net->ready; }
const TensorMap* net_tensors(const TgEngine* e) { return e && e->net ? &e->net->tensors : nullptr; }

namespace {

template <class T>
hipError_t upload(DevBuf& b, const std::vector<T>& v) {
    hipError_t e = b.ensure(v.size() * sizeof(T));
    return e != hipSuccess ? e : hipMemcpy(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
}

hipError_t upload_conv(const Folded& f, int O, int I, int Ipad, ConvLayer& L, int last_t = 4) {
    std::vector<float> wp, bp;
    pack_conv(f, O, I, Ipad, last_t, wp, bp);
    L.cin_pad = Ipad; L.cout = O; L.cout_pad = (int)bp.size();
    hipError_t e = upload(L.w, wp);
    return e != hipSuccess ? e : upload(L.b, bp);
}

// tile slot → square table of a halo tower's workgroup: pw positions at a stride of ps cells
hipError_t upload_halo_map(int n, int pw, int ps, DevBuf& buf) {
    std::vector<uint32_t> map((size_t)((pw * n * n + 15) / 16) * 16);
    tower_halo_slotmap(n, pw, ps, map.data());
    return upload(buf, map);
}

}  // namespace

int net_finalize(TgEngine* e) {
    if (!e || !e->net) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    TG_HIP(hipSetDevice(e->cfg.device));
    Net* n = e->net;
    const int F = n->F, R = n->R, N = e->g.n, nsq = e->g.nsq, P = e->policy_size;
    const size_t K = (size_t)F * nsq;
    const bool fc_head = e->cfg.policy_head == TG_HEAD_FC5;
    // fold: every (conv, bn) pair once, every tensor looked up in the order a missing one is reported
    std::string err;
    Folded f0, fhead;
    std::vector<Folded> fres(2 * R);  // res i: conv1 + bn1 at 2i, conv2 + bn2 at 2i + 1
    if (!fold_conv_bn(n->tensors, "conv0", "bn0", F, n->cin, f0, err)) return fail(TG_ERR_WEIGHTS, err);
    for (int l = 0; l < 2 * R; l++) {
        const std::string p = "res" + std::to_string(l / 2), k = std::to_string(1 + l % 2);
        if (!fold_conv_bn(n->tensors, p + ".conv" + k, p + ".bn" + k, F, F, fres[l], err)) return fail(TG_ERR_WEIGHTS, err);
    }
    const std::vector<float>*polw = nullptr, *polb = nullptr;
    if (fc_head) {
        polw = find(n->tensors, "policy.weight", (size_t)P * K, err);
        polb = polw ? find(n->tensors, "policy.bias", P, err) : nullptr;
        if (!polb) return fail(TG_ERR_WEIGHTS, err);
    } else if (!fold_conv_bn(n->tensors, "policy", "", P / nsq, F, fhead, err)) return fail(TG_ERR_WEIGHTS, err);
    auto wv = find(n->tensors, "value.weight", K, err);
    auto bv = wv ? find(n->tensors, "value.bias", 1, err) : nullptr;
    if (!bv) return fail(TG_ERR_WEIGHTS, err);
    const bool s3 = n->precision == TG_PRECISION_BF16X3;
    n->s3 = false;
    if (s3 && (!tower_s3_supported(N, F) || 1 + 2 * R > 48 || n->cin > 96))
        return fail(TG_ERR_INVALID_ARG, "TG_PRECISION_BF16X3 supports 5x5 with 64 or 128 filters and 6x6 with 128 filters, with at most "
                                        "48 conv layers (23 residual blocks); this network has " + std::to_string(1 + 2 * R) + " layers");
    // the FC head's geometry: padded outputs on either precision, which FC runs, and whether the padding leaves the value
    // head a column (decided here, once, for every layout below)
    const int np = fc_head ? fc_padded_cols(K, P) : 0, np3 = s3 ? round_up(P, FC_S3_COLS) : 0;
    const bool split_fc = fc_head && s3 && fc_s3_supported((int)K, np3);
    const bool value_col = fc_head && np > P && (!split_fc || np3 > P);
    const FcColumns fc{fc_head ? polw->data() : nullptr, fc_head ? polb->data() : nullptr, value_col ? wv->data() : nullptr, (*bv)[0], P, F, nsq};

    // exact-path weights
    TG_HIP(upload_conv(f0, F, n->cin, n->cin_pad, n->conv0));
    n->res1 = std::vector<ConvLayer>(R); n->res2 = std::vector<ConvLayer>(R);
    for (int i = 0; i < R; i++) {
        TG_HIP(upload_conv(fres[2 * i], F, F, F, n->res1[i]));
        TG_HIP(upload_conv(fres[2 * i + 1], F, F, F, n->res2[i]));
    }
    if (fc_head) {
        const std::vector<float> wp = pack_fc(fc, np);
        TG_HIP(upload(n->policy_w, wp));
        TG_HIP(upload(n->policy_w_lin, pack_fc_lanes(wp, np)));
        TG_HIP(upload(n->policy_b, fc.bias(np)));
    } else TG_HIP(upload_conv(fhead, P / nsq, F, F, n->policy_conv));
    n->value_b = (*bv)[0];
    TG_HIP(upload(n->value_w, pack_value(wv->data(), F, nsq)));

    n->fused = tower_supported(N, F, n->cin_pad) && 1 + 2 * R <= 48;
    if (n->fused) {
        TowerParams& T = n->tower;
        T.nlayers = 1 + 2 * R; T.cin_pad = n->cin_pad; T.F = F;
        // layer 0: 72 of 80 (5×5) / 92 of 96 (6×6) input channels are real; with the last chunk permuted 2 of 20 / 1 of 24
        // MFMAs per tile and tap multiply padding only and are skipped — the towers get their own copy of the weights
        const int tail = n->cin - (n->cin_pad - 16);
        T.cin_last_t = (tail > 0 && tail <= 12) ? (tail + 3) / 4 : 4;
        if (T.cin_last_t < 2) T.cin_last_t = 4;
        TG_HIP(upload_conv(f0, F, n->cin, n->cin_pad, n->conv0_tower, T.cin_last_t));
        T.w[0] = n->conv0_tower.w.as<float>(); T.b[0] = n->conv0.b.as<float>();
        // Constant planes as a bias (kernels.h TowerParams.cb; states entry): the table S, and conv0's weights of the board planes
        // as the rows layer 0 sums
        T.cb = 0; T.cplane_sums = nullptr; T.w0_rows = nullptr;
        const int bc = board_channels(N), nconst = n->cin - bc;
        if (!env_on("TG_NO_CONST_BIAS") && bc > 16 && bc <= 28 && nconst > 0) {
            TG_HIP(upload(n->cplane_sums, pack_cplane_sums(f0, F, n->cin, bc)));
            TG_HIP(upload(n->board_rows, pack_board_rows(f0, F, n->cin, bc)));
            T.cb = 1; T.cplane_sums = n->cplane_sums.as<float>(); T.w0_rows = n->board_rows.as<float>();
        }
        for (int i = 0; i < R; i++) {
            T.w[1 + 2 * i] = n->res1[i].w.as<float>(); T.b[1 + 2 * i] = n->res1[i].b.as<float>();
            T.w[2 + 2 * i] = n->res2[i].w.as<float>(); T.b[2 + 2 * i] = n->res2[i].b.as<float>();
        }
        T.slotmap = nullptr; T.halo_pw = 0; T.halo_ps = 0;
        T.split_flags = nullptr; T.split_err = nullptr;
        if (T.cb && (F == 128 || (F == 64 && N == 5))) {  // small batches split a position over several workgroups (k_tower_split)
            TG_HIP(n->split_ctl.ensure((size_t)TOWER_SPLIT_CTL_WORDS * 4));
            TG_HIP(hipMemset(n->split_ctl.p, 0, (size_t)TOWER_SPLIT_CTL_WORDS * 4));
            TG_HIP(n->split_buf.ensure((size_t)2 * TOWER_SPLIT_MAX_BATCH * nsq * F * 4));
            T.split_flags = n->split_ctl.as<unsigned>();
            T.split_err = n->split_ctl.as<int>() + TOWER_SPLIT_CTL_WORDS - 32;
        }
        // FC-head networks whose value head rides in the FC's padding column: nothing but the policy FC reads the tower's
        // output, so it is written in the FC's fragment order
        T.frag_out = (value_col && fc_frag_supported(nsq * F, np) && !env_on("TG_NO_FRAG_OUT")) ? 1 : 0;
        int pw, ps;
        if (tower_halo_geometry(N, F, &pw, &ps)) {
            TG_HIP(upload_halo_map(N, pw, ps, n->halo_map));
            T.slotmap = n->halo_map.as<uint32_t>(); T.halo_pw = pw; T.halo_ps = ps;
        }
    }
    HeadPlan H;
    if (s3) {
        TowerS3Params& T = n->tower_s3;
        T.nlayers = 1 + 2 * R; T.cin_pad = n->cin_pad; T.F = F;
        n->s3_w = std::vector<DevBuf>(T.nlayers);
        TG_HIP(upload(n->s3_w[0], pack_conv_s3(f0, F, n->cin, 3)));
        T.w[0] = n->s3_w[0].p; T.b[0] = n->conv0.b.as<float>();
        for (int l = 1; l <= 2 * R; l++) {
            TG_HIP(upload(n->s3_w[l], pack_conv_s3(fres[l - 1], F, F, F / 32)));
            T.w[l] = n->s3_w[l].p; T.b[l] = (l % 2 ? n->res1[(l - 1) / 2] : n->res2[(l - 1) / 2]).b.as<float>();
        }
        // constant planes as a bias on the split towers too: the f32 table S of the exact path, conv0 restricted to the board planes
        T.cb = 0; T.w0_board = nullptr; T.cplane_sums = nullptr;
        if (n->fused && n->tower.cb) {
            const int bc = board_channels(N);
            TG_HIP(upload(n->s3_w0_board, pack_conv_s3(restrict_to_board(f0, F, n->cin, bc), F, bc, 1)));
            T.cb = 1; T.w0_board = n->s3_w0_board.p; T.cplane_sums = n->cplane_sums.as<float>();
        }
        T.slotmap = nullptr; T.halo_ps = 0;
        int pw3, ps3;
        if (tower_s3_halo_geometry(N, F, &pw3, &ps3)) {
            TG_HIP(upload_halo_map(N, pw3, ps3, n->s3_halo_map));
            T.slotmap = n->s3_halo_map.as<uint32_t>(); T.halo_ps = ps3;
        }
        T.head_w = nullptr; T.head_b = nullptr; T.head_out = nullptr; T.head_cout = 0;
        if (!fc_head && n->policy_conv.cout_pad % 32 == 0) {
            TG_HIP(upload(n->s3_head, pack_conv_s3(fhead, P / nsq, F, F / 32, n->policy_conv.cout_pad)));
            T.head_w = n->s3_head.p; T.head_b = n->policy_conv.b.as<float>(); T.head_cout = n->policy_conv.cout_pad;
            H.conv_in_tower = true;
        }
        if (split_fc) {
            TG_HIP(upload(n->s3_fc, pack_fc_s3(fc, np3, FC_S3_COLS)));
            if (P + 1 <= FC_TILES * 16 && K % 64 == 0) {
                TG_HIP(upload(n->s3_fc_ring, pack_fc_s3_ring(fc, FC_TILES)));
                H.w_ring = n->s3_fc_ring.p;
            }
            TG_HIP(upload(n->s3_fc_b, fc.bias(np3)));
        }
        n->s3 = true;
    }
    // head plan
    H.kind = !fc_head ? HEAD_CONV_F32 : split_fc ? HEAD_FC_SPLIT : HEAD_FC_F32;
    H.split_act = split_fc || H.conv_in_tower;
    H.frag_act = H.kind == HEAD_FC_F32 && !s3 && n->fused && n->tower.frag_out;
    H.ld = !fc_head ? nsq * n->policy_conv.cout_pad : split_fc ? np3 : np;
    H.value_col = value_col;
    H.search_logits = value_col && P <= 2048 && !(s3 && !split_fc);  // (split tower with the f32 FC: keep the plain path)
    // the FC emits the softmax statistics per column block, nobody re-reads whole rows (one statistics geometry — softmax.cuh — on
    // both precisions: the split-bf16 FC's ring kernel emits it from its epilogue, k_fc_stats computes it behind k_fc_s3b for ≤ 512 rows)
    H.stats = value_col && !env_on("TG_NO_FC_STATS") && P + 1 <= FC_TILES * 16 &&
              (split_fc ? np3 >= FC_TILES * 16 : fc_stats_supported(nsq * F, np, np));
    H.stat_blocks = H.stats ? FC_STAT_BLOCKS : 0;
    H.stat_stride = H.stats ? FC_STAT_STRIDE : 0;
    if (H.kind == HEAD_FC_SPLIT) { H.w = n->s3_fc.p; H.b = n->s3_fc_b.as<float>(); }
    if (H.kind == HEAD_FC_F32) { H.w = n->policy_w.p; H.b = n->policy_b.as<float>(); H.w_ring = n->policy_w_lin.p; }
    n->head = H;
    // activation buffers
    size_t mb = (size_t)e->cfg.max_batch;
    TG_HIP(n->x.ensure(((mb + 15) / 16 * 16) * nsq * F * 4));  // (whole tiles of 16 positions: fragment-major FC input)
    TG_HIP(n->y.ensure(mb * nsq * F * 4));
    TG_HIP(n->logits.ensure(mb * (size_t)std::max(H.ld, np) * 4));
    TG_HIP(n->planes_nhwc.ensure(mb * nsq * n->cin_pad * 4));
    if (H.stats) TG_HIP(n->fc_stats.ensure(mb * (size_t)H.stat_stride * 2 * 4));
    if (int rc = symm_tables_build(e); rc) return rc;  // once per engine: the policy permutation tables of the 8 symmetries
    n->ready = true;
    return TG_OK;
}

static int net_forward_impl(TgEngine* e, int nb, const float* d_planes, const uint8_t* d_states, float* d_policy, float* d_eval);

// planes NHWC [nb][nsq][cin_pad] (device) → policy [nb][P] (softmax, reference order), eval [nb]
int net_forward_dev(TgEngine* e, int nb, const float* d_planes, float* d_policy, float* d_eval) {
    return net_forward_impl(e, nb, d_planes, nullptr, d_policy, d_eval);
}

bool net_takes_states(const TgEngine* e) { return net_ready(e) && (e->net->fused || e->net->s3); }

// FC head with the value column: the logits buffer ([max_batch][*ld], logit P = value pre-activation) the search reads when it
// passes d_policy = nullptr to the forward (no softmax kernel, no probabilities in HBM); nullptr for every other topology
const float* net_fc_logits(const TgEngine* e, int* ld) {
    if (!net_ready(e) || !e->net->head.search_logits) return nullptr;
    *ld = e->net->head.ld;  // the row stride the FC kernel in use writes
    return e->net->logits.as<float>();
}

// the block statistics that go with net_fc_logits' buffer ([max_batch][*blocks][2]), or nullptr: the consumer then takes max and
// Σexp over the whole row itself (softmax_stats_wave)
const float* net_fc_stats(const TgEngine* e, int* blocks, int* stride) {
    if (!net_ready(e) || !e->net->head.stats || !e->net->head.search_logits) return nullptr;  // (as net_fc_logits declines)
    *blocks = e->net->head.stat_blocks;
    *stride = e->net->head.stat_stride;
    return e->net->fc_stats.as<float>();
}

// Search iterations on the exact-f32 FC head need, of the FC's output, only the logits of every leaf's children: with a gather
// target set (and a batch the ring kernel serves), a logits-only forward (d_policy = nullptr) of `leaves` rows writes
// child_logit[row][child] and the statistics record (with the value pre-activation) — no logits rows.  net_gather_ok tells
// the search whether the next such forward will do so (then its backup reads child_logit, else the logits buffer).
bool net_gather_ok(const TgEngine* e, int leaves) {
    if (!net_ready(e)) return false;
    const HeadPlan& H = e->net->head;
    static const bool off = env_on("TG_NO_FC_GATHER");  // A/B: logits rows + the backup's own gather (same bits)
    if (off || !H.stats || !H.search_logits) return false;
    if (H.kind == HEAD_FC_SPLIT) return H.w_ring && !env_on("TG_S3_NO_FC_RING") && fc_s3_ring_supported(leaves, e->g.nsq * e->net->F, e->policy_size + 1);
    return fc_gather_supported(leaves, e->g.nsq * e->net->F, H.ld);
}
void net_set_gather(TgEngine* e, const FcGatherArgs* g) {
    if (!e || !e->net) return;
    e->net->gather_on = g != nullptr;
    if (g) e->net->gather = *g;
}

int net_forward_states_dev(TgEngine* e, int nb, const uint8_t* d_states, float* d_policy, float* d_eval) {
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    if (nb <= 0) return TG_OK;
    if (e->net->fused || e->net->s3) return net_forward_impl(e, nb, nullptr, d_states, d_policy, d_eval);
    launch_encode_nhwc(e->stream, d_states, nb, e->g.n, e->net->planes_nhwc.as<float>(), e->net->cin_pad);
    TG_HIP(hipGetLastError());
    return net_forward_impl(e, nb, e->net->planes_nhwc.as<float>(), nullptr, d_policy, d_eval);
}

// every launch on the engine stream, the batch in the first nb position slots of the activation buffers
static int net_forward_impl(TgEngine* e, int nb, const float* d_planes, const uint8_t* d_states, float* d_policy, float* d_eval) {
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    if (nb <= 0) return TG_OK;
    if (nb > e->cfg.max_batch) return fail(TG_ERR_INVALID_ARG, "batch larger than max_batch");
    Net* n = e->net;
    const HeadPlan& H = n->head;
    hipStream_t st = e->stream;
    const int F = n->F, nsq = e->g.nsq, N = e->g.n;
    const int M = nb * nsq;
    float* x = n->x.as<float>();
    float* y = n->y.as<float>();
    std::vector<hipEvent_t>* chain = nullptr;
    if (n->prof_every > 0 && (n->prof_counter++ % (uint64_t)n->prof_every) == 0) {
        if (n->ev_chains.size() >= 256) {  // bound the number of pending events
            TG_HIP(hipStreamSynchronize(st));
            prof_collect(n);
        }
        n->ev_chains.emplace_back();
        chain = &n->ev_chains.back();
        n->conv_rows = M;
        // algorithmic FLOPs of one timed launch: one F→F conv (per-layer path) or the whole tower (fused)
        n->conv_flops = (n->fused || n->s3) ? 2ll * M * 9 * ((long long)n->cin * F + 2ll * n->R * F * F) : 2ll * M * 9 * F * F;
        // executed: with the constant planes as a bias layer 0 issues no MFMA (it is a sum of weight rows on the vector pipe); the
        // square-tile tower issues the MFMAs of on-board (square, tap) pairs only (169 of 225 on 5×5) in the F → F layers
        if (n->fused && !n->s3) {
            const bool cb0 = d_states && n->tower.cb;
            const long long taps = tower_square_tiles(N, F, nb) ? (long long)nb * 169 : 9ll * M;  // (row, tap) pairs of a layer ≥ 1
            n->conv_flops_exec = (cb0 ? 0ll : 2ll * 9 * M * n->cin * F) + 2ll * taps * 2ll * n->R * F * F;
        } else n->conv_flops_exec = n->conv_flops;
        chain->push_back(prof_event(n, st));
    }
    if (n->s3) {
        if (chain) chain->push_back(prof_event(n, st));
        TowerS3Params T3 = n->tower_s3;
        if (H.conv_in_tower) T3.head_out = n->logits.as<float>();
        if (d_states) TG_HIP(launch_tower_s3_states(st, d_states, T3, x, nb, N, H.split_act));
        else TG_HIP(launch_tower_s3(st, d_planes, T3, x, nb, N, H.split_act));
        if (chain) chain->push_back(prof_event(n, st));
    } else if (n->fused) {
        if (chain) chain->push_back(prof_event(n, st));
        // (small batches of wide networks run split by channel tile through the exchange buffers)
        if (d_states) TG_HIP(launch_tower_states(st, d_states, n->tower, x, nb, N, n->split_buf.as<float>()));
        else TG_HIP(launch_tower(st, d_planes, n->tower, x, nb, N));
        if (chain) chain->push_back(prof_event(n, st));
    } else {
        TG_HIP(launch_conv3x3(st, d_planes, n->conv0.w.as<float>(), n->conv0.b.as<float>(), nullptr, x, M, N, n->cin_pad,
                              n->conv0.cout_pad, F, F, true));
        if (chain) chain->push_back(prof_event(n, st));
        for (int i = 0; i < n->R; i++) {
            TG_HIP(launch_conv3x3(st, x, n->res1[i].w.as<float>(), n->res1[i].b.as<float>(), nullptr, y, M, N, F,
                                  n->res1[i].cout_pad, F, F, true));
            if (chain) chain->push_back(prof_event(n, st));
            TG_HIP(launch_conv3x3(st, y, n->res2[i].w.as<float>(), n->res2[i].b.as<float>(), x, x, M, N, F,
                                  n->res2[i].cout_pad, F, F, true));
            if (chain) chain->push_back(prof_event(n, st));
        }
    }
    float* logits = n->logits.as<float>();
    const int P = e->policy_size;
    bool value_done = false;
    if (H.kind == HEAD_CONV_F32) {
        const ConvLayer& L = n->policy_conv;
        if (!H.conv_in_tower)
            TG_HIP(launch_conv3x3(st, x, L.w.as<float>(), L.b.as<float>(), nullptr, logits, M, N, F, L.cout_pad, L.cout_pad, L.cout, false));
        // (exact-f32 path: the softmax's launch computes the value head too — one launch less per forward)
        const ValueHeadArgs vh{x, n->value_w.as<float>(), n->value_b, nsq * F, d_eval};
        TG_HIP(launch_softmax(st, logits, H.ld, true, nsq, L.cout_pad, P, nb, d_policy, nullptr, H.split_act ? nullptr : &vh, &value_done));
    } else {
        float* stats = H.stats ? n->fc_stats.as<float>() : nullptr;
        const FcGatherArgs* gather = !d_policy && n->gather_on && net_gather_ok(e, nb) ? &n->gather : nullptr;
        const int cols = P + (H.value_col ? 1 : 0);
        if (H.kind == HEAD_FC_SPLIT) TG_HIP(launch_fc_s3(st, x, H.w, H.w_ring, H.b, logits, nb, nsq * F, H.ld, H.ld, cols, stats, P, gather));
        else {
            static const bool lin_src = !env_on("TG_FC_PERMUTED_SRC");  // A/B: the ring's LDS-DMA reads the [chunk][column][q] layout (same bits)
            TG_HIP(launch_gemm(st, x, nsq * F, (const float*)H.w, H.b, logits, nb, nsq * F, H.ld, H.ld, cols, H.frag_act, stats, P, gather,
                               lin_src ? (const float*)H.w_ring : nullptr));
        }
        if (d_policy && stats) TG_HIP(launch_softmax_stats(st, logits, H.ld, stats, H.stat_blocks, H.stat_stride, P, nb, d_policy, d_eval));
        else if (d_policy) TG_HIP(launch_softmax(st, logits, H.ld, false, nsq, 0, P, nb, d_policy, H.value_col ? d_eval : nullptr));
    }
    if (!d_policy && !H.value_col) return fail(TG_ERR_STATE, "logits-only forward needs the FC head with the value column");
    if (H.value_col) {
        // eval = tanh(logit P), written by the softmax kernel (or taken by the tree backup straight from the logits)
    } else if (H.split_act) TG_HIP(launch_value_head_s3(st, x, n->value_w.as<float>(), n->value_b, nb, nsq * F, d_eval));
    else if (!value_done) TG_HIP(launch_value_head(st, x, n->value_w.as<float>(), n->value_b, nb, nsq * F, d_eval));
    if (chain) chain->push_back(prof_event(n, st));
    return TG_OK;
}

// after a stream sync: has a bounded wait of k_tower_split given up?  (never seen; it would mean a sibling workgroup of a position
// was not running — the counters are reset so that the next launch starts clean)
int net_poll_errors(TgEngine* e) {
    if (!e || !e->net || !e->net->split_ctl.p) return TG_OK;
    int err = 0;
    TG_HIP(hipMemcpy(&err, e->net->split_ctl.as<int>() + TOWER_SPLIT_CTL_WORDS - 32, 4, hipMemcpyDeviceToHost));
    if (!err) return TG_OK;
    TG_HIP(hipMemset(e->net->split_ctl.p, 0, (size_t)TOWER_SPLIT_CTL_WORDS * 4));
    return fail(TG_ERR_HIP, err == 2 ? "k_tower_split: the workgroups of one position ran on different XCDs (the same-L2 exchange is not safe on this "
                                       "device: set TG_SPLIT_AGENT_FENCES=1 or TG_NO_SPLIT_TOWER=1); the forward's results are invalid"
                                     : "k_tower_split: a workgroup waited for its position's siblings beyond the bound; the forward's results are invalid");
}

int net_profile_enable(TgEngine* e, int sample_every) {
    if (!e || !e->net) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    if (sample_every < 0) return fail(TG_ERR_INVALID_ARG, "sample_every must be >= 0");
    e->net->prof_every = sample_every;
    e->net->prof_counter = 0;
    return TG_OK;
}

int net_profile_read(TgEngine* e, TgProfile* out) {
    if (!e || !e->net || !out) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    Net* n = e->net;
    TG_HIP(hipSetDevice(e->cfg.device));
    TG_HIP(hipStreamSynchronize(e->stream));
    prof_collect(n);
    out->conv_launches = n->conv_n; out->conv_ms = n->conv_ms; out->forwards = n->fwd_n; out->forward_ms = n->fwd_ms;
    out->conv_rows = n->conv_rows; out->conv_flops = n->conv_flops; out->conv_flops_executed = n->conv_flops_exec;
    n->conv_n = n->fwd_n = 0;
    n->conv_ms = n->fwd_ms = 0.0;
    return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_net_set_tensor(TgEngine* e, const char* name, const float* data, size_t count) { return net_set_tensor(e, name, data, count); }
int tg_net_finalize(TgEngine* e) { return net_finalize(e); }

// Network::default() (net5.rs:29-73 / net6.rs:29-69): every layer with tch's default initialisers — conv2d: weight
// KaimingUniform = U(±1/sqrt(fan_in)), bias 0; batch_norm2d: weight U(0,1), bias 0, running mean 0 / var 1; linear: weight
// KaimingUniform, bias U(±1/sqrt(in)).  (tch 0.7 is not vendored in the reference: these are its documented defaults; only the
// distribution matters.)  Draws come from Philox(seed; tensor index, element index).
int tg_net_init_random(TgEngine* e, uint64_t seed) {
    if (!e || !e->net) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    Net* n = e->net;
    const int F = e->cfg.filters, R = e->cfg.res_blocks, nsq = e->g.nsq;
    uint32_t tensor_id = 0;
    auto uniform = [&](const std::string& name, size_t count, float lo, float hi) {
        std::vector<float> v(count);
        for (size_t i = 0; i < count; i += 4) {
            U4 r = philox4x32_10(seed, tensor_id, (uint32_t)(i >> 2), (uint32_t)((uint64_t)i >> 34), 0x696e6974u);
            for (size_t k = 0; k < 4 && i + k < count; k++) v[i + k] = lo + (hi - lo) * ((float)(r.v[k] >> 8) * (1.0f / 16777216.0f));
        }
        n->tensors[name] = std::move(v);
        tensor_id++;
    };
    auto constant = [&](const std::string& name, size_t count, float c) { n->tensors[name] = std::vector<float>(count, c); };
    auto conv = [&](const std::string& name, int O, int I) {
        float b = 1.0f / std::sqrt((float)(I * 9));
        uniform(name + ".weight", (size_t)O * I * 9, -b, b);
        constant(name + ".bias", O, 0.0f);
    };
    auto bn = [&](const std::string& name) {
        uniform(name + ".weight", F, 0.0f, 1.0f);
        constant(name + ".bias", F, 0.0f);
        constant(name + ".running_mean", F, 0.0f);
        constant(name + ".running_var", F, 1.0f);
    };
    auto linear = [&](const std::string& name, int out, int in) {
        float b = 1.0f / std::sqrt((float)in);
        uniform(name + ".weight", (size_t)out * in, -b, b);
        uniform(name + ".bias", out, -b, b);
    };
    conv("conv0", F, e->cin);
    bn("bn0");
    for (int i = 0; i < R; i++) {
        std::string r = "res" + std::to_string(i);
        conv(r + ".conv1", F, F);
        conv(r + ".conv2", F, F);
        bn(r + ".bn1");
        bn(r + ".bn2");
    }
    if (e->cfg.policy_head == TG_HEAD_FC5) linear("policy", e->policy_size, F * nsq);
    else conv("policy", e->policy_size / nsq, F);
    linear("value", 1, F * nsq);
    n->ready = false;
    return TG_OK;
}

// the tensor as last given to tg_net_set_tensor / tg_net_init_random / tg_train_commit (Network::save reads these)
int tg_net_get_tensor(TgEngine* e, const char* name, float* out, size_t count) {
    if (!e || !e->net) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    if (!name || !out) return fail(TG_ERR_INVALID_ARG, "tg_net_get_tensor: null argument");
    auto it = e->net->tensors.find(name);
    if (it == e->net->tensors.end()) return fail(TG_ERR_INVALID_ARG, (std::string("tg_net_get_tensor: no tensor ") + name).c_str());
    if (it->second.size() != count) return fail(TG_ERR_INVALID_ARG, (std::string("tg_net_get_tensor: ") + name + " has " + std::to_string(it->second.size()) + " elements").c_str());
    std::memcpy(out, it->second.data(), count * sizeof(float));
    return TG_OK;
}
int tg_net_set_precision(TgEngine* e, int precision) {
    if (!e || !e->net) return fail(TG_ERR_STATE, "engine has no network (evaluator is not TG_EVAL_RESNET)");
    if (precision != TG_PRECISION_F32 && precision != TG_PRECISION_BF16X3) return fail(TG_ERR_INVALID_ARG, "unknown precision");
    e->net->precision = precision;
    e->net->ready = false;  // takes effect at the next tg_net_finalize
    return TG_OK;
}
int tg_profile_enable(TgEngine* e, int sample_every) { return net_profile_enable(e, sample_every); }
int tg_profile_read(TgEngine* e, TgProfile* out) { return net_profile_read(e, out); }

// Network::policy_eval (net5.rs:120-130): encode on the device straight into NHWC, forward, copy out
int tg_policy_eval_dev(TgEngine* e, int n, const void* d_states, float* d_policy, float* d_eval) {
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    if (n < 0 || n > e->cfg.max_batch) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_dev: n out of range");
    if (n == 0) return TG_OK;
    // (logits-only forwards — d_policy = nullptr — are the search's private contract with the FC's gather epilogue)
    if (!d_states || !d_policy || !d_eval) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_dev: null argument");
    TG_HIP(hipSetDevice(e->cfg.device));
    return net_forward_states_dev(e, n, (const uint8_t*)d_states, d_policy, d_eval);
}

int tg_policy_eval(TgEngine* e, int n, const void* states, float* policy, float* eval) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "null engine");
    if (n < 0 || (n > 0 && (!states || !policy || !eval))) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval: bad arguments");
    if (n == 0) return TG_OK;  // net5.rs:121-123
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    TG_HIP(hipSetDevice(e->cfg.device));
    const size_t sb = e->g.bytes, P = (size_t)e->policy_size;
    TG_HIP(e->s_policy.ensure((size_t)e->cfg.max_batch * P * 4));
    TG_HIP(e->s_eval.ensure((size_t)e->cfg.max_batch * 4));
    for (int off = 0; off < n; off += e->cfg.max_batch) {
        int k = std::min(e->cfg.max_batch, n - off);
        TG_HIP(hipMemcpyAsync(e->s_states.p, (const uint8_t*)states + (size_t)off * sb, (size_t)k * sb, hipMemcpyHostToDevice, e->stream));
        int rc = tg_policy_eval_dev(e, k, e->s_states.p, e->s_policy.as<float>(), e->s_eval.as<float>());
        if (rc) return rc;
        TG_HIP(hipMemcpyAsync(policy + (size_t)off * P, e->s_policy.p, (size_t)k * P * 4, hipMemcpyDeviceToHost, e->stream));
        TG_HIP(hipMemcpyAsync(eval + off, e->s_eval.p, (size_t)k * 4, hipMemcpyDeviceToHost, e->stream));
        TG_HIP(hipStreamSynchronize(e->stream));
        rc = net_poll_errors(e);
        if (rc) return rc;
    }
    return TG_OK;
}

// Network::forward_mcts (net5.rs:106-111) on caller-encoded NCHW planes
int tg_forward_mcts(TgEngine* e, int n, const float* planes, float* policy, float* eval) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "null engine");
    if (n < 0 || (n > 0 && (!planes || !policy || !eval))) return fail(TG_ERR_INVALID_ARG, "tg_forward_mcts: bad arguments");
    if (n == 0) return TG_OK;
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    TG_HIP(hipSetDevice(e->cfg.device));
    Net* net = e->net;
    const size_t per = (size_t)e->cin * e->g.nsq, P = (size_t)e->policy_size;
    TG_HIP(net->planes_nchw.ensure((size_t)e->cfg.max_batch * per * 4));
    TG_HIP(e->s_policy.ensure((size_t)e->cfg.max_batch * P * 4));
    TG_HIP(e->s_eval.ensure((size_t)e->cfg.max_batch * 4));
    for (int off = 0; off < n; off += e->cfg.max_batch) {
        int k = std::min(e->cfg.max_batch, n - off);
        TG_HIP(hipMemcpyAsync(net->planes_nchw.p, planes + (size_t)off * per, (size_t)k * per * 4, hipMemcpyHostToDevice, e->stream));
        TG_HIP(launch_nchw_to_nhwc(e->stream, net->planes_nchw.as<float>(), k, e->cin, e->g.nsq, net->cin_pad, net->planes_nhwc.as<float>()));
        int rc = net_forward_dev(e, k, net->planes_nhwc.as<float>(), e->s_policy.as<float>(), e->s_eval.as<float>());
        if (rc) return rc;
        TG_HIP(hipMemcpyAsync(policy + (size_t)off * P, e->s_policy.p, (size_t)k * P * 4, hipMemcpyDeviceToHost, e->stream));
        TG_HIP(hipMemcpyAsync(eval + off, e->s_eval.p, (size_t)k * 4, hipMemcpyDeviceToHost, e->stream));
        TG_HIP(hipStreamSynchronize(e->stream));
    }
    return TG_OK;
}

// Losses of the deployed network on examples (no counterpart in the reference: network.rs:86 prints the losses of the batch it
// has just fitted).  Slices of ≤ max_batch positions: upload the slice's examples with their move lists packed, build the
// dihedral images on the device (symmetries), run the inference forward with FULL logits rows, k_example_metrics, k_eval_sum.
int tg_eval_examples(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves, const uint32_t* visits,
                     const float* results, int symmetries, TgExampleMetrics* sums, float* rows) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "null engine");
    if (e->cfg.evaluator != TG_EVAL_RESNET || !e->net) return fail(TG_ERR_STATE, "tg_eval_examples: the engine's evaluator is not TG_EVAL_RESNET");
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    if (!sums) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: sums is null");
    if (symmetries != 0 && symmetries != 1) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: symmetries must be 0 or 1");
    if (n < 0 || (n > 0 && (!states || !n_moves || !moves || !visits || !results))) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: bad arguments");
    if (n > INT_MAX / 8) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: more than 2^28 examples in one call");
    std::memset(sums, 0, sizeof(*sums));
    if (n == 0) return TG_OK;
    const size_t sb = e->g.bytes;
    const int mb = e->cfg.max_batch, P = e->policy_size, nsq = e->g.nsq;
    const bool symm = symmetries == 1;
    const long total = symm ? 8L * n : n;
    const uint8_t* hs = (const uint8_t*)states;
    auto first_ex = [&](long p) { return symm ? p >> 3 : p; };
    // every example is checked before the first launch (the checks of tg_train_chunk: a reachable state, 1 ≤ n_moves ≤
    // TG_MAX_MOVES, at least one visit; the visit total must also fit the u32 the kernels divide by)
    for (int i = 0; i < n; i++) {
        if (int rc = validate_states(e, 1, hs + (size_t)i * sb, "tg_eval_examples"); rc)
            return fail(rc, "tg_eval_examples: example " + std::to_string(i) + ": " + tg_last_error());
        if (n_moves[i] <= 0 || n_moves[i] > TG_MAX_MOVES) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: example " + std::to_string(i) + ": n_moves out of range");
        uint64_t tv = 0;
        for (int k = 0; k < n_moves[i]; k++) tv += visits[(size_t)i * TG_MAX_MOVES + k];
        if (tv == 0) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: example " + std::to_string(i) + " without visits (the policy target would be 0/0)");
        if (tv > UINT32_MAX) return fail(TG_ERR_INVALID_ARG, "tg_eval_examples: example " + std::to_string(i) + ": the visits add up to more than 2^32 - 1");
    }
    size_t max_entries = 0;  // the longest packed list of a slice
    for (long p0 = 0; p0 < total; p0 += mb) {
        const long k = std::min<long>(mb, total - p0);
        size_t entries = 0;
        for (long x = first_ex(p0); x <= first_ex(p0 + k - 1); x++) entries += (size_t)n_moves[x];
        max_entries = std::max(max_entries, entries);
    }
    TG_HIP(hipSetDevice(e->cfg.device));
    Net* net = e->net;
    hipStream_t st = e->stream;
    TG_HIP(hipStreamSynchronize(st));  // (a self-play step may still be running: buffers are (re)allocated below)
    TG_HIP(net->ev_states.ensure((size_t)mb * sb));
    TG_HIP(net->ev_rec.ensure((size_t)mb * sizeof(int4)));
    TG_HIP(net->ev_moves.ensure(max_entries * sizeof(uint16_t)));
    TG_HIP(net->ev_visits.ensure(max_entries * sizeof(uint32_t)));
    TG_HIP(net->ev_rows.ensure((size_t)mb * 16));
    TG_HIP(net->ev_ent.ensure((size_t)mb * 4));
    TG_HIP(net->ev_acc.ensure(48));
    TG_HIP(e->s_policy.ensure((size_t)mb * P * 4));
    TG_HIP(e->s_eval.ensure((size_t)mb * 4));
    TG_HIP(hipMemsetAsync(net->ev_acc.p, 0, 48, st));
    // FULL logits rows: the search's gather target (armed only inside its own calls) must not take the FC's output
    net_set_gather(e, nullptr);
    int ld = 0;
    const float* fc_logits = net_fc_logits(e, &ld);
    EvalLogits L;
    if (fc_logits) L = EvalLogits{fc_logits, (size_t)ld, 1, ld, P, nullptr};  // logits-only forward: v = tanh(logit P), as k_softmax_stats takes it
    else if (net->head.kind == HEAD_CONV_F32) {
        const int cs = net->policy_conv.cout_pad;
        L = EvalLogits{net->logits.as<float>(), (size_t)nsq * cs, nsq, cs, P / nsq, e->s_eval.as<float>()};
    } else L = EvalLogits{net->logits.as<float>(), (size_t)net->head.ld, 1, net->head.ld, P, e->s_eval.as<float>()};
    std::vector<int4> h_rec;
    std::vector<uint16_t> h_moves;
    std::vector<uint32_t> h_visits;
    for (long p0 = 0; p0 < total; p0 += mb) {
        const int k = (int)std::min<long>(mb, total - p0);
        const long ex0 = first_ex(p0), ex1 = first_ex(p0 + k - 1);
        const int kex = (int)(ex1 - ex0 + 1), phase = (int)(symm ? p0 - 8 * ex0 : 0);
        h_rec.resize(kex);
        h_moves.clear();
        h_visits.clear();
        for (int i = 0; i < kex; i++) {
            const size_t x = (size_t)(ex0 + i);
            int32_t zbits;
            std::memcpy(&zbits, &results[x], 4);
            h_rec[i] = int4{(int)h_moves.size(), n_moves[x], zbits, 0};
            h_moves.insert(h_moves.end(), moves + x * TG_MAX_MOVES, moves + x * TG_MAX_MOVES + n_moves[x]);
            h_visits.insert(h_visits.end(), visits + x * TG_MAX_MOVES, visits + x * TG_MAX_MOVES + n_moves[x]);
        }
        uint8_t* d_pos = e->s_states.as<uint8_t>();
        TG_HIP(hipMemcpyAsync(symm ? net->ev_states.p : (void*)d_pos, hs + (size_t)ex0 * sb, (size_t)kex * sb, hipMemcpyHostToDevice, st));
        TG_HIP(hipMemcpyAsync(net->ev_rec.p, h_rec.data(), (size_t)kex * sizeof(int4), hipMemcpyHostToDevice, st));
        TG_HIP(hipMemcpyAsync(net->ev_moves.p, h_moves.data(), h_moves.size() * sizeof(uint16_t), hipMemcpyHostToDevice, st));
        TG_HIP(hipMemcpyAsync(net->ev_visits.p, h_visits.data(), h_visits.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        if (symm) {
            launch_eval_images(st, net->ev_states.as<uint8_t>(), k, phase, e->g.n, d_pos);
            TG_HIP(hipGetLastError());
        }
        if (int rc = net_forward_states_dev(e, k, d_pos, fc_logits ? nullptr : e->s_policy.as<float>(), e->s_eval.as<float>()); rc) return rc;
        TG_HIP(launch_example_metrics(st, L, net->ev_rec.as<int4>(), net->ev_moves.as<uint16_t>(), net->ev_visits.as<uint32_t>(), k, phase, symm,
                                      e->g.n, e->legacy5, e->lut5.as<int16_t>(), net->ev_rows.as<float>(), net->ev_ent.as<float>()));
        TG_HIP(launch_eval_sum(st, net->ev_rows.as<float>(), net->ev_ent.as<float>(), net->ev_rec.as<int4>(), k, phase, symm, net->ev_acc.as<double>()));
        if (rows) TG_HIP(hipMemcpyAsync(rows + (size_t)p0 * 4, net->ev_rows.p, (size_t)k * 16, hipMemcpyDeviceToHost, st));
        // (the host lists are rebuilt for the next slice: their copies must have left them)
        TG_HIP(hipStreamSynchronize(st));
    }
    if (int rc = net_poll_errors(e); rc) return rc;
    uint64_t acc[6];
    TG_HIP(hipMemcpy(acc, net->ev_acc.p, 48, hipMemcpyDeviceToHost));
    std::memcpy(&sums->loss_p, &acc[0], 8);
    std::memcpy(&sums->loss_z, &acc[1], 8);
    std::memcpy(&sums->target_entropy, &acc[2], 8);
    sums->top1 = acc[3];
    sums->sign_ok = acc[4];
    sums->decided = acc[5];
    sums->positions = (uint64_t)total;
    return TG_OK;
}

}  // extern "C"
