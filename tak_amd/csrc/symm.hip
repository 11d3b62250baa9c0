// symm.hip — host side of the dihedral symmetries at the evaluation seam and in the search: the permutation tables built at
// tg_net_finalize, tg_policy_eval_symm / tg_policy_eval_symm_dev (images → one forward → gather-mean) and the search's hashed
// leaf image (tg_search_set_symmetry, the step search_iterate puts between the tree kernel and the forward).  No counterpart in
// the reference, which applies Symmetry (tak/src/symm.rs:11-20) to training examples only; kernels in symm_kernels.hip.
#include <algorithm>
#include <cstring>

#include "search_host.h"

namespace tg {

int symm_tables_build(TgEngine* e) {
    const size_t P = (size_t)e->policy_size;
    if (e->symm_perm.p) return TG_OK;  // a function of board size and policy head, not of the weights
    TG_HIP(e->symm_perm.ensure(8 * P * sizeof(int32_t)));
    TG_HIP(e->symm_count.ensure(sizeof(unsigned long long)));
    TG_HIP(hipMemsetAsync(e->symm_perm.p, 0xFF, 8 * P * sizeof(int32_t), e->stream));  // −1: a slot without an image
    TG_HIP(hipMemsetAsync(e->symm_count.p, 0, sizeof(unsigned long long), e->stream));
    TG_HIP(launch_symm_perm(e->stream, e->g.n, (int)P, e->legacy5, e->lut5.as<int16_t>(), e->symm_perm.as<int32_t>()));
    return TG_OK;
}

int symm_search_prepare(TgEngine* e) {
    Search* s = e->search;
    if (!s || e->symm_mode != TG_SYMM_HASHED || s->leaf_state.p) return TG_OK;
    // a tower that takes planes gets them from the tree kernel; the image is taken of a packed state, so under the hashed mode
    // the tree kernel leaves packed leaves and the forward encodes them (net_forward_states_dev): the same planes
    const size_t bytes = (size_t)s->d.G * (size_t)s->d.batch * e->g.bytes;
    TG_HIP(s->leaf_state.ensure(bytes));
    TG_HIP(hipMemsetAsync(s->leaf_state.p, 0, bytes, e->stream));
    return TG_OK;
}

int symm_search_leaves(TgEngine* e, const SearchDev& d, int leaves) {
    TG_HIP(launch_symm_leaves(e->stream, d, leaves, e->symm_perm.as<int32_t>(), e->symm_count.as<unsigned long long>()));
    return TG_OK;
}

static int check_symm_call(TgEngine* e, const char* who, int n, uint32_t mask) {
    if (!e) return fail(TG_ERR_INVALID_ARG, std::string(who) + ": null engine");
    if (e->cfg.evaluator != TG_EVAL_RESNET || !e->net) return fail(TG_ERR_STATE, std::string(who) + ": the engine's evaluator is not TG_EVAL_RESNET");
    if (mask == 0 || mask > 0xFFu) return fail(TG_ERR_INVALID_ARG, std::string(who) + ": mask must select at least one of the 8 symmetries (bits 0..7)");
    if (n < 0) return fail(TG_ERR_INVALID_ARG, std::string(who) + ": n out of range");
    if (!net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    return TG_OK;
}

// n·k ≤ max_batch states on the device → the folded outputs on the device; no synchronisation
static int eval_symm_dev(TgEngine* e, int n, const uint8_t* d_states, uint32_t mask, float* d_policy, float* d_eval) {
    const int k = __builtin_popcount(mask), P = e->policy_size;
    if (mask == 1u) return net_forward_states_dev(e, n, d_states, d_policy, d_eval);  // the identity alone: tg_policy_eval_dev
    TG_HIP(e->s_policy.ensure((size_t)e->cfg.max_batch * P * 4));
    TG_HIP(e->s_eval.ensure((size_t)e->cfg.max_batch * 4));
    uint8_t* images = e->s_states.as<uint8_t>();
    TG_HIP(launch_symm_images(e->stream, d_states, n, k, mask, e->g.n, images));
    if (int rc = net_forward_states_dev(e, n * k, images, e->s_policy.as<float>(), e->s_eval.as<float>()); rc) return rc;
    TG_HIP(launch_symm_fold(e->stream, e->s_policy.as<float>(), e->s_eval.as<float>(), e->symm_perm.as<int32_t>(), n, P, k, mask, d_policy, d_eval));
    return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_policy_eval_symm_dev(TgEngine* e, int n, const void* d_states, uint32_t mask, float* d_policy, float* d_eval) {
    if (int rc = check_symm_call(e, "tg_policy_eval_symm_dev", n, mask); rc) return rc;
    if ((long long)n * __builtin_popcount(mask) > e->cfg.max_batch) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_symm_dev: n x popcount(mask) exceeds max_batch");
    if (n == 0) return TG_OK;
    if (!d_states || !d_policy || !d_eval) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_symm_dev: null argument");
    if (d_states == e->s_states.p) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_symm_dev: d_states is the engine's own staging buffer");
    TG_HIP(hipSetDevice(e->cfg.device));
    return eval_symm_dev(e, n, (const uint8_t*)d_states, mask, d_policy, d_eval);
}

int tg_policy_eval_symm(TgEngine* e, int n, const void* states, uint32_t mask, float* policy, float* eval) {
    if (int rc = check_symm_call(e, "tg_policy_eval_symm", n, mask); rc) return rc;
    if (n == 0) return TG_OK;
    if (!states || !policy || !eval) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_symm: null argument");
    const int k = __builtin_popcount(mask), per = e->cfg.max_batch / k;
    if (per < 1) return fail(TG_ERR_INVALID_ARG, "tg_policy_eval_symm: max_batch is smaller than the number of selected symmetries");
    TG_HIP(hipSetDevice(e->cfg.device));
    const size_t sb = e->g.bytes, P = (size_t)e->policy_size;
    TG_HIP(e->symm_src.ensure((size_t)per * sb));
    TG_HIP(e->symm_policy.ensure((size_t)per * P * 4));
    TG_HIP(e->symm_eval.ensure((size_t)per * 4));
    for (int off = 0; off < n; off += per) {
        const int c = std::min(per, n - off);
        TG_HIP(hipMemcpyAsync(e->symm_src.p, (const uint8_t*)states + (size_t)off * sb, (size_t)c * sb, hipMemcpyHostToDevice, e->stream));
        if (int rc = eval_symm_dev(e, c, e->symm_src.as<uint8_t>(), mask, e->symm_policy.as<float>(), e->symm_eval.as<float>()); rc) return rc;
        TG_HIP(hipMemcpyAsync(policy + (size_t)off * P, e->symm_policy.p, (size_t)c * P * 4, hipMemcpyDeviceToHost, e->stream));
        TG_HIP(hipMemcpyAsync(eval + off, e->symm_eval.p, (size_t)c * 4, hipMemcpyDeviceToHost, e->stream));
        TG_HIP(hipStreamSynchronize(e->stream));
        if (int rc = net_poll_errors(e); rc) return rc;
    }
    return TG_OK;
}

int tg_symm_perm_read(TgEngine* e, int32_t* perm) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_symm_perm_read: null engine");
    if (e->cfg.evaluator != TG_EVAL_RESNET || !e->net) return fail(TG_ERR_STATE, "tg_symm_perm_read: the engine's evaluator is not TG_EVAL_RESNET");
    if (!perm) return fail(TG_ERR_INVALID_ARG, "tg_symm_perm_read: null argument");
    if (!net_ready(e) || !e->symm_perm.p) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    TG_HIP(hipSetDevice(e->cfg.device));
    TG_HIP(hipMemcpyAsync(perm, e->symm_perm.p, 8 * (size_t)e->policy_size * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    TG_HIP(hipStreamSynchronize(e->stream));
    return TG_OK;
}

int tg_search_set_symmetry(TgEngine* e, int mode) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_search_set_symmetry: null engine");
    if (mode != TG_SYMM_OFF && mode != TG_SYMM_HASHED) return fail(TG_ERR_INVALID_ARG, "tg_search_set_symmetry: unknown mode");
    if (e->cfg.evaluator != TG_EVAL_RESNET || !e->net) return fail(TG_ERR_STATE, "tg_search_set_symmetry: the engine's evaluator is not TG_EVAL_RESNET");
    if (mode != TG_SYMM_OFF && !net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    TG_HIP(hipSetDevice(e->cfg.device));
    e->symm_mode = mode;
    return symm_search_prepare(e);
}

int tg_search_get_symmetry(TgEngine* e, int* mode, uint64_t* leaves_transformed) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_search_get_symmetry: null engine");
    if (mode) *mode = e->symm_mode;
    if (leaves_transformed) {
        *leaves_transformed = 0;
        if (e->symm_count.p) {
            TG_HIP(hipSetDevice(e->cfg.device));
            TG_HIP(hipStreamSynchronize(e->stream));
            unsigned long long c = 0;
            TG_HIP(hipMemcpy(&c, e->symm_count.p, sizeof c, hipMemcpyDeviceToHost));
            *leaves_transformed = (uint64_t)c;
        }
    }
    return TG_OK;
}

}  // extern "C"
