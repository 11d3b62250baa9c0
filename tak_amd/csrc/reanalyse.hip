// reanalyse.hip — host side of tg_reanalyse (include/takgpu.h): re-search a logical range of the example window (window.hip) with
// the deployed network on the engine's caller-driven search object and write the new root visit counts into the rows in place —
// MuZero's Reanalyse restricted to the policy target.  No counterpart in the reference: training_loop trains on the whole window
// each round (train/src/main.rs:82-95) with the targets (Node::improved_policy, alpha-tak/src/search/play.rs:13-21) of whichever
// network searched a row when it was born.  The rows never leave the device: only the error word, the search counters and one
// status byte per row reach the host.  Kernels in reanalyse_kernels.hip.
//
// Per slice of `games` rows:  k_reanalyse_roots | k_reroot(−2) + k_pool_publish | [1 iteration | k_dirichlet] | `rollouts`
// iterations (search_iterate: one tree kernel per iteration) | wait, error word | k_reanalyse_store.
#include <algorithm>

#include "search_host.h"
#include "window.h"

using namespace tg;

namespace {

std::string field(const char* name) { return std::string("tg_reanalyse: ") + name; }

// the search object's own slot_base, back in place however the call ends
struct SlotBaseScope {
    Search* s;
    uint32_t kept;
    ~SlotBaseScope() { s->d.slot_base = kept; }
};

}  // namespace

extern "C" int tg_reanalyse(TgEngine* e, int first, int count, const TgReanalyseConfig* cfg, TgReanalyseStats* out) {
    if (!e) return fail(TG_ERR_INVALID_ARG, field("null engine"));
    if (!cfg) return fail(TG_ERR_INVALID_ARG, field("null cfg"));
    if (cfg->rollouts < 1) return fail(TG_ERR_INVALID_ARG, field("cfg.rollouts must be at least 1"));
    if (!(cfg->noise_alpha >= 0.0f)) return fail(TG_ERR_INVALID_ARG, field("cfg.noise_alpha must be 0 (no noise) or positive"));
    if (!(cfg->noise_ratio >= 0.0f && cfg->noise_ratio <= 1.0f)) return fail(TG_ERR_INVALID_ARG, field("cfg.noise_ratio must be in [0, 1]"));
    if (cfg->flags != 0) return fail(TG_ERR_INVALID_ARG, field("cfg.flags must be 0"));
    for (int i = 0; i < 4; i++)
        if (cfg->reserved[i] != 0) return fail(TG_ERR_INVALID_ARG, field("cfg.reserved must be 0"));
    if (first < 0) return fail(TG_ERR_INVALID_ARG, field("negative first"));
    if (count < 0) return fail(TG_ERR_INVALID_ARG, field("negative count"));
    TG_HIP(hipSetDevice(e->cfg.device));
    WindowDev W;
    uint64_t kept = 0, evicted = 0;
    if (!window_view(e, &W, &kept, &evicted)) return fail(TG_ERR_STATE, field("the engine has no example window (tg_window_create)"));
    Search* s = e->search;
    if (!s) return fail(TG_ERR_STATE, field("the engine has no search object (tg_search_create)"));
    if (s->selfplay) return fail(TG_ERR_STATE, field("the engine's search object is a self-play driver, whose games the call would destroy (tg_search_create)"));
    if ((uint64_t)first + (uint64_t)count > kept)
        return fail(TG_ERR_INVALID_ARG, field("first, count: [") + std::to_string(first) + ", " + std::to_string((long long)first + count) +
                                            ") is not inside the window's [0, " + std::to_string(kept) + ")");
    if (out) *out = TgReanalyseStats{};
    if (count == 0) return TG_OK;

    hipStream_t st = e->stream;
    const int G = s->d.G;
    uint8_t* d_status = nullptr;
    TG_HIP(bind(s->re_status, d_status, (size_t)count));
    TG_HIP(hipStreamSynchronize(st));  // what ran on the object before has finished: its counters are final
    unsigned long long before[2], after[2];
    int rc = read_counters(e, &before[0], &before[1]);
    if (rc) return rc;
    // as tg_search_reset: every tree dropped, the pool whole again (whatever an earlier exhaustion left of it), no sticky error.
    // Once per call; between slices the reset of launch_reroot returns a tree's chunks itself
    if ((rc = pool_init(e, s))) return rc;
    TG_HIP(hipMemsetAsync(s->err.p, 0, 4, st));
    TG_HIP(hipMemsetAsync(d_status, 0, (size_t)count, st));
    SlotBaseScope scope{s, s->d.slot_base};
    rc = TG_OK;
    for (int done = 0; done < count && rc == TG_OK; done += G) {
        const int k = std::min(G, count - done);
        const uint64_t at = (uint64_t)first + (uint64_t)done;  // logical index of the slice's first row; its cursor is evicted + at
        const uint32_t row0 = (uint32_t)ring_row(evicted, at, W.capacity);
        s->d.slot_base = (uint32_t)(evicted + at);  // slot g of the slice draws its noise as cursor evicted + at + g
        TG_HIP(launch_reanalyse_roots(st, s->d, W, row0, k, s->aux.op));
        launch_reroot(st, s->d, s->aux.op);
        TG_HIP(hipGetLastError());
        s->proof_ran = false;
        if (cfg->noise_alpha > 0.0f) {  // Player::add_noise: the root is expanded by one rollout, then noised
            if ((rc = search_iterate(e, 1))) break;
            launch_dirichlet(st, s->d, nullptr, cfg->noise_alpha, cfg->noise_ratio);
            TG_HIP(hipGetLastError());
        }
        if ((rc = search_iterate(e, cfg->rollouts))) break;
        if ((rc = sync_and_check(e))) break;  // a slice that ended in an error stores nothing
        TG_HIP(launch_reanalyse_store(st, s->d, W, row0, k, d_status + done));
    }
    const std::string msg = rc ? tg_last_error() : "";
    TG_HIP(hipStreamSynchronize(st));
    std::vector<uint8_t> status((size_t)count);
    TG_HIP(hipMemcpy(status.data(), d_status, (size_t)count, hipMemcpyDeviceToHost));
    if (int rc2 = read_counters(e, &after[0], &after[1])) return rc2;
    if (out) {
        out->rows = (uint64_t)count;
        for (uint8_t b : status) {
            out->updated += b == REANALYSE_UPDATED;
            out->mismatched += b == REANALYSE_MISMATCHED;
            out->unvisited += b == REANALYSE_UNVISITED;
        }
        out->expansions = after[0] - before[0];
        out->evals = after[1] - before[1];
    }
    return rc ? fail(rc, msg) : TG_OK;
}
