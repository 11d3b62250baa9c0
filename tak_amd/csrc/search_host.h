// search_host.h — what the two host files of the search share (search.hip: allocation, the iteration driver, tg_search_*;
// selfplay.hip: tg_selfplay_*).  Private to them.
#pragma once
#include "engine.h"
#include "kernels.h"
#include "search.cuh"

namespace tg {

// typed views of the buffers that no device struct carries (bound beside SearchDev's and SelfPlayDev's fields)
struct SearchAux {
    int32_t* op;         // [G] per-game re-root operation (launch_reroot)
    uint8_t* active;     // [G] a caller's mask, staged
    float* noise;        // [G][EX_MOVES] tg_search_apply_noise
    uint16_t* s_moves;   // [G] tg_search_play
    float* child_logit;  // [G·batch][EX_MOVES] the FC epilogue's gather target (bind_logits arms SearchDev.child_logit with it)
    // tg_search_root
    uint16_t* r_moves;   // [G][EX_MOVES]
    uint32_t* r_visits;  // [G][EX_MOVES]
    float *r_prior, *r_q;  // [G][EX_MOVES]
    int32_t* r_counts;   // [G]
    uint32_t* r_rv;      // [G]
    float* r_rq;         // [G]
    // rollout schedule
    int32_t *boost_list, *boost_count;  // [G] ascending game indices; their count
};

struct Search {
    TgSearchConfig cfg;
    SearchDev d{};
    SearchAux aux{};
    DevBuf hot, cold, root, alloc, chunk_head, chunk_link, chunk_fwd, chunk_used, free_ring, pool_ctl, root_state, alive, generation, path_len, path, leaf_kind, leaf_rec, child_pidx, child_logit, leaf_hash, planes, leaf_state, policy, eval,
        ctab, err, counters, op, active, noise, abort;
    DevBuf r_moves, r_visits, r_prior, r_q, r_counts, r_rv, r_rq, s_moves;
    DevBuf dbg_moves, dbg_visits, dbg_reward, dbg_policy, dbg_counts, dbg_eval, dbg_cmoves, dbg_cvisits, dbg_clen;  // tg_search_debug, one slice
    // self-play
    bool selfplay = false;
    TgSelfPlayConfig spcfg;
    SelfPlayDev p{};
    DevBuf st_hdr, st_state, st_moves, st_visits, st_count, out_hdr, out_state, out_moves, out_visits, fin, recycle, out_off, chosen,
        mask, stats;
    unsigned long long drained = 0, dropped = 0;
    int proof = 0;  // tg_search_set_proof: TG_PROOF_ON = the PROOF instantiations of the selects and of the self-play pick
    bool proof_ran = false;  // iterations have run under TG_PROOF_ON since the trees were last reset: they may hold TG_PROVEN_* codes
    DevBuf p_root, p_child, p_counts;  // tg_search_proof
    DevBuf re_status;                  // tg_reanalyse: one status byte per row of the call's range
    // rollout schedule (tg_selfplay_set_schedule): games under boost_plies run boost_factor × rollouts iterations, the extra
    // ones over a compacted list of those games
    TgRolloutSchedule sched{};
    bool stepped = false;           // tg_selfplay_step has run: the schedule is fixed
    DevBuf boost_list, boost_count;
    int32_t* h_boost_count = nullptr;  // pinned: the count sizes the grid and the network batch, so the host has to see it
    unsigned long long boosted_moves = 0, compact_iterations = 0, compact_leaves = 0;
    ~Search() { if (h_boost_count) (void)hipHostFree(h_boost_count); }
};

int need_search(TgEngine* e);      // the guard of every entry point: an engine with a search, on its device
int sync_and_check(TgEngine* e);   // stream sync, then the device error words → status
int read_counters(TgEngine* e, unsigned long long* expansions, unsigned long long* evals);
// tree_growth: how many times faster than one leaf per iteration a tree grows under the caller's schedule — the self-play
// driver runs `rollouts` ITERATIONS per move whatever the batch, so its trees are `batch` times larger; a caller-driven search
// decides its own iteration count (1).  Only the automatic pool size looks at it.
int search_alloc(TgEngine* e, const TgSearchConfig* cfg, size_t tree_growth = 1);
int pool_init(TgEngine* e, Search* s);  // every chunk but chunk 0 free, no game owning one (tg_search_reset, tg_reanalyse); synchronises
int search_reset_trees(TgEngine* e);  // every tree = Node::default(), every game alive with the given root state
// `iters` lock-step iterations, no host synchronisation inside: over the games of the device mask `d_active` (null: all), or over
// the compacted `list` of `count` games (null: all)
int search_iterate(TgEngine* e, int iters, const uint8_t* d_active = nullptr, const int32_t* list = nullptr, int count = 0);

}  // namespace tg
