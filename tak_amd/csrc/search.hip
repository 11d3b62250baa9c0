// search.hip — host side of the search entry points of include/takgpu.h: device allocation, the per-iteration schedule
// (select → network → backup, no host synchronisation inside a call), result read-back and the tree dump.  The self-play
// entry points are selfplay.hip's.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>

#include "search_host.h"

namespace tg {

void search_destroy(Search* s) { delete s; }

static int describe_errors(uint32_t bits) {
    std::string msg;
    int code = TG_ERR_STATE;
    auto add = [&](uint32_t b, const char* m, int c) {
        if (bits & b) { if (!msg.empty()) msg += "; "; msg += m; code = c; }
    };
    add(ERRF_DEPTH, "selection path deeper than 256 plies (TG_LIMIT_DEPTH)", TG_ERR_LIMIT);
    add(ERRF_CTAB, "a node was visited more often than the exploration-rate table is long (TG_LIMIT_VISITS / TgSearchConfig.visit_limit)", TG_ERR_LIMIT);
    add(ERRF_EXAMPLES, "a game lasted more than 512 plies (TG_LIMIT_GAME_PLIES)", TG_ERR_LIMIT);
    add(ERRF_MOVES, "a position has more than TG_MAX_MOVES legal moves", TG_ERR_LIMIT);
    add(ERRF_PICK, "pick_move on a root without visits", TG_ERR_STATE);
    add(ERRF_MOVE, "move is not a child of the root / has no policy index", TG_ERR_ILLEGAL_MOVE);
    add(ERRF_NAN, "NaN upper confidence bound (reference: \"tried comparing nan\")", TG_ERR_NAN);
    add(ERRF_ARENA, "MCTS node pool exhausted (raise TgSearchConfig.arena_nodes)", TG_ERR_ARENA_OVERFLOW);
    return fail(code, msg);
}

int search_poll_errors(TgEngine* e) {
    if (int rc = net_poll_errors(e)) return rc;
    if (!e || !e->search) return TG_OK;
    uint32_t bits = 0;
    TG_HIP(hipMemcpy(&bits, e->search->err.p, 4, hipMemcpyDeviceToHost));
    if (!bits) return TG_OK;
    return describe_errors(bits);
}

int need_search(TgEngine* e) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "null engine");
    if (!e->search) return fail(TG_ERR_STATE, "tg_search_create / tg_selfplay_create has not been called");
    TG_HIP(hipSetDevice(e->cfg.device));
    return TG_OK;
}

static int upload_mask(TgEngine* e, const uint8_t* active, const uint8_t** d_out) {
    *d_out = nullptr;
    if (!active) return TG_OK;
    Search* s = e->search;
    TG_HIP(hipMemcpyAsync(s->active.p, active, (size_t)s->d.G, hipMemcpyHostToDevice, e->stream));
    *d_out = s->aux.active;
    return TG_OK;
}

// Every chunk but chunk 0 free, no game owning one: the state after create and after tg_search_reset (which drops every
// tree, and with them a pool that an exhaustion has left inconsistent).  search_reset_trees then gives each game its root chunk.
int pool_init(TgEngine* e, Search* s) {
    const size_t G = (size_t)s->cfg.games, n_chunks = s->d.n_chunks;
    const int chunk_shift = s->d.chunk_shift;
    std::vector<uint32_t> ring(n_chunks, 0u);
    for (size_t i = 0; i + 1 < n_chunks; i++) ring[i] = (uint32_t)(i + 1);
    const unsigned long long ctl[4] = {0ull, (unsigned long long)(n_chunks - 1), (unsigned long long)(n_chunks - 1), 0ull};
    // everything on the engine's (non-blocking) stream: a legacy-stream hipMemset would not be ordered against the
    // kernels that follow on it
    hipStream_t st = e->stream;
    TG_HIP(hipMemcpyAsync(s->free_ring.p, ring.data(), n_chunks * 4, hipMemcpyHostToDevice, st));
    TG_HIP(hipMemcpyAsync(s->pool_ctl.p, ctl, sizeof ctl, hipMemcpyHostToDevice, st));
    TG_HIP(hipMemsetAsync(s->chunk_head.p, 0, G * 4, st));
    TG_HIP(hipMemsetAsync(s->chunk_link.p, 0, n_chunks * 4, st));
    TG_HIP(hipMemsetAsync(s->root.p, 0, G * 4, st));
    TG_HIP(hipMemsetAsync(s->alloc.p, 0, G * 8, st));
    // chunk 0 is where a not-yet-reset game's root index (0) points: an empty node without children
    TG_HIP(hipMemsetAsync(s->hot.p, 0, sizeof(NodeHot) << chunk_shift, st));
    TG_HIP(hipMemsetAsync(s->cold.p, 0, sizeof(NodeCold) << chunk_shift, st));
    TG_HIP(hipStreamSynchronize(st));  // `ring` / `ctl` are host temporaries
    return TG_OK;
}

int search_alloc(TgEngine* e, const TgSearchConfig* cfg, size_t tree_growth) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "null engine");
    if (!cfg || cfg->games <= 0 || cfg->games > e->cfg.max_batch) return fail(TG_ERR_INVALID_ARG, "games must be in 1..max_batch");
    const size_t B = cfg->batch ? cfg->batch : 1;  // virtual rollouts per tree and iteration
    if (B > 4096 || (e->cfg.evaluator == TG_EVAL_RESNET && (size_t)cfg->games * B > (size_t)e->cfg.max_batch))
        return fail(TG_ERR_INVALID_ARG, "games x batch leaves per iteration exceed max_batch");
    if (cfg->arena_nodes != 0 && cfg->arena_nodes < 1024) return fail(TG_ERR_INVALID_ARG, "arena_nodes must be 0 (auto) or at least 1024");
    if (cfg->visit_limit < 0 || (cfg->visit_limit != 0 && cfg->visit_limit < 16) || cfg->visit_limit > TG_LIMIT_VISITS)
        return fail(TG_ERR_INVALID_ARG, "visit_limit must be 0 (= TG_LIMIT_VISITS) or in 16..TG_LIMIT_VISITS");
    if (e->cfg.evaluator == TG_EVAL_RESNET && !net_ready(e)) return fail(TG_ERR_STATE, "network weights not finalized (tg_net_finalize)");
    TG_HIP(hipSetDevice(e->cfg.device));
    if (e->search) {
        TG_HIP(hipStreamSynchronize(e->stream));
        net_set_gather(e, nullptr);  // (its buffers go with the search)
        search_destroy(e->search);
        e->search = nullptr;
    }
    e->symm_mode = TG_SYMM_OFF;  // tg_search_set_symmetry is sticky for ONE search object
    std::unique_ptr<Search> sp(new Search());
    Search* s = sp.get();
    s->cfg = *cfg;
    // One node pool for all games (search.cuh).  arena_nodes is the AVERAGE budget per game: pool = games × arena_nodes,
    // and a single tree may grow far beyond it while others are small.  0 = auto: half of the free device memory,
    // at most 2^22 nodes per game (the reference's 10 000 rollouts on 6×6 peak at ≈ 2^20 per game) and at most what a
    // 32-bit node index addresses.
    const size_t node_bytes = sizeof(NodeHot) + sizeof(NodeCold);
    size_t pool_nodes;
    if (s->cfg.arena_nodes == 0) {
        size_t free_b = 0, total_b = 0;
        TG_HIP(hipMemGetInfo(&free_b, &total_b));
        // (a 32-bit node index addresses 2^32 nodes; the slack chunks added below count against that)
        const size_t index_limit = ((size_t)1 << 32) - (((size_t)3 * cfg->games + 2) << 11);
        // (the 2^22 per game are the reference's 10 000 one-leaf rollouts with a factor 4 to spare; `tree_growth` leaves per
        // iteration keep that factor as long as memory and the index allow)
        pool_nodes = std::min<size_t>({free_b / 2 / node_bytes, ((size_t)cfg->games << 22) * tree_growth, index_limit});
        pool_nodes = std::max<size_t>(pool_nodes, (size_t)cfg->games << 12);
        s->cfg.arena_nodes = (int32_t)std::min<size_t>(pool_nodes / (size_t)cfg->games, (size_t)1 << 30);
    } else {
        pool_nodes = (size_t)cfg->games * (size_t)cfg->arena_nodes;
        if (pool_nodes > ((size_t)1 << 32) - (((size_t)3 * cfg->games + 2) << 11))
            return fail(TG_ERR_INVALID_ARG, "games x arena_nodes exceeds the 2^32 nodes a pool can hold");
    }
    cfg = &s->cfg;
    const size_t G = (size_t)cfg->games;
    const int chunk_shift = pool_nodes / G >= 16384 ? 11 : 10;
    // + 3 chunks per game: the open chunk's unused tail, the first chunk of a re-rooted copy while the old tree still
    // holds its own, and chunk 0, which is never handed out (index 0 = "no children")
    const size_t n_chunks = (pool_nodes >> chunk_shift) + 3 * G + 1;
    if ((n_chunks << chunk_shift) > ((size_t)1 << 32)) return fail(TG_ERR_INVALID_ARG, "node pool exceeds 2^32 nodes");
    const int cin_pad = e->cin_pad;
    // one line per device buffer: sized in elements of the field it is bound to
    SearchDev& d = s->d;
    SearchAux& x = s->aux;
    TG_HIP(bind(s->hot, d.hot, n_chunks << chunk_shift));
    TG_HIP(bind(s->cold, d.cold, n_chunks << chunk_shift));
    TG_HIP(bind(s->root, d.root, G));
    TG_HIP(bind(s->alloc, d.alloc, G * 2));
    TG_HIP(bind(s->chunk_head, d.chunk_head, G));
    TG_HIP(bind(s->chunk_link, d.chunk_link, n_chunks));
    TG_HIP(bind(s->chunk_fwd, d.chunk_fwd, n_chunks));
    TG_HIP(bind(s->chunk_used, d.chunk_used, n_chunks));
    TG_HIP(bind(s->free_ring, d.free_ring, n_chunks));
    TG_HIP(bind(s->pool_ctl, d.pool_ctl, 4));
    TG_HIP(bind(s->root_state, d.root_state, G * e->g.bytes));
    TG_HIP(bind(s->alive, d.alive, G));
    TG_HIP(bind(s->abort, d.abort, G));
    TG_HIP(bind(s->generation, d.generation, G));
    TG_HIP(bind(s->path_len, d.path_len, G * B));
    TG_HIP(bind(s->path, d.path, G * B * MAX_DEPTH));
    TG_HIP(bind(s->leaf_kind, d.leaf_kind, G * B));
    TG_HIP(bind(s->leaf_rec, d.leaf_rec, G * B * 2));
    TG_HIP(bind(s->child_pidx, d.child_pidx, G * B * EX_MOVES));
    TG_HIP(bind(s->child_logit, x.child_logit, G * B * EX_MOVES));
    TG_HIP(hipMemsetAsync(s->leaf_rec.p, 0, G * B * 8, e->stream));
    TG_HIP(bind(s->leaf_hash, d.leaf_hash, G * B));
    TG_HIP(bind(s->op, x.op, G));
    TG_HIP(bind(s->active, x.active, G));
    TG_HIP(bind(s->noise, x.noise, G * EX_MOVES));
    TG_HIP(bind(s->err, d.err, 1));
    TG_HIP(bind(s->counters, d.counters, G * 4));  // (the second half: the proof counters)
    TG_HIP(bind(s->r_moves, x.r_moves, G * EX_MOVES));
    TG_HIP(bind(s->r_visits, x.r_visits, G * EX_MOVES));
    TG_HIP(bind(s->r_prior, x.r_prior, G * EX_MOVES));
    TG_HIP(bind(s->r_q, x.r_q, G * EX_MOVES));
    TG_HIP(bind(s->r_counts, x.r_counts, G));
    TG_HIP(bind(s->r_rv, x.r_rv, G));
    TG_HIP(bind(s->r_rq, x.r_rq, G));
    TG_HIP(bind(s->s_moves, x.s_moves, G));
    if (e->cfg.evaluator == TG_EVAL_RESNET) {
        if (net_takes_states(e)) {
            TG_HIP(bind(s->leaf_state, d.leaf_state, G * B * e->g.bytes));
            TG_HIP(hipMemsetAsync(s->leaf_state.p, 0, s->leaf_state.bytes, e->stream));
        } else
        TG_HIP(bind(s->planes, d.planes, G * B * e->g.nsq * cin_pad));
        TG_HIP(bind(s->policy, d.policy, G * B * (size_t)e->policy_size));
        TG_HIP(bind(s->eval, d.eval, G * B));
        if (s->planes.p) TG_HIP(hipMemsetAsync(s->planes.p, 0, s->planes.bytes, e->stream));
    }
    // exploration_rate(n) = ln((1 + n + base) / base) + init for integer visit counts (mcts.rs:10-12),
    // evaluated once on the host in f32 so that every GPU and the CPU agree on the last bit
    const int ctab_size = cfg->visit_limit ? cfg->visit_limit : TG_LIMIT_VISITS;
    std::vector<float> ctab(ctab_size);
    for (int i = 0; i < ctab_size; i++) {
        float nf = (float)i;
        ctab[i] = logf((1.0f + nf + cfg->exploration_base) / cfg->exploration_base) + cfg->exploration_init;
    }
    TG_HIP(bind(s->ctab, d.ctab, (size_t)ctab_size));
    TG_HIP(hipMemcpy(s->ctab.p, ctab.data(), (size_t)ctab_size * 4, hipMemcpyHostToDevice));
    TG_HIP(hipMemsetAsync(s->err.p, 0, 4, e->stream));
    TG_HIP(hipMemsetAsync(s->counters.p, 0, G * 32, e->stream));
    TG_HIP(hipMemsetAsync(s->generation.p, 0, G * 4, e->stream));
    TG_HIP(hipMemsetAsync(s->alive.p, 0, G, e->stream));
    TG_HIP(hipMemsetAsync(s->abort.p, 0, G, e->stream));
    d.n_chunks = (uint32_t)n_chunks; d.chunk_shift = chunk_shift; d.lut5 = e->lut5.as<int16_t>();
    if (int rc = pool_init(e, s)) return rc;
    d.G = cfg->games; d.n = e->g.n; d.cin_pad = cin_pad; d.P = e->policy_size; d.ctab_size = ctab_size;
    d.legacy5 = e->legacy5 ? 1 : 0; d.evaluator = e->cfg.evaluator; d.slot_base = cfg->slot_base; d.seed = cfg->seed;
    d.batch = (int)B; d.pass = 0;
    d.retire = 0;  // tg_selfplay_create turns it on: only the self-play driver can restart a game on its own
    d.logits = nullptr; d.logit_ld = 0; d.fc_stats = nullptr; d.fc_blocks = 0; d.fc_stride = 0; d.child_logit = nullptr;  // refreshed before every iteration (bind_logits)
    e->search = sp.release();
    return TG_OK;
}

int search_reset_trees(TgEngine* e) {
    Search* s = e->search;
    const size_t G = (size_t)s->d.G;
    std::vector<int32_t> op(G, -2);
    TG_HIP(hipMemcpyAsync(s->op.p, op.data(), G * 4, hipMemcpyHostToDevice, e->stream));
    launch_reroot(e->stream, s->d, s->aux.op);
    TG_HIP(hipGetLastError());
    TG_HIP(hipStreamSynchronize(e->stream));
    return TG_OK;
}

// FC-head networks: the backup reads the network's logits buffer directly (softmax statistics and tanh in the tree kernel,
// softmax.cuh).  Bound per call: the weights may have been re-finalised (tg_train_commit, another precision) since the
// search was created.
// `leaves`: rows of the forwards that follow (games × batch; a compacted iteration passes count × batch — whether the FC
// serves the gather depends on the batch, the bits do not)
static void bind_logits(TgEngine* e, int leaves) {
    Search* s = e->search;
    s->d.logits = nullptr;
    s->d.logit_ld = 0;
    s->d.fc_stats = nullptr;
    s->d.fc_blocks = 0;
    s->d.fc_stride = 0;
    s->d.child_logit = nullptr;
    net_set_gather(e, nullptr);
    if (e->cfg.evaluator != TG_EVAL_RESNET) return;
    int ld = 0;
    const float* lg = net_fc_logits(e, &ld);
    if (lg) {
        s->d.logits = lg; s->d.logit_ld = ld;
        int blocks = 0, stride = 0;
        const float* fs = net_fc_stats(e, &blocks, &stride);
        if (fs) { s->d.fc_stats = fs; s->d.fc_blocks = blocks; s->d.fc_stride = stride; }
        // exact-f32 FC at a batch its ring kernel serves: the FC's epilogue hands the backup the children's logits directly
        if (fs && !s->d.planes && net_gather_ok(e, leaves)) {
            const FcGatherArgs g{s->d.child_pidx, s->d.leaf_rec, s->aux.child_logit, EX_MOVES};
            net_set_gather(e, &g);
            s->d.child_logit = s->aux.child_logit;
        }
    }
}

// The gather target is armed for the iterations of ONE call and disarmed when it returns: a later logits-only forward by anyone
// else must not find the search's buffers behind a stale pointer.
struct GatherScope {
    TgEngine* e;
    ~GatherScope() { net_set_gather(e, nullptr); }
};

// `iters` lock-step iterations, each the body of train/src/self_play.rs:181-210.  `batch` virtual rollouts per tree (Player's
// batching model, alpha-tak/src/player.rs:77-93) run back to back inside the select kernel (a game's tree belongs to one wave),
// then ONE network batch of games × batch leaves, then the de-virtualisations in the same order inside the backup kernel.
//   d_active given:  select(mask) | net | backup, per iteration — the fused kernels take no mask
//   otherwise:       select(0) | net | backup(0)+select(1) | net | … | backup(iters-1): one tree kernel per iteration
//   list given:      the same over the compacted list of `count` games (0 < count < G): wave w serves list[w], leaf slots
//                    w·batch + pass, the network on count × batch leaves
//   TG_SYMM_HASHED:  one more kernel in front of every `net` (k_symm_leaves over the iteration's leaf slots); off: none
//   TG_PROOF_ON:     the same schedule with the PROOF instantiations of the selects; the backups are the same kernels
int search_iterate(TgEngine* e, int iters, const uint8_t* d_active, const int32_t* list, int count) {
    Search* s = e->search;
    if (iters <= 0 || (list && count <= 0)) return TG_OK;
    const int leaves = (list ? count : s->d.G) * s->d.batch;
    bind_logits(e, leaves);
    GatherScope scope{e};
    const bool proof = s->proof != 0;
    if (proof) s->proof_ran = true;
    SearchDev d = s->d;
    d.pass = d.batch > 1 ? -1 : 0;  // -1: the kernel runs the `batch` passes of a game back to back in that game's wave
    hipStream_t st = e->stream;
    // TG_SYMM_HASHED: every evaluated leaf goes to the network as its hashed dihedral image (symm.hip), from packed leaf states
    const bool symm = e->symm_mode == TG_SYMM_HASHED && e->cfg.evaluator == TG_EVAL_RESNET;
    if (symm) {
        if (int rc = symm_search_prepare(e); rc) return rc;
        if (d.planes) { d.planes = nullptr; d.leaf_state = s->leaf_state.as<uint8_t>(); }
    }
    for (int i = 0; i < iters; i++) {
        if (i == 0 || d_active) launch_select(st, d, d_active, list, count, proof);
        if (e->cfg.evaluator == TG_EVAL_RESNET) {
            if (symm) { if (int rc = symm_search_leaves(e, d, leaves); rc) return rc; }
            float* pol = d.logits ? nullptr : d.policy;  // logits mode: the backup takes softmax / tanh itself
            int rc = d.planes ? net_forward_dev(e, leaves, d.planes, pol, d.eval) : net_forward_states_dev(e, leaves, d.leaf_state, pol, d.eval);
            if (rc) return rc;
        }
        const bool last = d_active || i + 1 == iters;  // (nothing follows, or the next select needs the mask)
        if (last) launch_backup(st, d, list, count);
        else launch_backup_select(st, d, list, count, proof);
    }
    TG_HIP(hipGetLastError());
    return TG_OK;
}

int read_counters(TgEngine* e, unsigned long long* expansions, unsigned long long* evals) {
    Search* s = e->search;
    std::vector<unsigned long long> h((size_t)s->d.G * 2);
    TG_HIP(hipMemcpy(h.data(), s->counters.p, h.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long a = 0, b = 0;
    for (int g = 0; g < s->d.G; g++) { a += h[2 * (size_t)g]; b += h[2 * (size_t)g + 1]; }
    *expansions = a;
    *evals = b;
    return TG_OK;
}

int sync_and_check(TgEngine* e) {
    TG_HIP(hipStreamSynchronize(e->stream));
    return search_poll_errors(e);
}

// read-back of an optional output: `n` elements of its type; nothing for a null destination or an empty range
template <class T, class U>
static hipError_t copy_out(T* dst, const U* src, size_t n) {
    static_assert(sizeof(T) == sizeof(U), "host and device element differ");
    return dst && n ? hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_search_create(TgEngine* e, const TgSearchConfig* cfg) {
    return search_alloc(e, cfg);
}

int tg_search_reset(TgEngine* e, const void* states) {
    int rc = need_search(e);
    if (rc) return rc;
    if (!states) return fail(TG_ERR_INVALID_ARG, "tg_search_reset: null states");
    Search* s = e->search;
    rc = validate_states(e, s->d.G, (const uint8_t*)states, "tg_search_reset");
    if (rc) return rc;
    const size_t G = (size_t)s->d.G;
    rc = pool_init(e, s);
    if (rc) return rc;
    TG_HIP(hipMemcpyAsync(s->root_state.p, states, G * e->g.bytes, hipMemcpyHostToDevice, e->stream));
    TG_HIP(hipMemsetAsync(s->alive.p, 1, G, e->stream));
    TG_HIP(hipMemsetAsync(s->err.p, 0, 4, e->stream));
    s->proof_ran = false;
    return search_reset_trees(e);
}

int tg_search_run(TgEngine* e, int iters, const uint8_t* active) {
    int rc = need_search(e);
    if (rc) return rc;
    if (iters < 0) return fail(TG_ERR_INVALID_ARG, "tg_search_run: negative iters");
    const uint8_t* d_active;
    rc = upload_mask(e, active, &d_active);
    if (rc) return rc;
    rc = search_iterate(e, iters, d_active);
    if (rc) return rc;
    if (active) TG_HIP(hipStreamSynchronize(e->stream));  // the staged mask must outlive the launches
    return TG_OK;
}

int tg_search_apply_dirichlet(TgEngine* e, float alpha, float ratio, const uint8_t* active) {
    int rc = need_search(e);
    if (rc) return rc;
    const uint8_t* d_active;
    rc = upload_mask(e, active, &d_active);
    if (rc) return rc;
    launch_dirichlet(e->stream, e->search->d, d_active, alpha, ratio);
    TG_HIP(hipGetLastError());
    return sync_and_check(e);
}

int tg_search_apply_noise(TgEngine* e, const float* noise, float ratio, const uint8_t* active) {
    int rc = need_search(e);
    if (rc) return rc;
    if (!noise) return fail(TG_ERR_INVALID_ARG, "tg_search_apply_noise: null noise");
    Search* s = e->search;
    const uint8_t* d_active;
    rc = upload_mask(e, active, &d_active);
    if (rc) return rc;
    TG_HIP(hipMemcpyAsync(s->noise.p, noise, (size_t)s->d.G * EX_MOVES * 4, hipMemcpyHostToDevice, e->stream));
    launch_apply_noise(e->stream, s->d, d_active, s->aux.noise, ratio);
    TG_HIP(hipGetLastError());
    return sync_and_check(e);
}

int tg_search_root(TgEngine* e, TgMove* moves, uint32_t* visits, float* prior, float* q, int32_t* counts, uint32_t* root_visits,
                   float* root_q) {
    int rc = need_search(e);
    if (rc) return rc;
    Search* s = e->search;
    const SearchAux& x = s->aux;
    const size_t G = (size_t)s->d.G, R = G * EX_MOVES;
    TG_HIP(hipMemsetAsync(x.r_moves, 0, R * sizeof *x.r_moves, e->stream));
    TG_HIP(hipMemsetAsync(x.r_visits, 0, R * sizeof *x.r_visits, e->stream));
    TG_HIP(hipMemsetAsync(x.r_prior, 0, R * sizeof *x.r_prior, e->stream));
    TG_HIP(hipMemsetAsync(x.r_q, 0, R * sizeof *x.r_q, e->stream));
    launch_root_stats(e->stream, s->d, x.r_moves, x.r_visits, x.r_prior, x.r_q, x.r_counts, x.r_rv, x.r_rq);
    TG_HIP(hipGetLastError());
    rc = sync_and_check(e);
    if (rc) return rc;
    TG_HIP(copy_out(moves, x.r_moves, R));
    TG_HIP(copy_out(visits, x.r_visits, R));
    TG_HIP(copy_out(prior, x.r_prior, R));
    TG_HIP(copy_out(q, x.r_q, R));
    TG_HIP(copy_out(counts, x.r_counts, G));
    TG_HIP(copy_out(root_visits, x.r_rv, G));
    TG_HIP(copy_out(root_q, x.r_rq, G));
    return TG_OK;
}

int tg_search_debug(TgEngine* e, int depth, int top_k, TgMove* moves, uint32_t* visits, float* reward, float* policy, int32_t* counts,
                    float* eval, TgMove* cont_moves, uint32_t* cont_visits, int32_t* cont_len) {
    int rc = need_search(e);
    if (rc) return rc;
    if (depth < 0 || depth > TG_DEBUG_MAX_DEPTH || top_k < 0 || top_k > TG_MAX_MOVES)
        return fail(TG_ERR_INVALID_ARG, "tg_search_debug: need 0 <= depth <= TG_DEBUG_MAX_DEPTH and 0 <= top_k <= TG_MAX_MOVES");
    Search* s = e->search;
    rc = sync_and_check(e);
    if (rc) return rc;
    const size_t G = (size_t)s->d.G;
    // no continuation output wanted → walk none
    const size_t K = (cont_moves || cont_visits || cont_len) ? (size_t)top_k : 0, D = (size_t)depth;
    // the device scratch of one slice of games stays within TG_DEBUG_SCRATCH_BYTES (≤ 200 KB per game: at least 300 games a slice)
    const size_t per_game = EX_MOVES * (2 + 4 + 4 + 4) + 4 + 4 + K * D * (2 + 4) + K * 4;
    const size_t slice = std::max<size_t>(1, std::min<size_t>(G, (size_t)TG_DEBUG_SCRATCH_BYTES / per_game));
    DebugOut o{};
    TG_HIP(bind(s->dbg_moves, o.moves, slice * EX_MOVES));
    TG_HIP(bind(s->dbg_visits, o.visits, slice * EX_MOVES));
    TG_HIP(bind(s->dbg_reward, o.reward, slice * EX_MOVES));
    TG_HIP(bind(s->dbg_policy, o.policy, slice * EX_MOVES));
    TG_HIP(bind(s->dbg_counts, o.counts, slice));
    TG_HIP(bind(s->dbg_eval, o.eval, slice));
    TG_HIP(bind(s->dbg_cmoves, o.cont_moves, std::max<size_t>(1, slice * K * D)));  // (never an empty allocation)
    TG_HIP(bind(s->dbg_cvisits, o.cont_visits, std::max<size_t>(1, slice * K * D)));
    TG_HIP(bind(s->dbg_clen, o.cont_len, std::max<size_t>(1, slice * K)));
    for (size_t g0 = 0; g0 < G; g0 += slice) {
        const size_t ns = std::min(slice, G - g0);
        launch_search_debug(e->stream, s->d, (int)g0, (int)ns, depth, (int)K, o);
        TG_HIP(hipGetLastError());
        TG_HIP(hipStreamSynchronize(e->stream));
        const size_t R = g0 * EX_MOVES, C = g0 * K * D;
        TG_HIP(copy_out(moves ? moves + R : nullptr, o.moves, ns * EX_MOVES));
        TG_HIP(copy_out(visits ? visits + R : nullptr, o.visits, ns * EX_MOVES));
        TG_HIP(copy_out(reward ? reward + R : nullptr, o.reward, ns * EX_MOVES));
        TG_HIP(copy_out(policy ? policy + R : nullptr, o.policy, ns * EX_MOVES));
        TG_HIP(copy_out(counts ? counts + g0 : nullptr, o.counts, ns));
        TG_HIP(copy_out(eval ? eval + g0 : nullptr, o.eval, ns));
        TG_HIP(copy_out(cont_moves ? cont_moves + C : nullptr, o.cont_moves, ns * K * D));
        TG_HIP(copy_out(cont_visits ? cont_visits + C : nullptr, o.cont_visits, ns * K * D));
        TG_HIP(copy_out(cont_len ? cont_len + g0 * K : nullptr, o.cont_len, ns * K));
    }
    return TG_OK;
}

int tg_search_play(TgEngine* e, const TgMove* moves, const uint8_t* active) {
    int rc = need_search(e);
    if (rc) return rc;
    if (!moves) return fail(TG_ERR_INVALID_ARG, "tg_search_play: null moves");
    Search* s = e->search;
    const uint8_t* d_active;
    rc = upload_mask(e, active, &d_active);
    if (rc) return rc;
    TG_HIP(hipMemcpyAsync(s->s_moves.p, moves, (size_t)s->d.G * 2, hipMemcpyHostToDevice, e->stream));
    launch_play_move(e->stream, s->d, s->aux.s_moves, d_active, s->aux.op);
    launch_reroot(e->stream, s->d, s->aux.op);
    TG_HIP(hipGetLastError());
    return sync_and_check(e);
}

int tg_search_states(TgEngine* e, void* states) {
    int rc = need_search(e);
    if (rc) return rc;
    if (!states) return fail(TG_ERR_INVALID_ARG, "tg_search_states: null states");
    rc = sync_and_check(e);
    if (rc) return rc;
    TG_HIP(hipMemcpy(states, e->search->root_state.p, (size_t)e->search->d.G * e->g.bytes, hipMemcpyDeviceToHost));
    return TG_OK;
}

int tg_search_dump(TgEngine* e, int game, TgNodeRecord* records, size_t capacity, size_t* n_records) {
    int rc = need_search(e);
    if (rc) return rc;
    Search* s = e->search;
    if (game < 0 || game >= s->d.G || !n_records) return fail(TG_ERR_INVALID_ARG, "tg_search_dump: bad arguments");
    rc = sync_and_check(e);
    if (rc) return rc;
    // gather the game's chunks (its chain through chunk_link) and index the tree by pool index
    uint32_t root = 0, head = 0;
    TG_HIP(hipMemcpy(&root, s->d.root + game, 4, hipMemcpyDeviceToHost));
    TG_HIP(hipMemcpy(&head, s->d.chunk_head + game, 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> link(s->d.n_chunks);
    TG_HIP(hipMemcpy(link.data(), s->chunk_link.p, (size_t)s->d.n_chunks * 4, hipMemcpyDeviceToHost));
    const int sh = s->d.chunk_shift;
    const size_t CH = (size_t)1 << sh;
    std::map<uint32_t, size_t> where;  // chunk id → position in the host copies
    std::vector<NodeHot> hot_h;
    std::vector<NodeCold> cold_h;
    for (uint32_t c = head; c != 0; c = link[c]) {
        if (c >= s->d.n_chunks || where.count(c)) return fail(TG_ERR_STATE, "tg_search_dump: corrupt chunk chain");
        where[c] = hot_h.size();
        hot_h.resize(hot_h.size() + CH);
        cold_h.resize(cold_h.size() + CH);
        TG_HIP(hipMemcpy(hot_h.data() + where[c], s->d.hot + ((size_t)c << sh), CH * sizeof(NodeHot), hipMemcpyDeviceToHost));
        TG_HIP(hipMemcpy(cold_h.data() + where[c], s->d.cold + ((size_t)c << sh), CH * sizeof(NodeCold), hipMemcpyDeviceToHost));
    }
    bool corrupt = false;
    auto at = [&](uint32_t nd) -> size_t {
        auto it = where.find(nd >> sh);
        if (it == where.end()) { corrupt = true; return 0; }
        return it->second + (nd & (CH - 1));
    };
    if (where.empty()) return fail(TG_ERR_STATE, "tg_search_dump: the game has no tree");
    // depth-first in child order; uninitialised children become leaf records with n_children = 0xFFFF
    std::vector<TgNodeRecord> out;
    struct Frame { uint32_t node; uint32_t next; };
    std::vector<Frame> stack;
    auto emit = [&](uint32_t nd, bool is_root) {
        const NodeHot& h = hot_h[at(nd)];
        const NodeCold& c = cold_h[at(nd)];
        TgNodeRecord r;
        r.move = is_root ? 0 : c.mv;
        r.n_children = (uint16_t)(c.nres & 0xfff);
        r.visits = h.visits;
        r.virtual_visits = h.virt;
        r.result = c.nres >> 12;
        std::memcpy(&r.prior_bits, &h.prior, 4);
        std::memcpy(&r.q_bits, &h.q, 4);
        out.push_back(r);
    };
    emit(root, true);
    stack.push_back({root, 0u});
    while (!stack.empty() && !corrupt) {
        Frame& f = stack.back();
        const NodeCold& fc = cold_h[at(f.node)];
        uint32_t nch = fc.nres & 0xfff;
        if (f.next >= nch) { stack.pop_back(); continue; }
        uint32_t c = fc.child + f.next;
        f.next++;
        const NodeHot& ch = hot_h[at(c)];
        if (corrupt) break;
        if (ch.visits != 0 || ch.virt != 0) {
            emit(c, false);
            stack.push_back({c, 0u});
        } else {
            TgNodeRecord r;
            r.move = cold_h[at(c)].mv;
            r.n_children = 0xFFFF;
            r.visits = 0; r.virtual_visits = 0; r.result = 0;
            std::memcpy(&r.prior_bits, &ch.prior, 4);
            std::memcpy(&r.q_bits, &ch.q, 4);
            out.push_back(r);
        }
    }
    if (corrupt) return fail(TG_ERR_STATE, "tg_search_dump: corrupt tree (a child index points outside the game's chunks)");
    *n_records = out.size();
    if (out.size() > capacity || (!records && !out.empty())) return fail(TG_ERR_INVALID_ARG, "tg_search_dump: capacity too small");
    std::memcpy(records, out.data(), out.size() * sizeof(TgNodeRecord));
    return TG_OK;
}

int tg_search_counters(TgEngine* e, uint64_t* expansions, uint64_t* evals) {
    int rc = need_search(e);
    if (rc) return rc;
    rc = sync_and_check(e);
    if (rc) return rc;
    unsigned long long c[2];
    rc = read_counters(e, &c[0], &c[1]);
    if (rc) return rc;
    if (expansions) *expansions = c[0];
    if (evals) *evals = c[1];
    return TG_OK;
}

int tg_search_set_proof(TgEngine* e, int mode) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_search_set_proof: null engine");
    int rc = need_search(e);
    if (rc) return rc;
    if (mode != TG_PROOF_OFF && mode != TG_PROOF_ON) return fail(TG_ERR_INVALID_ARG, "tg_search_set_proof: unknown mode");
    // the rollouts of the off mode know the TgResult codes alone: they would back a proven node up as a draw
    if (mode == TG_PROOF_OFF && e->search->proof != TG_PROOF_OFF && e->search->proof_ran)
        return fail(TG_ERR_STATE, "tg_search_set_proof: iterations have run under TG_PROOF_ON since the last tg_search_reset, the trees may hold "
                                  "proven nodes; TG_PROOF_OFF is accepted in front of the first iteration after a tg_search_reset or a create");
    e->search->proof = mode;
    return TG_OK;
}

int tg_search_get_proof(TgEngine* e, int* mode, uint64_t* nodes_proven, uint64_t* rollouts_ended_on_proven) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_search_get_proof: null engine");
    int rc = need_search(e);
    if (rc) return rc;
    rc = sync_and_check(e);
    if (rc) return rc;
    Search* s = e->search;
    const size_t G = (size_t)s->d.G;
    std::vector<unsigned long long> h(G * 2);
    TG_HIP(hipMemcpy(h.data(), s->d.counters + G * 2, h.size() * 8, hipMemcpyDeviceToHost));
    unsigned long long a = 0, b = 0;
    for (size_t g = 0; g < G; g++) { a += h[2 * g]; b += h[2 * g + 1]; }
    if (mode) *mode = s->proof;
    if (nodes_proven) *nodes_proven = a;
    if (rollouts_ended_on_proven) *rollouts_ended_on_proven = b;
    return TG_OK;
}

int tg_search_proof(TgEngine* e, uint8_t* root_status, uint8_t* child_status, int32_t* counts) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "tg_search_proof: null engine");
    int rc = need_search(e);
    if (rc) return rc;
    Search* s = e->search;
    const size_t G = (size_t)s->d.G;
    uint8_t *d_root, *d_child;
    int32_t* d_counts;
    TG_HIP(bind(s->p_root, d_root, G));
    TG_HIP(bind(s->p_child, d_child, G * EX_MOVES));
    TG_HIP(bind(s->p_counts, d_counts, G));
    launch_proof_read(e->stream, s->d, d_root, d_child, d_counts);
    TG_HIP(hipGetLastError());
    rc = sync_and_check(e);
    if (rc) return rc;
    TG_HIP(copy_out(root_status, d_root, G));
    TG_HIP(copy_out(child_status, d_child, G * EX_MOVES));
    TG_HIP(copy_out(counts, d_counts, G));
    return TG_OK;
}

int tg_search_pool(TgEngine* e, uint64_t* nodes_total, uint64_t* nodes_in_use, uint64_t* nodes_peak) {
    int rc = need_search(e);
    if (rc) return rc;
    rc = sync_and_check(e);
    if (rc) return rc;
    Search* s = e->search;
    unsigned long long ctl[4];
    TG_HIP(hipMemcpy(ctl, s->pool_ctl.p, sizeof ctl, hipMemcpyDeviceToHost));
    // chunks handed out so far minus chunks returned beyond the initial fill of the ring = chunks owned by trees
    const unsigned long long initial = (unsigned long long)s->d.n_chunks - 1;
    const unsigned long long owned = ctl[0] - (ctl[1] - initial);
    if (nodes_total) *nodes_total = (uint64_t)initial << s->d.chunk_shift;
    if (nodes_in_use) *nodes_in_use = (uint64_t)owned << s->d.chunk_shift;
    if (nodes_peak) *nodes_peak = (uint64_t)ctl[3] << s->d.chunk_shift;
    return TG_OK;
}
}  // extern "C"
