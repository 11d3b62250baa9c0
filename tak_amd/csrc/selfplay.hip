// selfplay.hip — host side of the tg_selfplay_* entry points of include/takgpu.h: the per-ply schedule of self_play_parallel
// around the search's iteration driver (search.hip), the rollout schedule, statistics and the drain of the example ring.
#include <algorithm>
#include <cstring>

#include "search_host.h"
#include "window.h"

using namespace tg;

// the guard of every entry point behind tg_selfplay_create
static int need_selfplay(TgEngine* e, const char* who = nullptr) {
    if (int rc = need_search(e)) return rc;
    if (!e->search->selfplay) return fail(TG_ERR_STATE, (who ? std::string(who) + ": " : std::string()) + "tg_selfplay_create has not been called");
    return TG_OK;
}

extern "C" {

int tg_selfplay_create(TgEngine* e, const TgSearchConfig* scfg, const TgSelfPlayConfig* cfg) {
    if (!cfg || !scfg) return fail(TG_ERR_INVALID_ARG, "null self-play config");
    if (cfg->rollouts < 1 || cfg->max_examples < 1) return fail(TG_ERR_INVALID_ARG, "rollouts and max_examples must be positive");
    if (cfg->max_game_plies < 0 || cfg->max_game_plies > TG_LIMIT_GAME_PLIES)
        return fail(TG_ERR_INVALID_ARG, "max_game_plies must be 0 (= TG_LIMIT_GAME_PLIES) or in 1..TG_LIMIT_GAME_PLIES");
    // virtual rollouts per game and iteration: TgSelfPlayConfig.batch (0 = 1: self_play_parallel's one leaf per game,
    // self_play.rs:181-210; > 1: Player's batching as train/src/self_play.rs:21-92 uses it).  TgSearchConfig.batch is ignored.
    if (cfg->batch < 0) return fail(TG_ERR_INVALID_ARG, "TgSelfPlayConfig.batch must be in 0..4096 (0 = 1)");
    if (cfg->batch > 4096) return fail(TG_ERR_INVALID_ARG, "TgSelfPlayConfig.batch must be at most 4096 virtual rollouts per game and iteration");
    const int B = cfg->batch ? cfg->batch : 1;
    if (e && scfg->games > 0 && e->cfg.evaluator == TG_EVAL_RESNET && (long long)scfg->games * B > (long long)e->cfg.max_batch)
        return fail(TG_ERR_INVALID_ARG, "games x batch = " + std::to_string((long long)scfg->games * B) +
                                            " leaves per iteration exceed max_batch = " + std::to_string(e->cfg.max_batch));
    TgSearchConfig sc1 = *scfg;
    sc1.batch = (uint32_t)B;
    int rc = search_alloc(e, &sc1, (size_t)B);
    if (rc) return rc;
    Search* s = e->search;
    s->selfplay = true;
    s->spcfg = *cfg;
    s->d.retire = 1;
    const size_t G = (size_t)s->d.G, sb = (size_t)e->g.bytes;
    const int epg = TG_LIMIT_GAME_PLIES;
    const size_t ME = (size_t)cfg->max_examples;
    SelfPlayDev& p = s->p;
    TG_HIP(bind(s->st_hdr, p.st_hdr, G * epg));
    TG_HIP(bind(s->st_state, p.st_state, G * epg * sb));
    TG_HIP(bind(s->st_moves, p.st_moves, G * epg * EX_MOVES));
    TG_HIP(bind(s->st_visits, p.st_visits, G * epg * EX_MOVES));
    TG_HIP(bind(s->st_count, p.st_count, G));
    TG_HIP(bind(s->out_hdr, p.out_hdr, ME));
    TG_HIP(bind(s->out_state, p.out_state, ME * sb));
    TG_HIP(bind(s->out_moves, p.out_moves, ME * EX_MOVES));
    TG_HIP(bind(s->out_visits, p.out_visits, ME * EX_MOVES));
    TG_HIP(bind(s->fin, p.fin, G));
    TG_HIP(bind(s->recycle, p.recycle, G));
    TG_HIP(bind(s->out_off, p.out_off, G));
    TG_HIP(bind(s->chosen, p.chosen, G));
    TG_HIP(bind(s->mask, p.mask, G));
    TG_HIP(bind(s->stats, p.stats, ST_COUNT));
    TG_HIP(hipMemsetAsync(s->st_count.p, 0, G * 4, e->stream));
    TG_HIP(hipMemsetAsync(s->stats.p, 0, ST_COUNT * 8, e->stream));
    TG_HIP(hipMemsetAsync(s->fin.p, 0, G, e->stream));
    TG_HIP(bind(s->boost_list, s->aux.boost_list, G));
    TG_HIP(bind(s->boost_count, s->aux.boost_count, 1));
    TG_HIP(hipHostMalloc((void**)&s->h_boost_count, 4, hipHostMallocDefault));
    *s->h_boost_count = 0;
    p.ex_per_game = epg; p.max_examples = cfg->max_examples;
    p.max_game_plies = cfg->max_game_plies ? cfg->max_game_plies : epg;
    p.rollouts = cfg->rollouts; p.noise_plies = cfg->noise_plies; p.exploit_plies = cfg->exploit_plies; p.komi = cfg->komi;
    p.total_games = cfg->total_games; p.noise_alpha = cfg->noise_alpha; p.noise_ratio = cfg->noise_ratio;
    // games[i] = Game::with_komi(komi), nodes[i] = Node::default()  (self_play.rs:102-103)
    std::vector<uint8_t> start(sb, 0);
    {
        int stones, caps;
        starting_stones(e->g.n, stones, caps);
        TgHeader* h = (TgHeader*)(start.data() + sb - sizeof(TgHeader));
        h->n = (uint8_t)e->g.n; h->to_move = 0; h->ply = 0;
        h->white_stones = h->black_stones = (uint8_t)stones;
        h->white_caps = h->black_caps = (uint8_t)caps;
        h->half_komi = (int8_t)(cfg->komi * 2); h->reversible_plies = 0;
    }
    std::vector<uint8_t> all(G * sb);
    for (size_t g = 0; g < G; g++) std::memcpy(&all[g * sb], start.data(), sb);
    TG_HIP(hipMemcpy(s->root_state.p, all.data(), all.size(), hipMemcpyHostToDevice));
    TG_HIP(hipMemsetAsync(s->alive.p, 1, G, e->stream));
    return search_reset_trees(e);
}

int tg_selfplay_set_schedule(TgEngine* e, const TgRolloutSchedule* sc) {
    int rc = need_selfplay(e, "tg_selfplay_set_schedule");
    if (rc) return rc;
    Search* s = e->search;
    if (s->stepped) return fail(TG_ERR_STATE, "tg_selfplay_set_schedule: the schedule is fixed once tg_selfplay_step has run");
    if (!sc) return fail(TG_ERR_INVALID_ARG, "tg_selfplay_set_schedule: null schedule");
    if (sc->boost_plies < 0 || sc->boost_plies > TG_LIMIT_GAME_PLIES)
        return fail(TG_ERR_INVALID_ARG, "TgRolloutSchedule.boost_plies must be in 0..TG_LIMIT_GAME_PLIES");
    if (sc->boost_factor < 1 || sc->boost_factor > 64) return fail(TG_ERR_INVALID_ARG, "TgRolloutSchedule.boost_factor must be in 1..64");
    if (sc->reserved[0] != 0 || sc->reserved[1] != 0) return fail(TG_ERR_INVALID_ARG, "TgRolloutSchedule.reserved must be 0");
    if ((long long)s->spcfg.rollouts * sc->boost_factor > 2147483647ll)
        return fail(TG_ERR_INVALID_ARG, "TgSelfPlayConfig.rollouts x TgRolloutSchedule.boost_factor = " +
                                            std::to_string((long long)s->spcfg.rollouts * sc->boost_factor) + " does not fit an int32");
    s->sched = *sc;
    return TG_OK;
}

int tg_selfplay_schedule_stats(TgEngine* e, uint64_t* boosted_moves, uint64_t* compact_iterations, uint64_t* compact_leaves) {
    int rc = need_selfplay(e, "tg_selfplay_schedule_stats");
    if (rc) return rc;
    Search* s = e->search;
    rc = sync_and_check(e);
    if (rc) return rc;
    if (boosted_moves) *boosted_moves = s->boosted_moves;
    if (compact_iterations) *compact_iterations = s->compact_iterations;
    if (compact_leaves) *compact_leaves = s->compact_leaves;
    return TG_OK;
}

int tg_selfplay_step(TgEngine* e, int plies) {
    int rc = need_selfplay(e);
    if (rc) return rc;
    Search* s = e->search;
    hipStream_t st = e->stream;
    const size_t G = (size_t)s->d.G;
    int32_t* op = s->aux.op;
    if (plies > 0) s->stepped = true;
    const bool boost = s->sched.boost_plies > 0 && s->sched.boost_factor > 1;
    for (int ply = 0; ply < plies; ply++) {
        launch_sp_opening(st, s->d);                                   // (a) :110-116
        launch_sp_instant_win(st, s->d, s->p);                         // (b) :119-171
        TG_HIP(hipMemsetAsync(op, 0xFF, G * 4, st));
        launch_sp_finish(st, s->d, s->p, op);
        launch_reroot(st, s->d, op);
        launch_sp_noise_mask(st, s->d, s->p);                          // (c) :174-180
        rc = search_iterate(e, 1, s->p.mask);
        if (rc) return rc;
        launch_dirichlet(st, s->d, s->p.mask, s->p.noise_alpha, s->p.noise_ratio);
        rc = search_iterate(e, s->p.rollouts);                         // (d) :181-210
        if (rc) return rc;
        if (boost) {
            // train/src/self_play.rs:19,63: boost_factor × rollouts while game.ply < boost_plies.  The extra iterations run over
            // the games that are owed them only; their number sizes the grid and the network batch, hence the one wait per ply
            launch_sp_boost_list(st, s->d, s->sched.boost_plies, s->aux.boost_list, s->aux.boost_count);
            TG_HIP(hipGetLastError());
            TG_HIP(hipMemcpyAsync(s->h_boost_count, s->aux.boost_count, 4, hipMemcpyDeviceToHost, st));
            TG_HIP(hipStreamSynchronize(st));
            const int count = *s->h_boost_count;
            if (count < 0 || count > s->d.G) return fail(TG_ERR_STATE, "tg_selfplay_step: corrupt boost list");
            const int extra = (s->sched.boost_factor - 1) * s->p.rollouts;
            s->boosted_moves += (unsigned long long)count;
            if (count == s->d.G) rc = search_iterate(e, extra);
            else if (count > 0) {
                rc = search_iterate(e, extra, nullptr, s->aux.boost_list, count);
                s->compact_iterations += (unsigned long long)extra;
                s->compact_leaves += (unsigned long long)extra * (unsigned long long)count * (unsigned long long)s->d.batch;
            }
            if (rc) return rc;
        }
        launch_sp_pick(st, s->d, s->p, op, s->proof != 0);             // (e) :212-258; TG_PROOF_ON: the proof-aware pick (takgpu.h)
        launch_sp_finish(st, s->d, s->p, op);
        launch_reroot(st, s->d, op);
        launch_sp_count_ply(st, s->p);
        TG_HIP(hipGetLastError());
    }
    return TG_OK;
}

int tg_selfplay_stats(TgEngine* e, TgSelfPlayStats* out) {
    int rc = need_selfplay(e);
    if (rc) return rc;
    Search* s = e->search;
    if (!out) return fail(TG_ERR_STATE, "tg_selfplay_create has not been called");
    rc = sync_and_check(e);
    if (rc) return rc;
    unsigned long long st[ST_COUNT], c[2];
    TG_HIP(hipMemcpy(st, s->stats.p, sizeof st, hipMemcpyDeviceToHost));
    rc = read_counters(e, &c[0], &c[1]);
    if (rc) return rc;
    out->games_finished = st[ST_FINISHED]; out->examples = st[ST_EXAMPLES]; out->plies = st[ST_PLIES];
    out->white_wins = st[ST_WHITE]; out->black_wins = st[ST_BLACK]; out->draws = st[ST_DRAWS]; out->instant_wins = st[ST_INSTANT];
    out->expansions = c[0]; out->evals = c[1];
    out->aborted_games = st[ST_ABORTED];
    {
        std::vector<uint8_t> alive((size_t)s->d.G);
        TG_HIP(hipMemcpy(alive.data(), s->alive.p, alive.size(), hipMemcpyDeviceToHost));
        out->alive_games = 0;
        for (uint8_t a : alive) out->alive_games += a ? 1u : 0u;
    }
    {   // examples the ring has overwritten since the last drain count as dropped as soon as they are observable
        const unsigned long long ME = (unsigned long long)s->p.max_examples;
        unsigned long long lost = st[ST_EXAMPLES] - s->drained > ME ? st[ST_EXAMPLES] - s->drained - ME : 0ull;
        out->dropped_examples = s->dropped + lost;
    }
    return TG_OK;
}

int tg_selfplay_drain(TgEngine* e, int cap, TgExampleHeader* headers, void* states, TgMove* moves, uint32_t* visits, int32_t* n_out) {
    int rc = need_selfplay(e);
    if (rc) return rc;
    Search* s = e->search;
    if (cap < 0 || !n_out || (cap > 0 && (!headers || !states || !moves || !visits))) return fail(TG_ERR_INVALID_ARG, "tg_selfplay_drain: bad arguments");
    rc = sync_and_check(e);
    if (rc) return rc;
    unsigned long long total = 0;
    TG_HIP(hipMemcpy(&total, s->p.stats + ST_EXAMPLES, 8, hipMemcpyDeviceToHost));
    const unsigned long long ME = (unsigned long long)s->p.max_examples;
    if (total - s->drained > ME) {  // older ones were overwritten in the ring: skipped, and counted
        s->dropped += total - ME - s->drained;
        s->drained = total - ME;
    }
    const size_t sb = (size_t)e->g.bytes;
    const unsigned long long avail = total - s->drained;
    const int k = (int)std::min<unsigned long long>((unsigned long long)cap, avail);
    // the k examples are consecutive ring entries: at most two contiguous runs per array (wrap-around, window.h), one copy each
    std::vector<ExampleRec> hdr((size_t)k);
    const RingRuns runs = ring_runs(s->drained, (uint64_t)k, ME);
    for (int r = 0; r < runs.count; r++) {
        const size_t o = (size_t)runs.start[r], done = (size_t)runs.at[r], run = (size_t)runs.len[r];
        TG_HIP(hipMemcpy(hdr.data() + done, s->p.out_hdr + o, run * sizeof(ExampleRec), hipMemcpyDeviceToHost));
        TG_HIP(hipMemcpy((uint8_t*)states + done * sb, s->p.out_state + o * sb, run * sb, hipMemcpyDeviceToHost));
        TG_HIP(hipMemcpy(moves + done * EX_MOVES, s->p.out_moves + o * EX_MOVES, run * EX_MOVES * 2, hipMemcpyDeviceToHost));
        TG_HIP(hipMemcpy(visits + done * EX_MOVES, s->p.out_visits + o * EX_MOVES, run * EX_MOVES * 4, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < k; i++) {
        headers[i].game_id = hdr[i].slot | (hdr[i].generation << 20);
        headers[i].n_moves = hdr[i].n_moves;
        headers[i].result = hdr[i].result;
        headers[i].reserved = 0;
        // entries past n_moves are whatever an earlier example left in the ring slot: clear them for the caller
        const size_t nm = (size_t)std::min(std::max(hdr[i].n_moves, 0), (int32_t)EX_MOVES);
        std::memset(moves + (size_t)i * EX_MOVES + nm, 0, (EX_MOVES - nm) * 2);
        std::memset(visits + (size_t)i * EX_MOVES + nm, 0, (EX_MOVES - nm) * 4);
    }
    s->drained += (unsigned long long)k;
    *n_out = k;
    return TG_OK;
}

}  // extern "C"
