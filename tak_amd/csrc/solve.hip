// solve.hip — host side of the forced-win solver (include/takgpu.h: tg_solve, tg_search_solve; kernels in solve_kernels.hip).
// The positions run in chunks of SOLVE_CHUNK: per chunk one root launch, one scan, ONE host wait (the item total sizes the
// level grids), then a level launch and a fold per level with no host wait between them.
#include "solve.h"

#include <algorithm>
#include <cstring>

#include "search_host.h"

namespace tg {

constexpr int SOLVE_CHUNK = 4096;  // positions per chunk: ≤ 2^21 work items, 5 MB of move table

struct Solver {
    DevBuf states, active, counts, offsets, moves, move_values, value, best, decided, budget_hit, nodes, item_nodes, item_flag;
};
void solver_destroy(Solver* s) { delete s; }

static int check_config(const TgSolveConfig* cfg, const char* who, uint32_t* budget) {
    const std::string w(who);
    if (!cfg) return fail(TG_ERR_INVALID_ARG, w + ": null cfg");
    if (cfg->depth < 1 || cfg->depth > TG_SOLVE_MAX_DEPTH) return fail(TG_ERR_INVALID_ARG, w + ": depth must be 1 .. TG_SOLVE_MAX_DEPTH (6)");
    if (cfg->flags & ~(TG_SOLVE_ALL_MOVES | TG_SOLVE_ROAD_ONLY)) return fail(TG_ERR_INVALID_ARG, w + ": unknown bits in flags");
    for (int i = 0; i < 4; i++)
        if (cfg->reserved[i]) return fail(TG_ERR_INVALID_ARG, w + ": reserved must be 0");
    const uint64_t b = cfg->node_budget ? cfg->node_budget : (uint64_t)TG_SOLVE_DEFAULT_BUDGET;
    *budget = (uint32_t)std::min<uint64_t>(b, 0x7fffffffull);
    return TG_OK;
}

template <class T, class U>
static hipError_t copy_out(T* dst, const U* src, size_t n) {
    static_assert(sizeof(T) == sizeof(U), "host and device element differ");
    return dst && n ? hipMemcpy(dst, src, n * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

struct SolveOut {
    int8_t* value; TgMove* best; int32_t* counts; TgMove* moves; int8_t* move_values; uint8_t* budget_hit; uint64_t* nodes;
};

// K ≤ SOLVE_CHUNK positions already on the device (d_states; d_active / d_alive optional) → the caller's arrays at row `row0`
static int solve_chunk(TgEngine* e, int K, const uint8_t* d_states, const uint8_t* d_active, const uint8_t* d_alive,
                       const TgSolveConfig& cfg, uint32_t budget, const SolveOut& o, size_t row0, const char* who) {
    Solver* s = e->solver;
    const size_t k = (size_t)K, R = k * TG_MAX_MOVES;
    const bool road = (cfg.flags & TG_SOLVE_ROAD_ONLY) != 0;
    SolveDev D{};
    D.states = d_states;
    D.active = d_active;
    D.alive = d_alive;
    D.K = K;
    D.n = e->g.n;
    D.all_moves = cfg.flags & TG_SOLVE_ALL_MOVES;
    D.budget = budget;
    TG_HIP(bind(s->counts, D.counts, k));
    TG_HIP(bind(s->offsets, D.offsets, k + 1));
    TG_HIP(bind(s->moves, D.moves, R));
    TG_HIP(bind(s->move_values, D.move_values, R));
    TG_HIP(bind(s->value, D.value, k));
    TG_HIP(bind(s->best, D.best, k));
    TG_HIP(bind(s->decided, D.decided, k));
    TG_HIP(bind(s->budget_hit, D.budget_hit, k));
    TG_HIP(bind(s->nodes, D.nodes, k));
    TG_HIP(hipMemsetAsync(D.moves, 0, R * sizeof *D.moves, e->stream));
    TG_HIP(hipMemsetAsync(D.move_values, 0, R * sizeof *D.move_values, e->stream));
    launch_solve_root(e->stream, D);
    launch_solve_scan(e->stream, D);
    TG_HIP(hipGetLastError());
    int32_t items = 0;
    std::vector<int32_t> h_counts(k);
    TG_HIP(hipMemcpyAsync(&items, D.offsets + K, sizeof items, hipMemcpyDeviceToHost, e->stream));
    TG_HIP(hipMemcpyAsync(h_counts.data(), D.counts, k * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
    TG_HIP(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < k; i++)  // a root above the capacity is refused before anything is searched (roots inside the tree: takgpu.h)
        if (h_counts[i] > TG_MAX_MOVES)
            return fail(TG_ERR_INVALID_ARG, std::string(who) + ": position " + std::to_string(row0 + i) + " has more than TG_MAX_MOVES moves");
    if (items < 0 || (size_t)items > R) return fail(TG_ERR_STATE, std::string(who) + ": corrupt item count");
    if (items > 0) {
        TG_HIP(bind(s->item_nodes, D.item_nodes, (size_t)items));
        TG_HIP(bind(s->item_flag, D.item_flag, (size_t)items));
        TG_HIP(hipMemsetAsync(D.item_nodes, 0, (size_t)items * sizeof *D.item_nodes, e->stream));
        TG_HIP(hipMemsetAsync(D.item_flag, 0, (size_t)items, e->stream));
        for (int level = 1; level <= cfg.depth; level++) {
            launch_solve_level(e->stream, D, road, level, items);
            launch_solve_fold(e->stream, D);
        }
        TG_HIP(hipGetLastError());
    }
    TG_HIP(hipStreamSynchronize(e->stream));
    TG_HIP(copy_out(o.value ? o.value + row0 : nullptr, D.value, k));
    TG_HIP(copy_out(o.best ? o.best + row0 : nullptr, D.best, k));
    TG_HIP(copy_out(o.moves ? o.moves + row0 * TG_MAX_MOVES : nullptr, D.moves, R));
    TG_HIP(copy_out(o.move_values ? o.move_values + row0 * TG_MAX_MOVES : nullptr, D.move_values, R));
    TG_HIP(copy_out(o.budget_hit ? o.budget_hit + row0 : nullptr, D.budget_hit, k));
    TG_HIP(copy_out(o.nodes ? o.nodes + row0 : nullptr, D.nodes, k));
    if (o.counts) std::memcpy(o.counts + row0, h_counts.data(), k * sizeof(int32_t));
    return TG_OK;
}

static int ensure_solver(TgEngine* e) {
    if (!e->solver) e->solver = new Solver();
    return TG_OK;
}

}  // namespace tg

using namespace tg;

extern "C" {

int tg_solve(TgEngine* e, int n, const void* states, const TgSolveConfig* cfg, int8_t* value, TgMove* best, int32_t* counts,
             TgMove* moves, int8_t* move_values, uint8_t* budget_hit, uint64_t* nodes) {
    if (!e) return fail(TG_ERR_INVALID_ARG, "null engine");
    TG_HIP(hipSetDevice(e->cfg.device));
    uint32_t budget = 0;
    int rc = check_config(cfg, "tg_solve", &budget);
    if (rc) return rc;
    if (n < 0) return fail(TG_ERR_INVALID_ARG, "tg_solve: negative n");
    if (n > 0 && !states) return fail(TG_ERR_INVALID_ARG, "tg_solve: null states");
    if (n == 0) return TG_OK;
    rc = validate_states(e, n, (const uint8_t*)states, "tg_solve");
    if (rc) return rc;
    ensure_solver(e);
    const size_t sb = e->g.bytes;
    const SolveOut o{value, best, counts, moves, move_values, budget_hit, nodes};
    TG_HIP(e->solver->states.ensure((size_t)std::min(n, SOLVE_CHUNK) * sb));
    for (int off = 0; off < n; off += SOLVE_CHUNK) {
        const int k = std::min(SOLVE_CHUNK, n - off);
        TG_HIP(hipMemcpyAsync(e->solver->states.p, (const uint8_t*)states + (size_t)off * sb, (size_t)k * sb, hipMemcpyHostToDevice, e->stream));
        rc = solve_chunk(e, k, e->solver->states.as<uint8_t>(), nullptr, nullptr, *cfg, budget, o, (size_t)off, "tg_solve");
        if (rc) return rc;
    }
    return TG_OK;
}

int tg_search_solve(TgEngine* e, const TgSolveConfig* cfg, const uint8_t* active, int8_t* value, TgMove* best, int32_t* counts,
                    TgMove* moves, int8_t* move_values, uint8_t* budget_hit, uint64_t* nodes) {
    int rc = need_search(e);
    if (rc) return rc;
    uint32_t budget = 0;
    rc = check_config(cfg, "tg_search_solve", &budget);
    if (rc) return rc;
    rc = sync_and_check(e);  // a search that has raised an error flag has no roots to trust
    if (rc) return rc;
    ensure_solver(e);
    Search* s = e->search;
    const int G = s->d.G;
    const size_t sb = e->g.bytes;
    const uint8_t* d_active = nullptr;
    if (active) {
        TG_HIP(e->solver->active.ensure((size_t)G));
        TG_HIP(hipMemcpyAsync(e->solver->active.p, active, (size_t)G, hipMemcpyHostToDevice, e->stream));
        d_active = e->solver->active.as<uint8_t>();
    }
    const SolveOut o{value, best, counts, moves, move_values, budget_hit, nodes};
    for (int off = 0; off < G; off += SOLVE_CHUNK) {
        const int k = std::min(SOLVE_CHUNK, G - off);
        rc = solve_chunk(e, k, s->d.root_state + (size_t)off * sb, d_active ? d_active + off : nullptr, s->d.alive + off, *cfg, budget, o,
                         (size_t)off, "tg_search_solve");
        if (rc) return rc;
    }
    return TG_OK;
}

}  // extern "C"
