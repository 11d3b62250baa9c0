// search_proof_kernels.hip — the tree kernels with proven values (tg_search_set_proof(TG_PROOF_ON); the MCTS-solver backup of
// Winands et al., no counterpart in the reference): select_pass<.., PROOF = true> of tree_pass.cuh behind the same kernel bodies
// as search_kernels.hip (wave → game by identity) and search_list_kernels.hip (LIST: wave → game through a compacted list), the
// proof-aware pick of self-play, and the read-out of the roots' statuses.  A translation unit of its own: the code objects of
// the other two stay what they are without the mode.  backup_pass knows nothing of proofs: k_backup / k_backup_list serve both modes.
#undef TG_TREE_STAMPS  // the stamp buffer belongs to search_kernels.hip
#include "tree_pass.cuh"
#include "tree_launch.h"

namespace tg {

// wave w → (game, leaf-slot owner): identity, or entry w of the list (list[w] < S.G for every w < count ≤ S.G)
template <bool LIST>
__device__ __forceinline__ bool proof_wave_game(const SearchDev& S, const int32_t* __restrict__ list, int count, int& w, int& g) {
    w = game_of_wave();
    if (w >= (LIST ? count : S.G)) return false;
    g = LIST ? (int)uni((uint32_t)list[w]) : w;
    return true;
}

template <int NB, bool LIST>
__global__ __launch_bounds__(WPB * 64) void k_select_proof(SearchDev S, const uint8_t* __restrict__ active, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    int w, g;
    if (!proof_wave_game<LIST>(S, list, count, w, g)) return;
    uint32_t* path = path_lds[threadIdx.x >> 6];
    const int p0 = S.pass < 0 ? 0 : S.pass, p1 = S.pass < 0 ? S.batch : S.pass + 1;
    for (int p = p0; p < p1; p++) {
        select_pass<NB, LIST, true>(S, active, g, p, path, mv_lds[threadIdx.x >> 6], RootPre(), w);
        if (p + 1 < p1) wave_sync_mem();
    }
}

template <int NB, bool LIST>
__global__ __launch_bounds__(WPB * 64) void k_backup_select_proof(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    int w, g;
    if (!proof_wave_game<LIST>(S, list, count, w, g)) return;
    RootPre pre;
    const uint32_t root_v = S.root[g];
    const Geom geo = make_geom(NB ? NB : S.n);
    pre.raw = ws_load_raw(S.root_state + (size_t)g * geo.bytes, geo);
    pre.alive_v = (uint32_t)S.alive[g];
    pre.abort_v = (uint32_t)S.abort[g];
    pre.on = true;
    backup_pass<NB>(S, w, 0, root_v, &pre);
    wave_sync_mem();
    select_pass<NB, LIST, true>(S, nullptr, g, 0, path_lds[threadIdx.x >> 6], mv_lds[threadIdx.x >> 6], pre, w);
}

// (root hand-over between the passes: see k_backup_select_batch)
template <int NB, bool LIST>
__global__ __launch_bounds__(WPB * 64) void k_backup_select_batch_proof(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    int w, g;
    if (!proof_wave_game<LIST>(S, list, count, w, g)) return;
    RootPre pre;
    const uint32_t root_v = S.root[g];
    const Geom geo = make_geom(NB ? NB : S.n);
    pre.raw = ws_load_raw(S.root_state + (size_t)g * geo.bytes, geo);
    pre.alive_v = (uint32_t)S.alive[g];
    pre.abort_v = (uint32_t)S.abort[g];
    pre.on = true;
    const int B = S.batch;
    for (int p = 0; p < B; p++) {
        backup_pass<NB>(S, w, p, root_v, p + 1 == B ? &pre : nullptr);
        wave_sync_mem();
    }
    uint32_t* path = path_lds[threadIdx.x >> 6];
    uint16_t* mvl = mv_lds[threadIdx.x >> 6];
    for (int p = 0; p < B; p++) {
        select_pass<NB, LIST, true>(S, nullptr, g, p, path, mvl, pre, w);
        pre.on = false;
        if (p + 1 < B) wave_sync_mem();
    }
}

// tg_search_proof: the raw result nibble of every root and of its children, in possible_moves order; zero past the child count
__global__ __launch_bounds__(64) void k_proof_read(SearchDev S, uint8_t* __restrict__ root_status, uint8_t* __restrict__ child_status,
                                                   int32_t* __restrict__ counts) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const NodeCold rc = S.cold[S.root[g]];
    const uint32_t nchild = min((uint32_t)rc.nres & 0xfffu, (uint32_t)EX_MOVES), cb = rc.child;
    if (lane == 0) { root_status[g] = (uint8_t)(rc.nres >> 12); counts[g] = (int32_t)nchild; }
    for (uint32_t i = lane; i < (uint32_t)EX_MOVES; i += 64)
        child_status[(size_t)g * EX_MOVES + i] = i < nchild ? (uint8_t)(S.cold[cb + i].nres >> 12) : (uint8_t)0;
}

// (e) of self-play with the proof-aware pick: k_sp_pick (search_kernels.hip) with the candidates narrowed by the root children's
// statuses.  m = the root's colour to move.
//   1. some child decided for m: among those children the most visited, the LAST on ties — whatever the temperature
//   2. otherwise the candidates are the children not decided for the opponent (all children if that leaves none), and on them
//      pick_move (play.rs:49-67): exploit → most visited, last on ties; explore → the RNG_PICK draw over the visits with the
//      excluded children's visits taken as 0; candidates without a visit → exploit over the candidates (not ERRF_PICK)
// The example keeps the root's real visits.
__global__ __launch_bounds__(WPB * 64) void k_sp_pick_proof(SearchDev S, SelfPlayDev P, int32_t* __restrict__ op) {
    const int g = game_of_wave();
    if (g >= S.G) return;
    const int lane = lane_id();
    if (lane == 0) { P.fin[g] = 0; op[g] = -1; }
    if (!S.alive[g]) return;
    if (S.abort[g]) {  // the search of this ply ran into a capacity (depth, visits): retire the game
        if (lane == 0) P.fin[g] = FIN_ABORTED;
        return;
    }
    const Geom geo = make_geom(S.n);
    const NodeHot* hot = S.hot;
    const NodeCold* cold = S.cold;
    NodeCold rc = cold[S.root[g]];
    const uint32_t nchild = uni((uint32_t)rc.nres) & 0xfffu, cb = uni(rc.child);
    WState s;
    uint8_t* st = S.root_state + (size_t)g * geo.bytes;
    ws_load(s, st, geo);
    if (nchild == 0) { flag(S, ERRF_PICK); return; }
    const uint32_t m = s.to_move, opp = m ^ 1u;
    bool any_m = false, any_open = false;
    for (uint32_t i = lane; i < nchild; i += 64) {
        const uint32_t cs = proof_status((uint32_t)cold[cb + i].nres >> 12);
        any_m |= cs == m;
        any_open |= cs != opp;
    }
    const bool step1 = __ballot(any_m) != 0, narrow = __ballot(any_open) != 0;
    auto candidate = [&](uint32_t i) {
        const uint32_t cs = proof_status((uint32_t)cold[cb + i].nres >> 12);
        return step1 ? cs == m : narrow ? cs != opp : true;
    };
    unsigned long long total = 0;  // visits of the candidates
    for (uint32_t i = lane; i < nchild; i += 64) total += candidate(i) ? hot[cb + i].visits : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(total >> 32), d) << 32) |
                               (uint32_t)__shfl_xor((int)(uint32_t)total, d);
        total += o;
    }
    int pick = -1;
    if (step1 || total == 0 || (int)s.ply >= P.exploit_plies) {
        // max_by_key over the candidates: most visits, last on ties
        uint32_t bv = 0;
        int bi = -1;
        for (uint32_t i = lane; i < nchild; i += 64) {
            if (!candidate(i)) continue;
            uint32_t v = hot[cb + i].visits;
            if (bi < 0 || v >= bv) { bv = v; bi = (int)i; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            uint32_t ov = (uint32_t)__shfl_xor((int)bv, d);
            int oi = __shfl_xor(bi, d);
            if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi > bi))) { bv = ov; bi = oi; }
        }
        pick = bi;  // (≥ 0: there is always a candidate)
    } else {
        // WeightedIndex over the candidates' visits with one RNG_PICK draw
        U4 r = rng_draw(S.seed, S.slot_base + (uint32_t)g, S.generation[g], s.ply, RNG_PICK, 0, 0);
        unsigned long long x = ((unsigned long long)r.v[0] << 32) | r.v[1];
        unsigned long long target = __umul64hi(x, total);
        unsigned long long carry = 0;
        int last = -1;  // the last candidate with visits: where a draw that no prefix exceeds ends
        for (uint32_t i0 = 0; i0 < nchild; i0 += 64) {
            uint32_t i = i0 + lane;
            int v = (i < nchild && candidate(i)) ? (int)hot[cb + i].visits : 0;
            int incl = wave_inclusive_scan(v);
            uint64_t bb = __ballot(i < nchild && v > 0 && carry + (unsigned long long)incl > target);
            if (bb && pick < 0) pick = (int)i0 + __builtin_ctzll(bb);
            uint64_t nz = __ballot(v > 0);
            if (nz) last = (int)i0 + 63 - __builtin_clzll(nz);
            carry += (unsigned long long)__shfl(incl, 63);
        }
        if (pick < 0) pick = last;
    }
    if (pick < 0 || (uint32_t)pick >= nchild) { flag(S, ERRF_PICK); return; }  // (cannot happen; never index out of the block)
    // example = (game before the move, the REAL visit counts of every child)
    int slot;
    stage_example(S, P, g, s, geo, nchild, slot);
    if (slot < 0) {  // the game is past max_game_plies
        if (lane == 0) P.fin[g] = FIN_ABORTED;
        return;
    }
    {
        size_t e = (size_t)g * P.ex_per_game + slot;
        for (uint32_t i = lane; i < nchild && i < EX_MOVES; i += 64) {
            P.st_moves[e * EX_MOVES + i] = cold[cb + i].mv;
            P.st_visits[e * EX_MOVES + i] = hot[cb + i].visits;
        }
    }
    const uint32_t mv = uni((uint32_t)cold[cb + (uint32_t)pick].mv);
    ws_play(s, mv, geo);
    ws_store(s, st, geo);
    const uint32_t res = ws_result(s, geo);
    if (lane == 0) {
        P.fin[g] = (uint8_t)res;
        op[g] = pick;
        P.chosen[g] = pick;
    }
}

// ---- launchers --------------------------------------------------------------------------------
// list = null: wave → game by identity over S.G games (and the caller's mask); else over the compacted list of `count` games
#define TG_BY_BOARD_LIST(KERNEL, ...)                                            \
    do {                                                                         \
        if (list) TG_BY_BOARD_2(KERNEL, true, count, __VA_ARGS__);               \
        else TG_BY_BOARD_2(KERNEL, false, S.G, __VA_ARGS__);                     \
    } while (0)
#define TG_BY_BOARD_2(KERNEL, LIST, WAVES, ...)                                                                     \
    do {                                                                                                            \
        if (S.n == 5) hipLaunchKernelGGL((KERNEL<5, LIST>), wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__);      \
        else if (S.n == 6) hipLaunchKernelGGL((KERNEL<6, LIST>), wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<0, LIST>), wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__);               \
    } while (0)

void launch_select_proof(hipStream_t st, const SearchDev& S, const uint8_t* active, const int32_t* list, int count) {
    TG_BY_BOARD_LIST(k_select_proof, S, active, list, count);
}
void launch_backup_select_proof(hipStream_t st, const SearchDev& S, const int32_t* list, int count) {
    if (S.batch > 1) TG_BY_BOARD_LIST(k_backup_select_batch_proof, S, list, count);
    else TG_BY_BOARD_LIST(k_backup_select_proof, S, list, count);
}
void launch_proof_read(hipStream_t st, const SearchDev& S, uint8_t* root_status, uint8_t* child_status, int32_t* counts) {
    hipLaunchKernelGGL(k_proof_read, dim3(S.G), dim3(64), 0, st, S, root_status, child_status, counts);
}
void launch_sp_pick_proof(hipStream_t st, const SearchDev& S, const SelfPlayDev& P, int32_t* op) {
    hipLaunchKernelGGL(k_sp_pick_proof, wgrid(S.G), dim3(WPB * 64), 0, st, S, P, op);
}

}  // namespace tg
