// tree_kernels.hip — the kernels that walk the search trees, one wave per game: select, backup, and the two fused hand-overs
// between them.  Each is a thin shell around select_pass / backup_pass of tree_pass.cuh and exists once, as a template over
//   NB     the board size as a constant (5, 6: the BASELINE configs) or 0 = any size (3×3, 4×4)
//   LIST   false: wave w serves game w of S.G.  true: wave w < count serves game list[w] of a compacted list (the boosted
//          iterations of a self-play ply, selfplay.hip): everything of the tree and the game is game list[w]'s, its
//          leaves occupy slots w·batch + pass, the network is called with count × batch leaves.  list[w] < S.G for every
//          w < count (k_sp_boost_list writes game indices only) and count ≤ S.G, so every slot stays inside the G·batch per-leaf arrays
//   PROOF  the MCTS-solver backup inside select_pass (tg_search_set_proof(TG_PROOF_ON)); backup_pass knows nothing of proofs
// Same device functions, same order of operations on a game's tree in every instantiation → the same trees bit for bit.
#include <hip/hip_runtime.h>

// Diagnostic build only (-DTG_TREE_STAMPS, scripts/probes/tree_stamps.py): s_memtime stamps of the waves of the first 64 games
// at the phase boundaries of k_backup_select and of the passes it runs; tg_debug_tree_stamps copies them out.  The buffer and
// the macro are this file's: the product build, and every other file that includes tree_pass.cuh, compile none of it.
#ifdef TG_TREE_STAMPS
namespace tg {
__device__ unsigned long long g_tree_stamps[64][32];
}
#define TG_TSTAMP(g, slot)                                                                                    \
    do {                                                                                                      \
        if ((g) < 64 && (slot) < 32 && (threadIdx.x & 63) == 0) {                                             \
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                        \
            g_tree_stamps[(g)][(slot)] = __builtin_amdgcn_s_memtime();                                        \
        }                                                                                                     \
    } while (0)
#endif
#include "tree_pass.cuh"

namespace tg {

// wave w → (leaf-slot owner w, game g): identity, or entry w of the list; false: no game for this wave
template <bool LIST>
__device__ __forceinline__ bool wave_game(const SearchDev& S, const int32_t* __restrict__ list, int count, int& w, int& g) {
    w = game_of_wave();
    if (w >= (LIST ? count : S.G)) return false;
    g = LIST ? (int)uni((uint32_t)list[w]) : w;
    return true;
}

// What the select needs of the root and no backup writes, requested before the backup: the root's index (returned), the packed
// root position and the alive / abort flags; the root's cold record joins them inside the backup.  They arrive under the backup's
// own round trips (requested, none of them waited for: the first wait is inside the backup, behind its own independent requests).
template <int NB>
__device__ __forceinline__ uint32_t root_request(const SearchDev& S, int g, RootPre& pre) {
    const uint32_t root_v = S.root[g];
    const Geom geo = make_geom(NB ? NB : S.n);
    pre.raw = ws_load_raw(S.root_state + (size_t)g * geo.bytes, geo);
    pre.alive_v = (uint32_t)S.alive[g];
    pre.abort_v = (uint32_t)S.abort[g];
    pre.on = true;
    return root_v;
}

// S.pass ≥ 0: that one virtual rollout; S.pass < 0: all `batch` virtual rollouts of the iteration one after the other — a
// game's tree is only ever touched by its own wave, so the passes need no kernel boundary between them, only the wave's own
// stores ordered before its later loads (wave_sync_mem's s_waitcnt: a wave's accesses go through one in-order, write-through
// L1 path; an agent-scope fence would write back the whole L2 per wave and cost more than the launches it replaces).
template <int NB, bool LIST, bool PROOF>
__global__ __launch_bounds__(WPB * 64) void k_select(SearchDev S, const uint8_t* __restrict__ active, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    int w, g;
    if (!wave_game<LIST>(S, list, count, w, g)) return;
    uint32_t* path = path_lds[threadIdx.x >> 6];
    const int p0 = S.pass < 0 ? 0 : S.pass, p1 = S.pass < 0 ? S.batch : S.pass + 1;
    for (int p = p0; p < p1; p++) {
        select_pass<NB, LIST, PROOF>(S, active, g, p, path, mv_lds[threadIdx.x >> 6], RootPre(), w);
        if (p + 1 < p1) wave_sync_mem();
    }
}

// S.pass as in k_select: one de-virtualisation, or all of the iteration's in rollout order
template <int NB, bool LIST>
__global__ __launch_bounds__(WPB * 64) void k_backup(SearchDev S, const int32_t* __restrict__ list, int count) {
    int w, g;
    if (!wave_game<LIST>(S, list, count, w, g)) return;
    const int p0 = S.pass < 0 ? 0 : S.pass, p1 = S.pass < 0 ? S.batch : S.pass + 1;
    for (int p = p0; p < p1; p++) {
        backup_pass<NB>(S, w, p, S.root[g]);
        if (p + 1 < p1) wave_sync_mem();
    }
}

// De-virtualise iteration i and select the leaf of iteration i + 1 in one launch (one leaf per game): the two touch the same
// few nodes of the same tree from the same wave, so the second finds them in cache and one kernel boundary per iteration
// disappears.  Same device functions as the separate kernels → same trees.
template <int NB, bool LIST, bool PROOF>
__global__ __launch_bounds__(WPB * 64) void k_backup_select(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    int w, g;
    if (!wave_game<LIST>(S, list, count, w, g)) return;
    TG_TSTAMP(g, 0);
    RootPre pre;
    const uint32_t root_v = root_request<NB>(S, g, pre);
    backup_pass<NB>(S, w, 0, root_v, &pre);
    wave_sync_mem();
    TG_TSTAMP(g, 3);  // path updated
    select_pass<NB, LIST, PROOF>(S, nullptr, g, 0, path_lds[threadIdx.x >> 6], mv_lds[threadIdx.x >> 6], pre, w);
    TG_TSTAMP(g, 31);
}

// The same for `batch` > 1 virtual rollouts per tree and iteration (Player's batching, player.rs:77-110): the iteration's
// de-virtualisations in rollout order, then the next iteration's virtual rollouts, all in the game's wave — what k_backup
// followed by k_select do in two launches, on the same device functions → same trees.  A kernel of its own, so that the
// one-leaf k_backup_select keeps its straight-line form.  Between passes the wave's stores are ordered before its later loads
// by s_waitcnt alone (see k_select).
// Root hand-over: the root's index, packed position and the alive / abort flags are requested before the first backup (no
// backup writes them) and consumed by the first select; the root's cold record and its (visits, virtual) come from the LAST
// backup only — every earlier view of them is stale once a later pass has de-virtualised through the root.  The selects
// after the first read everything afresh: a pass that retires the game (limit_hit) sets S.abort[g], which the following
// passes must see to mark their slots skipped (leaf_kind 0: the next backup leaves them alone, and their network rows keep
// the finite contents of an earlier leaf).
template <int NB, bool LIST, bool PROOF>
__global__ __launch_bounds__(WPB * 64) void k_backup_select_batch(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    int w, g;
    if (!wave_game<LIST>(S, list, count, w, g)) return;
    RootPre pre;
    const uint32_t root_v = root_request<NB>(S, g, pre);
    const int B = S.batch;
    for (int p = 0; p < B; p++) {
        backup_pass<NB>(S, w, p, root_v, p + 1 == B ? &pre : nullptr);
        wave_sync_mem();
    }
    uint32_t* path = path_lds[threadIdx.x >> 6];
    uint16_t* mvl = mv_lds[threadIdx.x >> 6];
    for (int p = 0; p < B; p++) {
        select_pass<NB, LIST, PROOF>(S, nullptr, g, p, path, mvl, pre, w);
        pre.on = false;
        if (p + 1 < B) wave_sync_mem();
    }
}

// ---- launchers --------------------------------------------------------------------------------
// KERNEL<NB, TARGS…> over WAVES waves; TARGS: the template arguments behind the board size, in parentheses
#define TG_TARGS(...) __VA_ARGS__
#define TG_BY_BOARD(KERNEL, TARGS, WAVES, ...)                                                                                \
    do {                                                                                                                      \
        if (S.n == 5) hipLaunchKernelGGL((KERNEL<5, TG_TARGS TARGS>), wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__);      \
        else if (S.n == 6) hipLaunchKernelGGL((KERNEL<6, TG_TARGS TARGS>), wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__); \
        else hipLaunchKernelGGL((KERNEL<0, TG_TARGS TARGS>), wgrid(WAVES), dim3(WPB * 64), 0, st, __VA_ARGS__);               \
    } while (0)
// list = null: S.G waves, wave → game by identity; else `count` waves over the list (0 < count ≤ S.G)
#define TG_BY_BOARD_LIST_PROOF(KERNEL, ...)                                        \
    do {                                                                           \
        if (list && proof) TG_BY_BOARD(KERNEL, (true, true), count, __VA_ARGS__);  \
        else if (list) TG_BY_BOARD(KERNEL, (true, false), count, __VA_ARGS__);     \
        else if (proof) TG_BY_BOARD(KERNEL, (false, true), S.G, __VA_ARGS__);      \
        else TG_BY_BOARD(KERNEL, (false, false), S.G, __VA_ARGS__);                \
    } while (0)

void launch_select(hipStream_t st, const SearchDev& S, const uint8_t* active, const int32_t* list, int count, bool proof) {
    TG_BY_BOARD_LIST_PROOF(k_select, S, active, list, count);
}
void launch_backup(hipStream_t st, const SearchDev& S, const int32_t* list, int count) {
    if (list) TG_BY_BOARD(k_backup, (true), count, S, list, count);
    else TG_BY_BOARD(k_backup, (false), S.G, S, list, count);
}
void launch_backup_select(hipStream_t st, const SearchDev& S, const int32_t* list, int count, bool proof) {
    if (S.batch > 1) TG_BY_BOARD_LIST_PROOF(k_backup_select_batch, S, list, count);
    else TG_BY_BOARD_LIST_PROOF(k_backup_select, S, list, count);
}

#ifdef TG_TREE_STAMPS
extern "C" int tg_debug_tree_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tree_stamps), sizeof(g_tree_stamps));
}
#endif

}  // namespace tg
