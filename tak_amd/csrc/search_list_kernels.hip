// search_list_kernels.hip — the tree kernels over a compacted list of games, and the kernel that writes the list: the boosted
// iterations of a self-play ply (tg_selfplay_set_schedule; QUAD_ROLLOUT_PLIES, train/src/self_play.rs:19,63) run over the games
// that are owed them only.  The passes themselves are tree_pass.cuh's, shared with search_kernels.hip.  A translation unit of
// its own: the code object of search_kernels.hip stays what it was without the schedule.
#undef TG_TREE_STAMPS  // the stamp buffer belongs to search_kernels.hip
#include "tree_pass.cuh"
#include "tree_launch.h"

namespace tg {

// ------------------------------------------------------------------------------------------------
// The same four kernels over a compacted list of games (the boosted iterations of a self-play ply, selfplay.hip): wave w < count
// serves game list[w], its leaves occupy slots w·batch + pass, the network is called with count × batch leaves.  Same device
// functions, same order of operations on a game's tree as the identity-mapped kernels → same trees.  list[w] < S.G for every
// w < count (k_sp_boost_list writes game indices only), count ≤ S.G, so every slot stays inside the G·batch per-leaf arrays.
// ------------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(WPB * 64) void k_select_list(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    const int w = game_of_wave();
    if (w >= count) return;
    const int g = (int)uni((uint32_t)list[w]);
    uint32_t* path = path_lds[threadIdx.x >> 6];
    const int p0 = S.pass < 0 ? 0 : S.pass, p1 = S.pass < 0 ? S.batch : S.pass + 1;
    for (int p = p0; p < p1; p++) {
        select_pass<NB, true>(S, nullptr, g, p, path, mv_lds[threadIdx.x >> 6], RootPre(), w);
        if (p + 1 < p1) wave_sync_mem();
    }
}

template <int NB>
__global__ __launch_bounds__(WPB * 64) void k_backup_list(SearchDev S, const int32_t* __restrict__ list, int count) {
    const int w = game_of_wave();
    if (w >= count) return;
    const int g = (int)uni((uint32_t)list[w]);
    const int p0 = S.pass < 0 ? 0 : S.pass, p1 = S.pass < 0 ? S.batch : S.pass + 1;
    for (int p = p0; p < p1; p++) {
        backup_pass<NB>(S, w, p, S.root[g]);
        if (p + 1 < p1) wave_sync_mem();
    }
}

template <int NB>
__global__ __launch_bounds__(WPB * 64) void k_backup_select_list(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    const int w = game_of_wave();
    if (w >= count) return;
    const int g = (int)uni((uint32_t)list[w]);
    RootPre pre;
    const uint32_t root_v = S.root[g];
    const Geom geo = make_geom(NB ? NB : S.n);
    pre.raw = ws_load_raw(S.root_state + (size_t)g * geo.bytes, geo);
    pre.alive_v = (uint32_t)S.alive[g];
    pre.abort_v = (uint32_t)S.abort[g];
    pre.on = true;
    backup_pass<NB>(S, w, 0, root_v, &pre);
    wave_sync_mem();
    select_pass<NB, true>(S, nullptr, g, 0, path_lds[threadIdx.x >> 6], mv_lds[threadIdx.x >> 6], pre, w);
}

template <int NB>
__global__ __launch_bounds__(WPB * 64) void k_backup_select_batch_list(SearchDev S, const int32_t* __restrict__ list, int count) {
    __shared__ uint32_t path_lds[WPB][MAX_DEPTH];
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    const int w = game_of_wave();
    if (w >= count) return;
    const int g = (int)uni((uint32_t)list[w]);
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
        select_pass<NB, true>(S, nullptr, g, p, path, mvl, pre, w);
        pre.on = false;
        if (p + 1 < B) wave_sync_mem();
    }
}

// The games owed the boosted iterations of this ply (QUAD_ROLLOUT_PLIES, train/src/self_play.rs:19,63): alive, not retired by
// this ply's search so far, root ply < boost_plies — in ascending order, with their count.  One workgroup: every thread counts its
// run of consecutive games, an inclusive scan places the runs (as k_sp_finish_scan does).
__global__ __launch_bounds__(1024) void k_sp_boost_list(SearchDev S, int boost_plies, int32_t* __restrict__ list, int32_t* __restrict__ count) {
    __shared__ uint32_t s_n[1024];
    const int tid = threadIdx.x;
    const int per = (S.G + 1023) / 1024;
    const int g0 = min(tid * per, S.G), g1 = min(g0 + per, S.G);
    const Geom geo = make_geom(S.n);
    auto owed = [&](int g) {
        const uint32_t* hdr = (const uint32_t*)(S.root_state + (size_t)g * geo.bytes + geo.bytes - 16);
        return S.alive[g] && !S.abort[g] && (int)(hdr[0] >> 16) < boost_plies;
    };
    uint32_t n = 0;
    for (int g = g0; g < g1; g++) n += owed(g) ? 1u : 0u;
    s_n[tid] = n;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis–Steele inclusive scan
        const uint32_t a = tid >= d ? s_n[tid - d] : 0u;
        __syncthreads();
        s_n[tid] += a;
        __syncthreads();
    }
    uint32_t o = s_n[tid] - n;  // ≤ g0: the list never holds more entries than games
    for (int g = g0; g < g1; g++)
        if (owed(g)) list[o++] = g;
    if (tid == 1023) *count = (int32_t)s_n[1023];
}

// ---- launchers --------------------------------------------------------------------------------
// over a compacted list: 0 < count ≤ S.G entries, the grid sized from count
void launch_select_list(hipStream_t st, const SearchDev& S, const int32_t* list, int count) { TG_BY_BOARD(k_select_list, count, S, list, count); }
void launch_backup_list(hipStream_t st, const SearchDev& S, const int32_t* list, int count) { TG_BY_BOARD(k_backup_list, count, S, list, count); }
void launch_backup_select_list(hipStream_t st, const SearchDev& S, const int32_t* list, int count) {
    if (S.batch > 1) TG_BY_BOARD(k_backup_select_batch_list, count, S, list, count);
    else TG_BY_BOARD(k_backup_select_list, count, S, list, count);
}
void launch_sp_boost_list(hipStream_t st, const SearchDev& S, int boost_plies, int32_t* list, int32_t* count) {
    hipLaunchKernelGGL(k_sp_boost_list, dim3(1), dim3(1024), 0, st, S, boost_plies, list, count);
}

}  // namespace tg
