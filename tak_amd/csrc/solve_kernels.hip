// solve_kernels.hip — forced wins: an exact depth-limited AND/OR search on the wave-distributed board (board.cuh).
// Kernels behind tg_solve / tg_search_solve; the definitions they implement (W, X, move values) are in include/takgpu.h.
//
// Shape: k_solve_root (one wave per position: move generation, finished roots answered at once), k_solve_scan (item offsets),
// then per level L = 1 … depth one k_solve_level<L, ROAD> (one wave per (position, root move)) and one k_solve_fold (one wave per
// position).  All on one stream; the only host wait is the one that sizes the item grid, before level 1.
//
// A work item replays its root move and asks X(s_a, L-1), then W(s_a, L-1).  Both are compile-time recursions over the
// remaining depth: every level's position is a WState of its own in registers (4 VGPRs + the wave-uniform header), every
// level's move list is a row of LDS, every branch is wave-uniform (moves and results are).  Cutoffs inside a level are
// complete — first success at an OR node, first failure at an AND node — because distances come from deepening L.
//
// One wave per workgroup: items differ in cost by orders of magnitude (an X test usually fails on the first reply, a failing
// W test walks every line), and a workgroup's LDS and wave slots are held until its slowest wave ends.
#include "board.cuh"
#include "solve.h"

namespace tg {
namespace {

constexpr int ROOT_WPB = 4;  // waves per workgroup of the per-position kernels (uniform cost)

struct SolveCtx {
    uint16_t* lds;     // move lists: row r holds the list of the position with r + 1 plies left
    uint32_t budget;
    uint32_t cnt;      // positions created by ws_play in this item and level
    bool over;         // cnt passed the budget: nothing proven from here on
    bool cut;          // a test failed on a move list cut at TG_MAX_MOVES: the search goes on, the item is reported as given up
};

// `r` is a win of colour `who`: by road or by flats, with ROAD (TG_SOLVE_ROAD_ONLY) by road alone
template <bool ROAD>
__device__ __forceinline__ bool won_by(uint32_t r, uint32_t who) {
    if constexpr (ROAD) return who == 0 ? r == TG_WHITE_ROAD : r == TG_BLACK_ROAD;
    else return who == 0 ? (r == TG_WHITE_ROAD || r == TG_WHITE_FLAT) : (r == TG_BLACK_ROAD || r == TG_BLACK_FLAT);
}

// → the moves staged (at most TG_MAX_MOVES); `cut` = the position has more than that, so the row holds only the first TG_MAX_MOVES of
// its list (include/takgpu.h "Move-list capacity inside the tree": the caller gives up instead of deciding on the part)
__device__ __forceinline__ int list_moves(const WState& s, const Geom& g, uint16_t* mv, bool& cut) {
    const int c = ws_movegen(s, g, TG_MAX_MOVES, [&](int idx, uint32_t code) { mv[idx] = (uint16_t)code; });
    __builtin_amdgcn_wave_barrier();  // the list is read back wave-uniformly below: lanes read what other lanes wrote
    cut = c > TG_MAX_MOVES;
    return cut ? TG_MAX_MOVES : c;
}

template <int L, bool ROAD>
__device__ __forceinline__ bool x_test(const WState& s, const Geom& g, SolveCtx& c);

// W(s, L): some move wins at once, or leads to a position whose mover loses within L-1.  L = 1 is the instant-win scan.
// A list cut at TG_MAX_MOVES is searched as far as it is staged: a win among those moves is a win; without one the test fails and
// the item is marked as given up.
template <int L, bool ROAD>
__device__ __forceinline__ bool w_test(const WState& s, const Geom& g, SolveCtx& c) {
    uint16_t* mv = c.lds + (L - 1) * TG_MAX_MOVES;
    bool cut;
    const int count = list_moves(s, g, mv, cut);
    for (int k = 0; k < count; k++) {
        WState t = s;
        ws_play(t, uni((uint32_t)mv[k]), g);
        if (++c.cnt > c.budget) { c.over = true; return false; }
        const uint32_t r = ws_result(t, g);
        if (won_by<ROAD>(r, s.to_move)) return true;
        if constexpr (L > 1) {
            if (r == TG_ONGOING) {
                if (x_test<L - 1, ROAD>(t, g, c)) return true;
                if (c.over) return false;
            }
        }
    }
    if (cut) c.cut = true;
    return false;
}

// X(s, L): every move loses at once, or leads to a position whose mover wins within L-1.  The first move that does neither
// (a draw among them, with ROAD a flat ending too) ends the test; so does a sub-test that ran out of budget, which comes back as "not proven".
// "Every move" cannot be said of a list cut at TG_MAX_MOVES: such a position fails before its first move is played and the item is
// marked as given up.
template <int L, bool ROAD>
__device__ __forceinline__ bool x_test(const WState& s, const Geom& g, SolveCtx& c) {
    uint16_t* mv = c.lds + (L - 1) * TG_MAX_MOVES;
    bool cut;
    const int count = list_moves(s, g, mv, cut);
    if (cut) { c.cut = true; return false; }
    for (int k = 0; k < count; k++) {
        WState t = s;
        ws_play(t, uni((uint32_t)mv[k]), g);
        if (++c.cnt > c.budget) { c.over = true; return false; }
        const uint32_t r = ws_result(t, g);
        if (won_by<ROAD>(r, s.to_move ^ 1u)) continue;
        if constexpr (L > 1) {
            if (r == TG_ONGOING && w_test<L - 1, ROAD>(t, g, c)) continue;
        }
        return false;
    }
    return true;
}

__global__ __launch_bounds__(ROOT_WPB * 64) void k_solve_root(SolveDev D) {
    const int gi = (int)(blockIdx.x * ROOT_WPB + (threadIdx.x >> 6));
    if (gi >= D.K) return;
    const Geom g = make_geom(D.n);
    const bool on = uni((!D.active || D.active[gi]) && (!D.alive || D.alive[gi]) ? 1u : 0u) != 0u;
    int c = 0;
    if (on) {
        WState s;
        ws_load(s, D.states + (size_t)gi * g.bytes, g);
        if (ws_result(s, g) == TG_ONGOING) {
            uint16_t* out = D.moves + (size_t)gi * TG_MAX_MOVES;  // (the row is zero beyond the list: cleared by the host)
            c = ws_movegen(s, g, TG_MAX_MOVES, [&](int idx, uint32_t code) { out[idx] = (uint16_t)code; });
        }
    }
    if (lane_id() == 0) {
        D.counts[gi] = c;
        D.value[gi] = 0;
        D.best[gi] = 0;
        D.decided[gi] = 0;
        D.budget_hit[gi] = 0;
        D.nodes[gi] = 0ull;
    }
}

// offsets[i] = Σ_{j < i} min(counts[j], TG_MAX_MOVES), offsets[K] = the item total.  One workgroup: K is a chunk of positions.
__global__ __launch_bounds__(256) void k_solve_scan(SolveDev D) {
    __shared__ int part[256];
    const int t = (int)threadIdx.x;
    const int per = (D.K + 255) / 256;
    const int i0 = t * per, i1 = i0 + per < D.K ? i0 + per : D.K;
    auto items = [&](int i) { const int c = D.counts[i]; return c < TG_MAX_MOVES ? c : TG_MAX_MOVES; };
    int sum = 0;
    for (int i = i0; i < i1; i++) sum += items(i);
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        for (int j = 0; j < 256; j++) { const int v = part[j]; part[j] = acc; acc += v; }
        D.offsets[D.K] = acc;
    }
    __syncthreads();
    int acc = part[t];
    for (int i = i0; i < i1; i++) { D.offsets[i] = acc; acc += items(i); }
}

template <int L, bool ROAD>
__global__ __launch_bounds__(64) void k_solve_level(SolveDev D, int n_items) {
    __shared__ uint16_t lds[(L > 1 ? L - 1 : 1) * TG_MAX_MOVES];
    const int item = (int)blockIdx.x;
    if (item >= n_items) return;
    // the position of the item: the last one whose first item is not behind it (positions without items share an offset with
    // their successor and are stepped over)
    int lo = 0, hi = D.K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (D.offsets[mid] <= item) lo = mid; else hi = mid;
    }
    const int pos = lo, k = item - D.offsets[pos];
    const size_t slot = (size_t)pos * TG_MAX_MOVES + (size_t)k;
    if (D.move_values[slot] != 0) return;             // proven at an earlier level
    if (!D.all_moves && D.decided[pos]) return;       // the position stopped at the level that decided it
    if (D.item_flag[item] & ITEM_ENDED) return;
    const Geom g = make_geom(D.n);
    WState s;
    ws_load(s, D.states + (size_t)pos * g.bytes, g);
    WState t = s;
    ws_play(t, uni((uint32_t)D.moves[slot]), g);
    const uint32_t r = ws_result(t, g);
    SolveCtx c{lds, D.budget, 1u, false, false};
    int v = 0;
    bool ended = false;  // the root move ends the game and proves nothing: a draw, with ROAD also flats of either colour
    if constexpr (L == 1) {
        if (won_by<ROAD>(r, s.to_move)) v = 1;
        else if (won_by<ROAD>(r, s.to_move ^ 1u)) v = -1;
        else ended = r != TG_ONGOING;
    } else {  // (an item that reaches a later level has an ongoing s_a)
        if (x_test<L - 1, ROAD>(t, g, c)) v = L;
        else if (!c.over && w_test<L - 1, ROAD>(t, g, c)) v = -L;
    }
    if (lane_id() == 0) {
        if (v) D.move_values[slot] = (int8_t)v;
        D.item_nodes[item] += (unsigned long long)c.cnt;
        const bool gave_up = c.over || c.cut;
        if (ended || gave_up) D.item_flag[item] = (uint8_t)(D.item_flag[item] | (ended ? ITEM_ENDED : 0) | (gave_up ? ITEM_GAVE_UP : 0));
    }
}

__device__ __forceinline__ int wave_min(int v) {
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// value, best, decided, budget_hit and nodes of a position from its row of the move table and its items
__global__ __launch_bounds__(ROOT_WPB * 64) void k_solve_fold(SolveDev D) {
    const int gi = (int)(blockIdx.x * ROOT_WPB + (threadIdx.x >> 6));
    if (gi >= D.K) return;
    const int lane = lane_id();
    const int c = D.offsets[gi + 1] - D.offsets[gi];
    if (c == 0) return;  // (k_solve_root has written the zero row)
    const int8_t* mv = D.move_values + (size_t)gi * TG_MAX_MOVES;
    const size_t item0 = (size_t)D.offsets[gi];
    int min_pos = 127, max_abs = 0, non_neg = 0, hit = 0;
    unsigned long long nodes = 0;
    for (int k = lane; k < c; k += 64) {
        const int v = mv[k];
        if (v > 0 && v < min_pos) min_pos = v;
        if (v >= 0) non_neg = 1;
        const int a = v < 0 ? -v : v;
        if (a > max_abs) max_abs = a;
        nodes += D.item_nodes[item0 + k];
        hit |= (D.item_flag[item0 + k] & ITEM_GAVE_UP) ? 1 : 0;
    }
    min_pos = wave_min(min_pos);
    max_abs = wave_max(max_abs);
    non_neg = wave_max(non_neg);
    hit = wave_max(hit);
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)nodes, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(nodes >> 32), d);
        nodes += ((unsigned long long)hi << 32) | lo;
    }
    int value = 0;
    if (min_pos < 127) value = min_pos;
    else if (!non_neg) value = -max_abs;
    int first = TG_MAX_MOVES;
    if (value != 0)
        for (int k = lane; k < c; k += 64)
            if ((int)mv[k] == value) { first = k; break; }
    first = wave_min(first);
    if (lane == 0) {
        D.value[gi] = (int8_t)value;
        D.best[gi] = value != 0 ? D.moves[(size_t)gi * TG_MAX_MOVES + first] : (uint16_t)0;
        D.decided[gi] = value != 0;
        D.budget_hit[gi] = (uint8_t)hit;
        D.nodes[gi] = nodes;
    }
}

inline dim3 wave_grid(int count) { return dim3((count + ROOT_WPB - 1) / ROOT_WPB); }

}  // namespace

void launch_solve_root(hipStream_t st, const SolveDev& D) {
    if (D.K > 0) hipLaunchKernelGGL(k_solve_root, wave_grid(D.K), dim3(ROOT_WPB * 64), 0, st, D);
}
void launch_solve_scan(hipStream_t st, const SolveDev& D) {
    if (D.K > 0) hipLaunchKernelGGL(k_solve_scan, dim3(1), dim3(256), 0, st, D);
}
void launch_solve_level(hipStream_t st, const SolveDev& D, bool road, int level, int items) {
    if (items <= 0) return;
#define TG_SOLVE_LEVEL(L)                                                                                      \
    case L:                                                                                                    \
        if (road) hipLaunchKernelGGL((k_solve_level<L, true>), dim3(items), dim3(64), 0, st, D, items);        \
        else hipLaunchKernelGGL((k_solve_level<L, false>), dim3(items), dim3(64), 0, st, D, items);            \
        break
    switch (level) {
        TG_SOLVE_LEVEL(1);
        TG_SOLVE_LEVEL(2);
        TG_SOLVE_LEVEL(3);
        TG_SOLVE_LEVEL(4);
        TG_SOLVE_LEVEL(5);
        TG_SOLVE_LEVEL(6);
    }
#undef TG_SOLVE_LEVEL
}
void launch_solve_fold(hipStream_t st, const SolveDev& D) {
    if (D.K > 0) hipLaunchKernelGGL(k_solve_fold, wave_grid(D.K), dim3(ROOT_WPB * 64), 0, st, D);
}

}  // namespace tg
