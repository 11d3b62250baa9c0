// search_kernels.hip — GPU-resident MCTS (one wavefront per game): everything around the tree passes, and the self-play driver
// kernels.  The passes themselves (select, backup and their fused hand-overs) are tree_kernels.hip's.
//
// With tree_pass.cuh and tree_kernels.hip, replaces reference alpha-tak/src/search/mcts.rs (virtual_rollout :26-65, select :94-118,
// devirtualize_path :67-91, update_concrete :120-124), search/noise.rs, search/play.rs and the
// per-ply phases of train/src/self_play.rs:108-259.  The float arithmetic of PUCT and of the value
// backup is written in the reference's operation order and compiled with -ffp-contract=off, the
// exploration rate comes from a host-computed table over the (integer) visit count, and both argmaxes
// keep the LAST maximum like Iterator::max_by / max_by_key, so that search traces are reproducible bit
// for bit against a scalar CPU statement of the same algorithm.
#include <stdlib.h>

#include "board.cuh"
#include "kernels.h"
#include "rng.cuh"
#include "search.cuh"
#include "softmax.cuh"
#include "tree_pass.cuh"

namespace tg {

// after a kernel that returned chunks: make them available to the following launches
// (also the high-water mark of chunks owned by trees, sampled here — after every re-root, when the trees are smallest — and
// therefore taken BEFORE the returns of this launch are counted: the occupancy just before the move was played)
__global__ void k_pool_publish(SearchDev S) {
    const unsigned long long owned = S.pool_ctl[0] - (S.pool_ctl[2] - (unsigned long long)(S.n_chunks - 1));
    if (owned > S.pool_ctl[3]) S.pool_ctl[3] = owned;
    S.pool_ctl[2] = S.pool_ctl[1];
}

// ------------------------------------------------------------------------------------------------
// apply_dirichlet, noise.rs:6-16
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_dirichlet(SearchDev S, const uint8_t* __restrict__ active, float alpha, float ratio) {
    __shared__ double gam[EX_MOVES];
    __shared__ double sum_s;
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    if (!S.alive[g] || (active && !active[g])) return;
    const Geom geo = make_geom(S.n);
    const uint32_t root = S.root[g];
    NodeHot* hot = S.hot;
    NodeCold rc = S.cold[root];
    const uint32_t nchild = (uint32_t)rc.nres & 0xfffu, cb = rc.child;
    if (nchild == 0 || hot[root].visits == 0) return;  // reference asserts visits > 0
    const uint32_t* hdr = (const uint32_t*)(S.root_state + (size_t)g * geo.bytes + geo.bytes - 16);
    const uint32_t ply = hdr[0] >> 16;
    const uint32_t gen = S.generation[g];
    for (uint32_t i = lane; i < nchild && i < EX_MOVES; i += 64)
        gam[i] = gamma_sample((double)alpha, S.seed, S.slot_base + (uint32_t)g, gen, ply, i);
    __syncthreads();
    if (lane == 0) {
        double sum = 0.0;
        for (uint32_t i = 0; i < nchild; i++) sum += gam[i];  // index order: matches the sequential statement
        sum_s = sum;
    }
    __syncthreads();
    const double sum = sum_s;
    for (uint32_t i = lane; i < nchild; i += 64) {
        float noise = sum > 0.0 ? (float)(gam[i] / sum) : (float)(1.0 / (double)nchild);
        float p = hot[cb + i].prior;
        hot[cb + i].prior = noise * ratio + p * (1.0f - ratio);
    }
}

__global__ __launch_bounds__(64) void k_apply_noise(SearchDev S, const uint8_t* __restrict__ active, const float* __restrict__ noise, float ratio) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    if (!S.alive[g] || (active && !active[g])) return;
    NodeHot* hot = S.hot;
    NodeCold rc = S.cold[S.root[g]];
    const uint32_t nchild = (uint32_t)rc.nres & 0xfffu, cb = rc.child;
    for (uint32_t i = lane; i < nchild && i < EX_MOVES; i += 64) {
        float p = hot[cb + i].prior;
        hot[cb + i].prior = noise[(size_t)g * EX_MOVES + i] * ratio + p * (1.0f - ratio);
    }
}

// ------------------------------------------------------------------------------------------------
// tree reuse: Node::play, play.rs:26-43.  op[g]: -2 = reset the tree (Node::default()), -1 = nothing,
// ≥ 0 = make that child the root.  The kept subtree is copied breadth-first into fresh chunks and the game's
// old chunks go back to the pool.  The copy is its own work queue (Cheney): a node is first copied with the OLD
// index of its children block; a scan pointer follows the allocation pointer through the new chunks and, for
// every copied node that has children, copies that block behind the allocation pointer and patches the index.
// No queue in LDS, no limit on the width or depth of the tree.  One wave per game.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_reroot(SearchDev S, const int32_t* __restrict__ op) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int o = op[g];
    if (o == -1) return;
    const uint32_t CH = 1u << S.chunk_shift;
    const uint32_t old_root = S.root[g];
    const uint32_t old_head = S.chunk_head[g];
    NodeHot* hot = S.hot;
    NodeCold* cold = S.cold;
    if (o == -2) {
        pool_give_chain(S, old_head);
        const uint32_t c = pool_take(S);
        if (c == 0) { flag(S, ERRF_ARENA); return; }
        const uint32_t a = c << S.chunk_shift;
        if (lane == 0) {
            NodeHot h; h.prior = 0.0f; h.q = 0.0f; h.visits = 0; h.virt = 0;
            NodeCold cc; cc.child = 0; cc.mv = 0; cc.nres = 0;
            hot[a] = h;
            cold[a] = cc;
            S.root[g] = a;
            S.alloc[2 * g] = a + 1;
            S.alloc[2 * g + 1] = a + CH;
            S.chunk_link[c] = 0;
            S.chunk_head[g] = c;
        }
        return;
    }
    const NodeCold rc = cold[old_root];
    const uint32_t rn = (uint32_t)rc.nres & 0xfffu;
    if ((uint32_t)o >= rn) { flag(S, ERRF_MOVE); return; }
    const uint32_t oc = rc.child + (uint32_t)o;
    uint32_t cur = pool_take(S);  // the chunk being filled
    if (cur == 0) { flag(S, ERRF_ARENA); return; }
    const uint32_t first = cur;
    uint32_t aoff = 1;            // nodes used in `cur`
    if (lane == 0) {
        hot[first << S.chunk_shift] = hot[oc];
        cold[first << S.chunk_shift] = cold[oc];  // .child still names the old block: patched when the scan reaches it
        S.chunk_link[first] = 0;
    }
    wave_sync_mem();
    uint32_t scan_c = first, scan_off = 0;
    for (;;) {
        const uint32_t limit = scan_c == cur ? aoff : uni(S.chunk_used[scan_c]);
        if (scan_off >= limit) {
            if (scan_c == cur) break;
            scan_c = uni(S.chunk_fwd[scan_c]);
            scan_off = 0;
            continue;
        }
        const uint32_t m = min(64u, limit - scan_off);
        const uint32_t idx = (scan_c << S.chunk_shift) + scan_off + (uint32_t)lane;
        const bool on = (uint32_t)lane < m;
        NodeCold c;
        c.child = 0; c.mv = 0; c.nres = 0;
        if (on) c = cold[idx];
        const uint32_t nch = on ? ((uint32_t)c.nres & 0xfffu) : 0u;
        uint32_t my_new = 0;
        bool failed = false;
        for (uint64_t bb = __ballot(nch > 0); bb; bb &= bb - 1) {
            const int l = __builtin_ctzll(bb);
            const uint32_t cnt = uni((uint32_t)__shfl((int)nch, l));
            const uint32_t src = uni((uint32_t)__shfl((int)c.child, l));
            if (aoff + cnt > CH) {  // close the chunk, open the next
                const uint32_t c2 = pool_take(S);
                if (c2 == 0) { failed = true; break; }
                if (lane == 0) { S.chunk_used[cur] = aoff; S.chunk_fwd[cur] = c2; S.chunk_link[c2] = cur; }
                cur = c2;
                aoff = 0;
            }
            const uint32_t dst = (cur << S.chunk_shift) + aoff;
            for (uint32_t k = lane; k < cnt; k += 64) {
                hot[dst + k] = hot[src + k];
                cold[dst + k] = cold[src + k];
            }
            if (lane == l) my_new = dst;
            aoff += cnt;
        }
        if (failed) { flag(S, ERRF_ARENA); return; }  // the error is sticky: the engine refuses further work until reset
        if (nch > 0) cold[idx].child = my_new;
        scan_off += m;
        wave_sync_mem();  // the scan reads back what this wave has just written
    }
    if (lane == 0) {
        S.root[g] = first << S.chunk_shift;
        S.alloc[2 * g] = (cur << S.chunk_shift) + aoff;
        S.alloc[2 * g + 1] = (cur + 1) << S.chunk_shift;
        S.chunk_head[g] = cur;
    }
    pool_give_chain(S, old_head);
}

// root children → host-visible arrays (Node::improved_policy, play.rs:13-21, plus priors / q)
__global__ __launch_bounds__(64) void k_root_stats(SearchDev S, uint16_t* moves, uint32_t* visits, float* prior, float* q,
                                                   int32_t* counts, uint32_t* root_visits, float* root_q) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const uint32_t root = S.root[g];
    NodeCold rc = S.cold[root];
    NodeHot rh = S.hot[root];
    const uint32_t nchild = (uint32_t)rc.nres & 0xfffu, cb = rc.child;
    if (lane == 0) { counts[g] = (int32_t)nchild; root_visits[g] = rh.visits; root_q[g] = rh.q; }
    for (uint32_t i = lane; i < nchild && i < EX_MOVES; i += 64) {
        NodeHot h = S.hot[cb + i];
        size_t o = (size_t)g * EX_MOVES + i;
        moves[o] = S.cold[cb + i].mv;
        visits[o] = h.visits;
        prior[o] = h.prior;
        q[o] = h.q;
    }
}

// tg_search_debug: Node::debug(depth) of every root (alpha-tak/src/search/debug.rs:9-51), one 256-thread workgroup per game of the
// slice [g0, g0 + gridDim.x).  Outputs are slice-local (row b = game g0 + b):
//   children  [b][EX_MOVES]      sorted by visits descending, ties by child index descending (a stable ascending sort + reverse();
//                                the reference's sort_unstable_by_key + reverse gives the same for ≤ 20 children, leaves it
//                                unspecified beyond); zero past the child count
//   counts/eval [b]              eval = Σ reward_i · (visits_i / total) in the sorted order from +0.0f, f32, no contraction
//   cont_*    [b][top_k][depth]  Node::continuation of the first top_k sorted children: while the node is initialised (visits or
//                                virtual visits ≠ 0) and has children, step to its most visited child (last on ties, pick_move(true),
//                                play.rs:49-57); zero past cont_len [b][top_k]
// Every index read from the tree is checked against the pool (a bad one ends that walk), so no read leaves the node arrays.
constexpr int DBG_WAVES = 4;

__global__ __launch_bounds__(DBG_WAVES * 64) void k_search_debug(SearchDev S, int g0, int depth, int top_k, DebugOut o) {
    __shared__ uint64_t key[EX_MOVES];     // (visits << 32) | child index, in child order
    __shared__ uint32_t s_node[EX_MOVES];  // sorted position → pool index of the child
    __shared__ uint32_t s_vis[EX_MOVES];
    __shared__ float s_q[EX_MOVES];
    const int b = blockIdx.x, g = g0 + b;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t pool = (uint64_t)S.n_chunks << S.chunk_shift;
    const uint32_t root = S.root[g];
    uint32_t nchild = 0, cb = 0;
    if (root < pool) {
        const NodeCold rc = S.cold[root];
        nchild = min((uint32_t)rc.nres & 0xfffu, (uint32_t)EX_MOVES);
        cb = rc.child;
        if ((uint64_t)cb + nchild > pool) nchild = 0;
    }
    for (uint32_t i = tid; i < nchild; i += DBG_WAVES * 64) key[i] = ((uint64_t)S.hot[cb + i].visits << 32) | i;
    __syncthreads();
    // rank = number of children with a larger key (all keys differ): the child's position in the sorted list
    for (uint32_t i = tid; i < (uint32_t)EX_MOVES; i += DBG_WAVES * 64) {
        const size_t ob = (size_t)b * EX_MOVES;
        if (i < nchild) {
            const uint64_t ki = key[i];
            uint32_t r = 0;
            for (uint32_t j = 0; j < nchild; j++) r += key[j] > ki ? 1u : 0u;
            const NodeHot h = S.hot[cb + i];
            o.moves[ob + r] = S.cold[cb + i].mv;
            o.visits[ob + r] = h.visits;
            o.reward[ob + r] = h.q;
            o.policy[ob + r] = h.prior;
            s_node[r] = cb + i;
            s_vis[r] = h.visits;
            s_q[r] = h.q;
        } else {  // the ranks of the children fill [0, nchild) exactly
            o.moves[ob + i] = 0;
            o.visits[ob + i] = 0;
            o.reward[ob + i] = 0.0f;
            o.policy[ob + i] = 0.0f;
        }
    }
    __syncthreads();
    if (tid == 0) {  // NodeDebugInfo::eval (debug.rs:43-51): u32 sum of visits, then one f32 chain in the sorted order
        uint32_t sum = 0;
        for (uint32_t r = 0; r < nchild; r++) sum += s_vis[r];
        const float total = (float)sum;
        float acc = 0.0f;
        for (uint32_t r = 0; r < nchild; r++) acc = acc + s_q[r] * ((float)s_vis[r] / total);
        o.counts[b] = (int32_t)nchild;
        o.eval[b] = acc;
    }
    // continuations: wave w walks ranks r ≡ w (mod DBG_WAVES); each level is one coalesced scan of the node's children
    for (int r = wave; r < top_k; r += DBG_WAVES) {
        const size_t ob = ((size_t)b * top_k + r) * depth;
        int len = 0;
        uint32_t node = (uint32_t)r < nchild ? s_node[r] : 0u;
        while ((uint32_t)r < nchild && len < depth) {
            const NodeHot h = S.hot[node];
            const NodeCold c = S.cold[node];
            const uint32_t nch = (uint32_t)c.nres & 0xfffu, ccb = c.child;
            if ((h.visits == 0 && h.virt == 0) || nch == 0 || (uint64_t)ccb + nch > pool) break;
            uint64_t best = 0;
            for (uint32_t i = lane; i < nch; i += 64) {
                const uint64_t k = ((uint64_t)S.hot[ccb + i].visits << 32) | i;
                best = k > best ? k : best;
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const uint64_t ot = __shfl_xor(best, d);
                best = ot > best ? ot : best;
            }
            node = ccb + (uint32_t)best;
            if (lane == 0) {
                o.cont_moves[ob + len] = S.cold[node].mv;
                o.cont_visits[ob + len] = (uint32_t)(best >> 32);
            }
            len++;
        }
        for (int l = len + lane; l < depth; l += 64) {
            o.cont_moves[ob + l] = 0;
            o.cont_visits[ob + l] = 0;
        }
        if (lane == 0) o.cont_len[(size_t)b * top_k + r] = len;
    }
}

// tg_search_play: find the child for a caller-chosen move, play it on the root state
__global__ __launch_bounds__(WPB * 64) void k_play_move(SearchDev S, const uint16_t* __restrict__ moves, const uint8_t* __restrict__ active,
                                                   int32_t* __restrict__ op) {
    const int g = game_of_wave();
    if (g >= S.G) return;
    const int lane = lane_id();
    if (!S.alive[g] || (active && !active[g])) { if (lane == 0) op[g] = -1; return; }
    const Geom geo = make_geom(S.n);
    NodeCold rc = S.cold[S.root[g]];
    const uint32_t nchild = uni((uint32_t)rc.nres) & 0xfffu, cb = uni(rc.child);
    const uint32_t mv = uni((uint32_t)moves[g]);
    int found = -1;
    for (uint32_t i0 = 0; i0 < nchild && found < 0; i0 += 64) {
        uint32_t i = i0 + lane;
        bool hit = i < nchild && S.cold[cb + i].mv == mv;
        uint64_t bb = __ballot(hit);
        if (bb) found = (int)i0 + __builtin_ctzll(bb);
    }
    if (found < 0) {  // "tried to play an invalid move" / "node must be initialized" (play.rs:10,35)
        flag(S, ERRF_MOVE);
        if (lane == 0) op[g] = -1;
        return;
    }
    WState s;
    uint8_t* st = S.root_state + (size_t)g * geo.bytes;
    ws_load(s, st, geo);
    ws_play(s, mv, geo);
    ws_store(s, st, geo);
    if (lane == 0) op[g] = found;
}

// ------------------------------------------------------------------------------------------------
// self_play_parallel phases (train/src/self_play.rs:108-259)
// ------------------------------------------------------------------------------------------------

// (a) opening, :110-116.  "a1", then one of the two far corners (reference hard-codes the 6×6 names
// a6 / f6; generalised to (0, N-1) / (N-1, N-1)).
__global__ __launch_bounds__(WPB * 64) void k_sp_opening(SearchDev S) {
    const int g = game_of_wave();
    if (g >= S.G) return;
    if (!S.alive[g]) return;
    const Geom geo = make_geom(S.n);
    WState s;
    uint8_t* st = S.root_state + (size_t)g * geo.bytes;
    ws_load(s, st, geo);
    if (s.ply != 0) return;
    ws_play(s, 0u /* a1 flat */, geo);
    U4 r = rng_draw(S.seed, S.slot_base + (uint32_t)g, S.generation[g], 0, RNG_OPENING, 0, 0);
    uint32_t col = (r.v[0] & 1u) ? 0u : (uint32_t)(geo.n - 1);
    ws_play(s, (uint32_t)((geo.n - 1) * geo.n) + col, geo);
    ws_store(s, st, geo);
}

// (b) instant-win scan, :119-171
__global__ __launch_bounds__(WPB * 64) void k_sp_instant_win(SearchDev S, SelfPlayDev P) {
    __shared__ uint16_t mv_lds[WPB][EX_MOVES];
    __shared__ uint8_t win_lds[WPB][EX_MOVES];
    const int g = game_of_wave();
    if (g >= S.G) return;
    const int lane = lane_id();
    if (lane == 0) P.fin[g] = 0;
    if (!S.alive[g]) return;
    const Geom geo = make_geom(S.n);
    WState s;
    ws_load(s, S.root_state + (size_t)g * geo.bytes, geo);
    uint16_t* mv = mv_lds[threadIdx.x >> 6];
    uint8_t* wl = win_lds[threadIdx.x >> 6];
    int count = ws_movegen(s, geo, EX_MOVES, [&](int idx, uint32_t code) { mv[idx] = (uint16_t)code; });
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (count > EX_MOVES) {  // (such positions exist on 5×5 and 6×6, takgpu.h TG_LIMIT_*: the capacity is reported, the list is never used cut)
        limit_hit(S, g, ERRF_MOVES);
        if (lane == 0) P.fin[g] = FIN_ABORTED;
        return;
    }
    bool win = false;
    for (int k = 0; k < count; k++) {
        WState t = s;
        ws_play(t, (uint32_t)mv[k], geo);
        uint32_t r = ws_result(t, geo);
        bool w = (r >= TG_WHITE_ROAD && r <= TG_BLACK_FLAT) && (((r == TG_WHITE_ROAD || r == TG_WHITE_FLAT) ? 0u : 1u) == s.to_move);
        if (lane == 0) wl[k] = w ? 1 : 0;
        win |= w;
    }
    if (!win) return;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int slot;
    stage_example(S, P, g, s, geo, (uint32_t)count, slot);
    if (slot < 0) {  // the game is past max_game_plies: retired without examples
        if (lane == 0) P.fin[g] = FIN_ABORTED;
        return;
    }
    {
        size_t e = (size_t)g * P.ex_per_game + slot;
        for (int k = lane; k < count; k += 64) {
            P.st_moves[e * EX_MOVES + k] = mv[k];
            P.st_visits[e * EX_MOVES + k] = wl[k] ? 1000u : 1u;  // fake visits, :129-134
        }
    }
    if (lane == 0) {
        P.fin[g] = (uint8_t)(s.to_move == 0 ? TG_WHITE_FLAT : TG_BLACK_FLAT);  // Winner { color: to_move, road: false }, :147
        atomicAdd(&P.stats[ST_INSTANT], 1ull);
    }
}

// ordered bookkeeping of the games that ended in this phase (slot order = the reference's loop order):
// completed counter, recycle-or-retire decision (:151,237), contiguous output ranges for their examples.
__global__ __launch_bounds__(1024) void k_sp_finish_scan(SearchDev S, SelfPlayDev P) {
    __shared__ uint32_t s_fin[1024], s_ex[1024];
    const int tid = threadIdx.x;
    const int per = (S.G + 1023) / 1024;
    const int g0 = tid * per, g1 = min(g0 + per, S.G);
    uint32_t nf = 0, ne = 0;
    // (a retired game — FIN_ABORTED — is not a completed game and emits nothing; its slot always restarts)
    for (int g = g0; g < g1; g++)
        if (P.fin[g] && P.fin[g] != FIN_ABORTED) { nf++; ne += (uint32_t)P.st_count[g]; }
    s_fin[tid] = nf;
    s_ex[tid] = ne;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {  // Hillis–Steele inclusive scan
        uint32_t a = tid >= d ? s_fin[tid - d] : 0u, b = tid >= d ? s_ex[tid - d] : 0u;
        __syncthreads();
        s_fin[tid] += a;
        s_ex[tid] += b;
        __syncthreads();
    }
    const unsigned long long done0 = P.stats[ST_FINISHED], ex0 = P.stats[ST_EXAMPLES];
    uint32_t rf = s_fin[tid] - nf, re = s_ex[tid] - ne;
    for (int g = g0; g < g1; g++) {
        if (!P.fin[g]) continue;
        if (P.fin[g] == FIN_ABORTED) { P.recycle[g] = 1; continue; }
        unsigned long long completed = done0 + rf + 1;
        P.recycle[g] = (P.total_games == 0 || completed + (unsigned long long)S.G < (unsigned long long)P.total_games) ? 1 : 0;
        P.out_off[g] = (uint32_t)((ex0 + re) % (unsigned long long)P.max_examples);
        rf++;
        re += (uint32_t)P.st_count[g];
    }
    __syncthreads();
    if (tid == 1023) {
        P.stats[ST_FINISHED] = done0 + s_fin[1023];
        P.stats[ST_EXAMPLES] = ex0 + s_ex[1023];
    }
}

// complete the finished games' examples (:158-169, :245-256), reset tree and game (or retire the slot)
__global__ __launch_bounds__(WPB * 64) void k_sp_finish_apply(SearchDev S, SelfPlayDev P, int32_t* __restrict__ op) {
    const int g = game_of_wave();
    if (g >= S.G) return;
    const int lane = lane_id();
    const uint32_t r = P.fin[g];
    if (!r) return;
    const Geom geo = make_geom(S.n);
    const bool aborted = r == FIN_ABORTED;
    const float white_result = (r == TG_WHITE_ROAD || r == TG_WHITE_FLAT) ? 1.0f : (r == TG_BLACK_ROAD || r == TG_BLACK_FLAT) ? -1.0f : 0.0f;
    const int cnt = aborted ? 0 : P.st_count[g];
    const uint32_t off = P.out_off[g];
    for (int k = 0; k < cnt; k++) {
        size_t e = (size_t)g * P.ex_per_game + k;
        size_t o = (size_t)((off + (uint32_t)k) % (uint32_t)P.max_examples);
        ExampleRec h = P.st_hdr[e];
        const uint8_t* st = P.st_state + e * geo.bytes;
        uint32_t to_move = st[geo.bytes - 16 + 1];
        h.result = to_move == 0 ? white_result : -white_result;
        if (lane == 0) P.out_hdr[o] = h;
        for (int b = lane; b < geo.bytes / 4; b += 64) ((uint32_t*)(P.out_state + o * geo.bytes))[b] = ((const uint32_t*)st)[b];
        for (int m = lane; m < h.n_moves; m += 64) {
            P.out_moves[o * EX_MOVES + m] = P.st_moves[e * EX_MOVES + m];
            P.out_visits[o * EX_MOVES + m] = P.st_visits[e * EX_MOVES + m];
        }
    }
    WState s;
    ws_start(s, geo, P.komi * 2);
    ws_store(s, S.root_state + (size_t)g * geo.bytes, geo);
    if (lane == 0) {
        P.st_count[g] = 0;
        S.generation[g] += 1;
        if (!P.recycle[g]) S.alive[g] = 0;
        op[g] = -2;  // *node = Node::default()
        S.abort[g] = 0;
        atomicAdd(&P.stats[aborted ? ST_ABORTED : white_result > 0 ? ST_WHITE : white_result < 0 ? ST_BLACK : ST_DRAWS], 1ull);
    }
}

__global__ void k_sp_noise_mask(SearchDev S, SelfPlayDev P) {
    int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= S.G) return;
    const Geom geo = make_geom(S.n);
    const uint32_t* hdr = (const uint32_t*)(S.root_state + (size_t)g * geo.bytes + geo.bytes - 16);
    P.mask[g] = (S.alive[g] && (int)(hdr[0] >> 16) < P.noise_plies) ? 1 : 0;
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

// (e) pick_move (play.rs:49-67), example (:222-225), play (:227-228), result (:230)
// PROOF (tg_search_set_proof(TG_PROOF_ON); no counterpart in the reference): the candidates are narrowed by the root children's
// statuses.  m = the root's colour to move.
//   1. some child decided for m: among those children the most visited, the LAST on ties — whatever the temperature
//   2. otherwise the candidates are the children not decided for the opponent (all children if that leaves none), and on them
//      pick_move: exploit → most visited, last on ties; explore → the RNG_PICK draw over the visits with the excluded children's
//      visits taken as 0; candidates without a visit → exploit over the candidates (not ERRF_PICK)
// The example keeps the root's real visits.  PROOF off: every child is a candidate, none of the narrowing is compiled.
template <bool PROOF>
__global__ __launch_bounds__(WPB * 64) void k_sp_pick(SearchDev S, SelfPlayDev P, int32_t* __restrict__ op) {
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
    bool step1 = false, narrow = false;
    if constexpr (PROOF) {
        bool any_m = false, any_open = false;
        for (uint32_t i = lane; i < nchild; i += 64) {
            const uint32_t cs = proof_status((uint32_t)cold[cb + i].nres >> 12);
            any_m |= cs == m;
            any_open |= cs != opp;
        }
        step1 = __ballot(any_m) != 0;
        narrow = __ballot(any_open) != 0;
    }
    auto candidate = [&](uint32_t i) {
        if constexpr (PROOF) {
            const uint32_t cs = proof_status((uint32_t)cold[cb + i].nres >> 12);
            return step1 ? cs == m : narrow ? cs != opp : true;
        } else return true;
    };
    auto visits_of_candidates = [&]() {
        unsigned long long total = 0;
        for (uint32_t i = lane; i < nchild; i += 64) total += candidate(i) ? hot[cb + i].visits : 0u;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            unsigned long long o = ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(total >> 32), d) << 32) |
                                   (uint32_t)__shfl_xor((int)(uint32_t)total, d);
            total += o;
        }
        return total;
    };
    // PROOF: the total decides the branch (no visit on a candidate → exploit); off: it is taken on the explore branch only
    unsigned long long total = 0;
    bool exploit = (int)s.ply >= P.exploit_plies;
    if constexpr (PROOF) {
        total = visits_of_candidates();
        exploit = step1 || total == 0 || exploit;
    }
    int pick = -1;
    if (exploit) {
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
        if constexpr (!PROOF) {
            total = visits_of_candidates();
            if (total == 0) { flag(S, ERRF_PICK); return; }
        }
        U4 r = rng_draw(S.seed, S.slot_base + (uint32_t)g, S.generation[g], s.ply, RNG_PICK, 0, 0);
        unsigned long long x = ((unsigned long long)r.v[0] << 32) | r.v[1];
        unsigned long long target = __umul64hi(x, total);
        unsigned long long carry = 0;
        // where a draw that no prefix exceeds ends: the last child, or (PROOF) the last candidate with visits
        int last = (int)nchild - 1;
        if constexpr (PROOF) last = -1;
        for (uint32_t i0 = 0; i0 < nchild && (PROOF || pick < 0); i0 += 64) {
            uint32_t i = i0 + lane;
            int v = (i < nchild && candidate(i)) ? (int)hot[cb + i].visits : 0;
            int incl = wave_inclusive_scan(v);
            uint64_t bb = __ballot(i < nchild && (!PROOF || v > 0) && carry + (unsigned long long)incl > target);
            if (bb && pick < 0) pick = (int)i0 + __builtin_ctzll(bb);
            if constexpr (PROOF) {
                uint64_t nz = __ballot(v > 0);
                if (nz) last = (int)i0 + 63 - __builtin_clzll(nz);
            }
            carry += (unsigned long long)__shfl(incl, 63);
        }
        if (pick < 0) pick = last;
    }
    if constexpr (PROOF)
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

__global__ void k_sp_count_ply(SelfPlayDev P) { P.stats[ST_PLIES] += 1; }

// ---- launchers --------------------------------------------------------------------------------
void launch_dirichlet(hipStream_t st, const SearchDev& S, const uint8_t* active, float alpha, float ratio) {
    hipLaunchKernelGGL(k_dirichlet, dim3(S.G), dim3(64), 0, st, S, active, alpha, ratio);
}
void launch_apply_noise(hipStream_t st, const SearchDev& S, const uint8_t* active, const float* noise, float ratio) {
    hipLaunchKernelGGL(k_apply_noise, dim3(S.G), dim3(64), 0, st, S, active, noise, ratio);
}
void launch_reroot(hipStream_t st, const SearchDev& S, const int32_t* op) {
    hipLaunchKernelGGL(k_reroot, dim3(S.G), dim3(64), 0, st, S, op);
    hipLaunchKernelGGL(k_pool_publish, dim3(1), dim3(1), 0, st, S);
}
void launch_root_stats(hipStream_t st, const SearchDev& S, uint16_t* moves, uint32_t* visits, float* prior, float* q, int32_t* counts,
                       uint32_t* root_visits, float* root_q) {
    hipLaunchKernelGGL(k_root_stats, dim3(S.G), dim3(64), 0, st, S, moves, visits, prior, q, counts, root_visits, root_q);
}
void launch_search_debug(hipStream_t st, const SearchDev& S, int g0, int games, int depth, int top_k, const DebugOut& o) {
    hipLaunchKernelGGL(k_search_debug, dim3(games), dim3(DBG_WAVES * 64), 0, st, S, g0, depth, top_k, o);
}
void launch_play_move(hipStream_t st, const SearchDev& S, const uint16_t* moves, const uint8_t* active, int32_t* op) {
    hipLaunchKernelGGL(k_play_move, wgrid(S.G), dim3(WPB * 64), 0, st, S, moves, active, op);
}
void launch_sp_opening(hipStream_t st, const SearchDev& S) { hipLaunchKernelGGL(k_sp_opening, wgrid(S.G), dim3(WPB * 64), 0, st, S); }
void launch_sp_instant_win(hipStream_t st, const SearchDev& S, const SelfPlayDev& P) {
    hipLaunchKernelGGL(k_sp_instant_win, wgrid(S.G), dim3(WPB * 64), 0, st, S, P);
}
void launch_sp_finish(hipStream_t st, const SearchDev& S, const SelfPlayDev& P, int32_t* op) {
    hipLaunchKernelGGL(k_sp_finish_scan, dim3(1), dim3(1024), 0, st, S, P);
    hipLaunchKernelGGL(k_sp_finish_apply, wgrid(S.G), dim3(WPB * 64), 0, st, S, P, op);
}
void launch_sp_noise_mask(hipStream_t st, const SearchDev& S, const SelfPlayDev& P) {
    hipLaunchKernelGGL(k_sp_noise_mask, dim3((S.G + 255) / 256), dim3(256), 0, st, S, P);
}
void launch_sp_pick(hipStream_t st, const SearchDev& S, const SelfPlayDev& P, int32_t* op, bool proof) {
    if (proof) hipLaunchKernelGGL(k_sp_pick<true>, wgrid(S.G), dim3(WPB * 64), 0, st, S, P, op);
    else hipLaunchKernelGGL(k_sp_pick<false>, wgrid(S.G), dim3(WPB * 64), 0, st, S, P, op);
}
void launch_sp_boost_list(hipStream_t st, const SearchDev& S, int boost_plies, int32_t* list, int32_t* count) {
    hipLaunchKernelGGL(k_sp_boost_list, dim3(1), dim3(1024), 0, st, S, boost_plies, list, count);
}
void launch_proof_read(hipStream_t st, const SearchDev& S, uint8_t* root_status, uint8_t* child_status, int32_t* counts) {
    hipLaunchKernelGGL(k_proof_read, dim3(S.G), dim3(64), 0, st, S, root_status, child_status, counts);
}
void launch_sp_count_ply(hipStream_t st, const SelfPlayDev& P) { hipLaunchKernelGGL(k_sp_count_ply, dim3(1), dim3(1), 0, st, P); }

}  // namespace tg
