// tree_pass.cuh — the two device functions every tree kernel is made of, and what they need: the virtual rollout of one leaf
// (select_pass: virtual_rollout + select, mcts.rs:26-65,94-118) and its de-virtualisation (backup_pass: devirtualize_path,
// mcts.rs:67-91), the node pool's take / give, the wave helpers.  tree_kernels.hip wraps the two in its four kernel templates
// (wave → game by identity or through a compacted list, with or without proven values): the same operations on a game's tree in
// the same order from every instantiation, so the trees are the same bit for bit.  search_kernels.hip and symm_kernels.hip use
// the pool and the helpers.
#pragma once
#include <stdlib.h>

#include "board.cuh"
#include "kernels.h"
#include "rng.cuh"
#include "search.cuh"
#include "softmax.cuh"

namespace tg {

#ifndef TG_WPB
#define TG_WPB 4
#endif
constexpr int WPB = TG_WPB;  // waves (games) per block (4: 256 threads; other values: scripts/probes/tree_wpb_probe.sh)

__device__ inline int game_of_wave() { return (int)(blockIdx.x * WPB + (threadIdx.x >> 6)); }
static inline dim3 wgrid(int waves) { return dim3((waves + WPB - 1) / WPB); }  // the grid of a one-wave-per-game launch
__device__ inline void flag(const SearchDev& S, uint32_t bit) { atomicOr(S.err, bit); }
// A game ran into one of the fixed capacities (TG_LIMIT_*, takgpu.h).  Self-play retires that game alone — the bit is kept
// per game, its wave stops touching the tree, and the end of the ply discards its examples and restarts the slot;
// a caller-driven search has nobody to restart the game, so the engine-wide sticky error stays.  Called by the whole wave.
__device__ inline void limit_hit(const SearchDev& S, int g, uint32_t bit) {
    if (S.retire) { if (lane_id() == 0) S.abort[g] = (uint8_t)(S.abort[g] | bit); }
    else flag(S, bit);
}
__device__ inline void wave_sync_mem() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

// The phase stamps of the diagnostic build: tree_kernels.hip defines the macro (and owns the buffer) under -DTG_TREE_STAMPS
// before it includes this file; everywhere else, and in the product build, they are nothing.
#ifndef TG_TSTAMP
#define TG_TSTAMP(g, slot) do { } while (0)
#endif

// ---- node pool (search.cuh): chunks of 2^chunk_shift nodes handed out from a ring of free chunk ids ----
// Take one chunk for the calling wave (wave-uniform result, 0 = pool exhausted).  Only chunks whose return was
// published before this kernel started are handed out, so a taker never reads a ring slot that a concurrent
// pool_give of the same launch has reserved but not yet written.
__device__ inline uint32_t pool_take(const SearchDev& S) {
    uint32_t c = 0;
    if (lane_id() == 0) {
        const unsigned long long h = atomicAdd(&S.pool_ctl[0], 1ull);
        if (h < S.pool_ctl[2]) c = S.free_ring[h % S.n_chunks];
    }
    return uni((uint32_t)__shfl((int)c, 0));
}
// Return every chunk of a game's chain (lane 0 walks it; a chain is a handful to a few hundred chunks, once per move)
__device__ inline void pool_give_chain(const SearchDev& S, uint32_t head) {
    if (lane_id() != 0) return;
    for (uint32_t c = head; c != 0;) {
        const uint32_t next = S.chunk_link[c];
        const unsigned long long t = atomicAdd(&S.pool_ctl[1], 1ull);
        S.free_ring[t % S.n_chunks] = c;
        c = next;
    }
}
__device__ inline uint64_t ws_hash(const WState& s, const Geom& g) {
    // same function of the packed bytes as the CPU statement: stack words, meta bytes, 10 header bytes
    uint64_t h = 0x243F6A8885A308D3ull;
    for (int i = 0; i < g.nsq; i++) h = mix64(h ^ shfl64(s.stack, i)) + (uint64_t)i;
    for (int i = 0; i < g.nsq; i++) {
        uint32_t hh = (uint32_t)__shfl((int)s.height, i), tp = (uint32_t)__shfl((int)s.top, i);
        uint64_t meta = hh | ((hh ? tp : 0u) << 6);
        h = mix64(h ^ (meta << 8) ^ (uint64_t)(i + 1));
    }
    uint64_t a = (uint64_t)g.n | ((uint64_t)s.to_move << 8) | ((uint64_t)(s.ply & 0xffff) << 16) | ((uint64_t)s.ws << 32) |
                 ((uint64_t)s.wc << 40) | ((uint64_t)s.bs << 48) | ((uint64_t)s.bc << 56);
    uint64_t b = ((uint64_t)s.half_komi & 0xff) | ((uint64_t)(s.rev & 0xff) << 8);
    h = mix64(h ^ a);
    h = mix64(h ^ b);
    return h;
}

// update_concrete, mcts.rs:120-124
__device__ inline void update_concrete(NodeHot& h, float reward) {
    float cumulative = h.q * (float)h.visits;
    h.visits += 1;
    h.q = (cumulative + reward) / (float)h.visits;
}

// self-play (k_sp_instant_win, k_sp_pick): reserves the next staging slot of game g and writes header +
// state; returns the slot (or -1)
__device__ inline void stage_example(const SearchDev& S, const SelfPlayDev& P, int g, const WState& s, const Geom& geo,
                                     uint32_t nmoves, int& slot_out) {
    int k = P.st_count[g];
    if (k >= P.max_game_plies) { limit_hit(S, g, ERRF_EXAMPLES); slot_out = -1; return; }
    size_t e = (size_t)g * P.ex_per_game + k;
    ws_store(s, P.st_state + e * geo.bytes, geo);
    if (lane_id() == 0) {
        ExampleRec h;
        h.slot = (int32_t)(S.slot_base + (uint32_t)g);
        h.generation = (int32_t)S.generation[g];
        h.n_moves = (int32_t)nmoves;
        h.result = 0.0f;
        P.st_hdr[e] = h;
        P.st_count[g] = k + 1;
    }
    slot_out = k;
}

// ---- proven values in the tree (the MCTS-solver backup of Winands et al.; no counterpart in the reference) ----
// status of a node from the result nibble of its cold record: 0 = decided for white, 1 = for black, 2 = a draw, 3 = unknown
// (ongoing; an uninitialised child's record is 0 = TG_ONGOING)
constexpr uint32_t PS_DRAW = 2u, PS_UNKNOWN = 3u;
__device__ inline uint32_t proof_status(uint32_t r) {
    return (r == TG_WHITE_ROAD || r == TG_WHITE_FLAT || r == TG_PROVEN_WHITE) ? 0u
         : (r == TG_BLACK_ROAD || r == TG_BLACK_FLAT || r == TG_PROVEN_BLACK) ? 1u
         : (r == TG_DRAW || r == TG_DRAW_REVERSIBLE || r == TG_PROVEN_DRAW) ? PS_DRAW : PS_UNKNOWN;
}
// The rule, for an initialised ongoing node X whose side to move has colour c: some child decided for c → X is TG_PROVEN_c;
// else no child unknown → TG_PROVEN_DRAW if some child is a draw, TG_PROVEN_(opponent of c) otherwise; else nothing.
// Called by the whole wave of game g behind the unwind of a rollout that has just initialised the terminal node at depth `depth`
// (path[d - 1] = the node at depth d, in LDS) with result `res`: walks upward from the leaf's parent.  A child decided for
// the parent's mover decides the parent without a scan; otherwise one lane-strided scan of the parent's children block (cold
// records only).  Stops at the first level that stays unknown.  The parent keeps its child count and its children.
__device__ inline void proof_walk(const SearchDev& S, const int g, const uint32_t root, const uint32_t root_color,
                                  const uint32_t* path, const int depth, const uint32_t res) {
    const int lane = lane_id();
    NodeCold* cold = S.cold;
    uint32_t cst = proof_status(res);  // wave-uniform: status of the child the walk comes from
    uint32_t proven = 0;
    wave_sync_mem();  // the leaf's record was written by lane 0; the scans below read it from every lane
    for (int d = depth - 1; d >= 0 && cst != PS_UNKNOWN; d--) {
        const uint32_t x = uni(d == 0 ? root : path[d - 1]);
        const uint32_t c = root_color ^ (uint32_t)(d & 1);
        const NodeCold xc = cold[x];
        const uint32_t xn = uni((uint32_t)xc.nres), xb = uni(xc.child);
        if ((xn >> 12) != TG_ONGOING) break;  // (cannot be: the descent went through it)
        uint32_t code = 0;
        if (cst == c) code = c == 0 ? TG_PROVEN_WHITE : TG_PROVEN_BLACK;
        else {
            const uint32_t nchild = xn & 0xfffu;
            bool unk = false, win = false, drw = false;
            for (uint32_t i = lane; i < nchild; i += 64) {
                const uint32_t st = proof_status((uint32_t)cold[xb + i].nres >> 12);
                unk |= st == PS_UNKNOWN; win |= st == c; drw |= st == PS_DRAW;
            }
            if (__ballot(win)) code = c == 0 ? TG_PROVEN_WHITE : TG_PROVEN_BLACK;
            else if (!__ballot(unk)) code = __ballot(drw) ? TG_PROVEN_DRAW : (c == 0 ? TG_PROVEN_BLACK : TG_PROVEN_WHITE);
        }
        if (code == 0) break;
        if (lane == 0) cold[x].nres = (uint16_t)((xn & 0xfffu) | (code << 12));
        proven++;
        cst = proof_status(code);
        wave_sync_mem();  // the next level's scan reads this record
    }
    if (proven && lane == 0)
        __hip_atomic_fetch_add(&S.counters[2 * (size_t)S.G + 2 * (size_t)g], (unsigned long long)proven, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ------------------------------------------------------------------------------------------------
// virtual_rollout (+ select): descend, expand the first uninitialised node, mark the path with a
// virtual visit (or back a concrete result up when the rollout ends on a terminal node), and leave
// the leaf encoded in the network input batch.
// ------------------------------------------------------------------------------------------------
// NB: board size as a compile-time constant (5, 6; 0 = read S.n).  With n known the geometry masks fold to immediates and the
// many divisions by n / n² of move generation, play and the encoder become multiply-shifts instead of ≈ 20-instruction
// software divisions — the tree kernels are bound by vector issue, so this is time.
// What the fused kernel loads of the root BEFORE the backup runs (none of it is written by the backup), so that the select does
// not start with a chain of dependent loads: the root's index, packed state and cold record; `hot_known`: the backup also handed
// over the root's (visits, virtual) as it left them.
struct RootPre {
    bool on = false, hot_known = false;
    uint32_t root = 0, vis = 0, vv = 0;
    NodeCold cold;
    WRaw raw;  // the packed root position as requested (ws_load_raw); unpacked by the select
    uint32_t alive_v = 1, abort_v = 0;  // S.alive[g], S.abort[g] (neither changes between the request and the select)
};

// LIST: the wave serves an entry of a compacted list of games (tree_kernels.hip): everything of the tree and the game
// is game g's, the leaf slot is the LIST POSITION w's — w·batch + p — so that the network sees a dense batch of the listed games.
// PROOF: the MCTS-solver backup (tg_search_set_proof): a rollout that has just initialised a terminal
// node draws the conclusion for its ancestors (proof_walk above), a rollout that ends on a proven node backs its colour up like
// a terminal's.  false: none of it is compiled.
template <int NB, bool LIST = false, bool PROOF = false>
__device__ __forceinline__ void select_pass(const SearchDev& S, const uint8_t* __restrict__ active, const int g, const int pass,
                                            uint32_t* path, uint16_t* mvl, const RootPre& pre = RootPre(), const int w = 0) {
    const int lane = lane_id();
    // leaf slot of this pass: `batch` virtual rollouts per tree and iteration (Player's batching, player.rs:77-93), pass p
    // writing slot g·batch + p
    const size_t slot = (size_t)(LIST ? w : g) * (size_t)S.batch + (size_t)pass;
    {
        // (both flags and the game's allocation cursor are requested together; read one after the other behind `||` they were
        // two round trips in a row in front of the descent)
        const uint32_t alive_v = pre.on ? pre.alive_v : (uint32_t)S.alive[g];
        const uint32_t abort_v = pre.on ? pre.abort_v : (uint32_t)S.abort[g];
        if (!uni(alive_v) || (active && !active[g]) || (S.retire && uni(abort_v))) {
            if (lane == 0) S.leaf_kind[slot] = 0;
            return;
        }
    }
    // the open chunk of the game's node allocation, needed only if this descent expands a leaf: requested now, it is there by then
    const uint32_t alloc_a = S.alloc[2 * g], alloc_e = S.alloc[2 * g + 1];
    const Geom geo = make_geom(NB ? NB : S.n);
    WState s;
    if (pre.on) ws_unpack(s, pre.raw, geo);
    else ws_load(s, S.root_state + (size_t)g * geo.bytes, geo);
    NodeHot* hot = S.hot;
    NodeCold* cold = S.cold;
    const uint32_t root = pre.on ? pre.root : uni(S.root[g]);
    const uint32_t root_color = s.to_move;
    uint32_t node = root;
    int depth = 0;
    uint32_t res = TG_ONGOING;
    bool terminal = false;
    bool fresh = false;  // (PROOF) the rollout ended by initialising its node, not on a known one

    // The (visits, virtual, child, n|result) of the node being visited travel in registers: they are read
    // once for the root and afterwards come out of the children scan of the level above, so each level
    // costs ONE dependent memory round trip (the coalesced hot + cold records of all children).
    uint32_t vis, vv, nres, cbase;
    {
        NodeCold nc = pre.on ? pre.cold : cold[root];
        nres = uni((uint32_t)nc.nres); cbase = uni(nc.child);
        if (pre.on && pre.hot_known) { vis = pre.vis; vv = pre.vv; }
        else { NodeHot nh = hot[root]; vis = uni(nh.visits); vv = uni(nh.virt); }
    }
    TG_TSTAMP(g, 4);  // root state + root record loaded
    // The records of the first 64 children of the node about to be visited are requested as soon as its children block is
    // known — for the root here, for every later level right before the move is played on the wave's position — so that the
    // round trip of the children scan passes under ws_play instead of after it.
    NodeHot pf_h, pf_h2;   // children lane and lane + 64 (the opening's 70-odd placements do not fit one round of the scan)
    NodeCold pf_c, pf_c2;
    pf_h.prior = 0.0f; pf_h.q = 0.0f; pf_h.visits = 0; pf_h.virt = 0;
    pf_c.child = 0; pf_c.mv = 0; pf_c.nres = 0;
    pf_h2 = pf_h; pf_c2 = pf_c;
    float c_pf = 0.0f;  // exploration_rate(visits + virtual) of the node about to be visited (mcts.rs:10-12), from the table
    auto prefetch_children = [&]() {
        // (a vector load of one address: it returns with the children's records instead of on the scalar path in front of them)
        const uint32_t tn = vis + vv;
        c_pf = S.ctab[tn < (uint32_t)S.ctab_size ? tn : (uint32_t)S.ctab_size - 1u];
        if ((vis | vv) != 0u && (nres >> 12) == TG_ONGOING && (uint32_t)lane < (nres & 0xfffu)) {
            pf_h = hot[cbase + (uint32_t)lane];
            pf_c = cold[cbase + (uint32_t)lane];
            if ((uint32_t)lane + 64u < (nres & 0xfffu)) {
                pf_h2 = hot[cbase + (uint32_t)lane + 64u];
                pf_c2 = cold[cbase + (uint32_t)lane + 64u];
            }
        }
    };
    prefetch_children();
    for (;;) {
        if (vis == 0 && vv == 0) {
            // uninitialised node: initialise it and stop (mcts.rs:41-53)
            TG_TSTAMP(g, 24);  // descent done
            res = ws_result(s, geo);
            TG_TSTAMP(g, 25);
            uint32_t count = 0, cb = 0;
            if (res == TG_ONGOING) {
                // the legal moves are staged in LDS so that the children block can be placed once its size is known
                count = (uint32_t)ws_movegen(s, geo, EX_MOVES, [&](int idx, uint32_t code) { mvl[idx] = (uint16_t)code; });
                TG_TSTAMP(g, 26);
                if (count > (uint32_t)EX_MOVES) {
                    limit_hit(S, g, ERRF_MOVES);
                    if (lane == 0) S.leaf_kind[slot] = 0;
                    return;
                }
                uint32_t a = uni(alloc_a), end = uni(alloc_e);
                if (a + count > end) {  // the block does not fit into the game's open chunk: take the next one
                    const uint32_t c = pool_take(S);
                    if (c == 0) {
                        flag(S, ERRF_ARENA);
                        if (lane == 0) S.leaf_kind[slot] = 0;
                        return;
                    }
                    a = c << S.chunk_shift;
                    end = a + (1u << S.chunk_shift);
                    if (lane == 0) {
                        S.chunk_link[c] = S.chunk_head[g];
                        S.chunk_head[g] = c;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                const float temp_policy = 1.0f / (float)count;
                bool bad = false;
                for (uint32_t i = lane; i < count; i += 64) {
                    NodeCold cc;
                    cc.child = 0; cc.mv = mvl[i]; cc.nres = 0;
                    cold[a + i] = cc;
                    NodeHot c;
                    c.prior = temp_policy; c.q = 0.0f; c.visits = 0; c.virt = 0;
                    hot[a + i] = c;
                    // the child's policy index now, while its move is at hand (move_index, move_map.rs:19-48): the backup of this
                    // leaf gathers the network's output by it
                    const int idx = move_index_dev((uint32_t)mvl[i], NB ? NB : S.n, S.legacy5 != 0, S.lut5);
                    const bool ok = idx >= 0 && idx < S.P;
                    bad |= !ok;
                    S.child_pidx[slot * EX_MOVES + i] = ok ? (uint16_t)idx : (uint16_t)0xFFFF;
                }
                if (__ballot(bad)) flag(S, ERRF_MOVE);  // "could not map turn to index" (move_map.rs:24)
                cb = a;
                if (lane == 0) { S.alloc[2 * g] = a + count; S.alloc[2 * g + 1] = end; }
            }
            if (lane == 0) {
                cold[node].child = cb;
                cold[node].nres = (uint16_t)(count | (res << 12));
                S.leaf_rec[2 * slot] = cb;
                S.leaf_rec[2 * slot + 1] = count;
            }
            terminal = res != TG_ONGOING;
            fresh = true;
            TG_TSTAMP(g, 27);  // children created
            break;
        }
        res = nres >> 12;
        if (res != TG_ONGOING) { terminal = true; break; }  // known terminal node: same result again (mcts.rs:35-38)
        // ---- select, mcts.rs:94-118 ----
        const uint32_t nchild = nres & 0xfffu;
        const uint32_t nsum = vis + vv;
        const float visit_count = (float)nsum;
        uint32_t ti = nsum;
        if ((int)ti >= S.ctab_size) {
            limit_hit(S, g, ERRF_CTAB);
            if (S.retire) {  // nothing of this rollout has touched the tree yet (virtual visits are marked in the unwind)
                if (lane == 0) S.leaf_kind[slot] = 0;
                return;
            }
            ti = (uint32_t)S.ctab_size - 1;
        }
        const float c_rate = c_pf;  // = S.ctab[ti], requested with the children
        const float root_n = sqrtf(visit_count);
        float best = -INFINITY;
        int best_i = -1;
        bool nan = false;
        NodeHot bh;      // records of this lane's best child
        NodeCold bc;
        bh.prior = 0.0f; bh.q = 0.0f; bh.visits = 0; bh.virt = 0;
        bc.child = 0; bc.mv = 0; bc.nres = 0;
        for (uint32_t i = lane; i < nchild; i += 64) {
            NodeHot ch;
            NodeCold cc;
            if (i == (uint32_t)lane) { ch = pf_h; cc = pf_c; }  // the first 128 children were requested a level ago
            else if (i == (uint32_t)lane + 64u) { ch = pf_h2; cc = pf_c2; }
            else { ch = hot[cbase + i]; cc = cold[cbase + i]; }
            float cn = (float)(ch.visits + ch.virt);
            float qv = (ch.visits | ch.virt) ? (ch.q * (float)ch.visits - (float)ch.virt) / cn : 0.0f;
            float u = qv + c_rate * ch.prior * (root_n / (1.0f + cn));
            if (u != u) nan = true;
            if (u >= best) { best = u; best_i = (int)i; bh = ch; bc = cc; }
        }
        // the wave's best (value, index): the largest pair under (value, then index) — `max_by` keeps the LAST maximum
        // (mcts.rs:107-117).  Six DPP steps (row_shr 1, 2, 4, 8, row_bcast15, row_bcast31: an inclusive max-scan whose lane 63
        // holds the total) instead of six butterfly rounds of two ds_bpermute each — 12 trips through the LDS crossbar, one after
        // the other, at every level of every descent.  The order of a total order's maximum does not matter: same winner.
        float wb = best;
        int wi = best_i;
#define TG_ARGMAX_STEP(CTRL, ROWS)                                                                                               \
        {                                                                                                                        \
            const float ob = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(-INFINITY), __float_as_int(wb), CTRL, ROWS, 0xf, false)); \
            const int oi = __builtin_amdgcn_update_dpp(-1, wi, CTRL, ROWS, 0xf, false);                                        \
            if (ob > wb || (ob == wb && oi > wi)) { wb = ob; wi = oi; }                                                          \
        }
        TG_ARGMAX_STEP(0x111, 0xf) TG_ARGMAX_STEP(0x112, 0xf) TG_ARGMAX_STEP(0x114, 0xf) TG_ARGMAX_STEP(0x118, 0xf)
        TG_ARGMAX_STEP(0x142, 0xa) TG_ARGMAX_STEP(0x143, 0xc)
#undef TG_ARGMAX_STEP
        wb = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wb), 63));
        wi = __builtin_amdgcn_readlane(wi, 63);
        if (__ballot(nan)) flag(S, ERRF_NAN);
        if (wi < 0) {  // cannot happen for a consistent tree; never index out of the arena
            flag(S, ERRF_NAN);
            if (lane == 0) S.leaf_kind[slot] = 0;
            return;
        }
        // the winning lane (the one whose own best is the wave's best) hands its child's records down
        const int src = __builtin_ctzll(__ballot(best_i == wi));
        const uint32_t chosen = cbase + (uint32_t)wi;
        const uint32_t mv = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bc.mv, src);  // (v_readlane: no LDS round trip)
        vis = (uint32_t)__builtin_amdgcn_readlane((int)bh.visits, src);
        vv = (uint32_t)__builtin_amdgcn_readlane((int)bh.virt, src);
        nres = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bc.nres, src);
        cbase = (uint32_t)__builtin_amdgcn_readlane((int)bc.child, src);
        TG_TSTAMP(g, 5 + 2 * (depth < 9 ? depth : 9));  // children scanned, best child known
        prefetch_children();  // of the chosen child, under the play of its move
        ws_play(s, mv, geo);
        TG_TSTAMP(g, 6 + 2 * (depth < 9 ? depth : 9));  // move played
        if (depth >= MAX_DEPTH) {
            limit_hit(S, g, ERRF_DEPTH);
            if (lane == 0) S.leaf_kind[slot] = 0;
            return;
        }
        if (lane == 0) path[depth] = chosen;
        depth++;
        node = chosen;
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // ---- unwind (mcts.rs:55-62): lane d handles the node at depth d ----
    const bool winner = (res >= TG_WHITE_ROAD && res <= TG_BLACK_FLAT) || (PROOF && (res == TG_PROVEN_WHITE || res == TG_PROVEN_BLACK));
    const uint32_t wcolor = (res == TG_WHITE_ROAD || res == TG_WHITE_FLAT || (PROOF && res == TG_PROVEN_WHITE)) ? 0u : 1u;
    for (int d = lane; d <= depth; d += 64) {
        uint32_t nd = d == 0 ? root : path[d - 1];
        if (!terminal && S.batch == 1) {
            // virtual_visits += 1 as a returnless atomic: nothing to wait for (the record's load and store were a round trip
            // in front of the leaf's stores); the tree belongs to this wave alone.  Only with one rollout per launch: the atomic
            // is performed in L2, and a second pass of the same wave would read the record through its L1
            __hip_atomic_fetch_add(&hot[nd].virt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            NodeHot h = hot[nd];
            if (terminal) {
                uint32_t curr = root_color ^ (uint32_t)(d & 1);
                float reward = winner ? (wcolor == curr ? -1.0f : 1.0f) : 0.0f;
                update_concrete(h, reward);
            } else {
                h.virt += 1;
            }
            hot[nd] = h;
        }
    }
    TG_TSTAMP(g, 28);  // virtual visits marked
    if constexpr (PROOF) {
        if (terminal && fresh) proof_walk(S, g, root, root_color, path, depth, res);
        else if (terminal && res >= TG_PROVEN_WHITE && lane == 0)  // the descent ended on a proven node
            __hip_atomic_fetch_add(&S.counters[2 * (size_t)S.G + 2 * (size_t)g + 1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    uint32_t* gpath = S.path + slot * MAX_DEPTH;
    for (int d = lane; d < depth; d += 64) gpath[d] = path[d];
    if (!terminal) {
        if (S.evaluator == TG_EVAL_RESNET) {
            if (S.planes) ws_encode<true>(s, geo, S.planes + slot * geo.nsq * S.cin_pad, S.cin_pad);
            else ws_store(s, S.leaf_state + slot * geo.bytes, geo);  // game_repr happens inside the fused tower
        }
        else if (S.evaluator == TG_EVAL_HASH) {
            uint64_t h = ws_hash(s, geo);
            if (lane == 0) S.leaf_hash[slot] = h;
        }
    }
    TG_TSTAMP(g, 29);  // leaf state stored
    if (lane == 0) {
        S.path_len[slot] = depth;
        S.leaf_kind[slot] = terminal ? 2 : 1;
        __hip_atomic_fetch_add(&S.counters[2 * (size_t)g], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (returnless: no round trip)
        if (!terminal) __hip_atomic_fetch_add(&S.counters[2 * (size_t)g + 1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------
// devirtualize_path, mcts.rs:67-91: real priors for the leaf's children, value backed up with
// alternating sign, virtual visits removed.
// ------------------------------------------------------------------------------------------------
// Every load that does not depend on another load is issued first (leaf kind, path length, the leaf's children block and their
// policy indices — both recorded by the select that expanded it —, the FC's softmax statistics, the value logit, this lane's
// path entry); the second round is the gather of the children's logits and the path nodes' records; then the stores.  Round 2
// walked path → leaf → children's moves → index table → logits, five dependent round trips (19 k of the wave's 56 k cycles).
// Returns through `pre` the root's (visits, virtual) as this backup leaves them, for the select that follows in the same launch.
// `g` only names the leaf slots (g·batch + pass); the tree comes in through root_v.  The list-mapped kernels pass the list position.
template <int NB>
__device__ __forceinline__ void backup_pass(const SearchDev& S, const int g, const int pass, const uint32_t root_v, RootPre* pre = nullptr) {
    const size_t slot = (size_t)g * (size_t)S.batch + (size_t)pass;
    const int lane = lane_id();
    NodeHot* hot = S.hot;
    const uint32_t* path = S.path + slot * MAX_DEPTH;
    const float* lrow = S.logits ? S.logits + slot * (size_t)S.logit_ld : nullptr;
    const float* pol = S.policy + slot * S.P;
    const uint16_t* pidx = S.child_pidx + slot * EX_MOVES;
    // round 1 — every load whose address does not come out of another load, requested back to back and unconditionally (all
    // addresses are valid whatever the slot holds; the wave-uniform values are made scalar only after the last request): the
    // leaf's kind, path length and children block, this lane's child index and path entry, the statistics, the value logit
    const uint32_t kind_v = (uint32_t)S.leaf_kind[slot];
    const uint32_t len_v = (uint32_t)S.path_len[slot];
    const uint32_t cb_v = S.leaf_rec[2 * slot], n_v = S.leaf_rec[2 * slot + 1];
    const uint32_t raw_idx = (uint32_t)pidx[lane], raw_idx2 = (uint32_t)pidx[lane + 64];  // (EX_MOVES ≥ 128 entries per slot)
    const uint32_t raw_nd = path[lane ? lane - 1 : 0];
    // round 4: the policy FC's epilogue has already picked the children's logits out of its accumulators (child_logit, in child
    // order): two coalesced loads in THIS round replace the dependent gather logits[pidx[child]] of round 2, and the value
    // pre-activation comes with the statistics record
    const float* clog = S.child_logit ? S.child_logit + slot * EX_MOVES : nullptr;
    const float clog_v = clog ? clog[lane] : 0.0f, clog_v2 = clog ? clog[lane + 64] : 0.0f;
    const float vlogit_v = (S.evaluator == TG_EVAL_RESNET && lrow && !clog) ? lrow[S.P] : 0.0f;
    // root_v = S.root[g] as the caller requested it, not yet waited for: it was the first request, so making it scalar here
    // waits for that one load alone, and the select's cold record of the root joins the requests above
    const uint32_t root = uni(root_v);
    if (pre) { pre->root = root; pre->cold = S.cold[root]; }
    const bool live = uni(kind_v) == 1u;
    const int L = (int)uni(len_v);
    const uint32_t cb = uni(cb_v), nchild = uni(n_v);
    float e;
    uint64_t hsh = 0;
    float lmx = 0.0f, linv = 0.0f;
    if (S.evaluator == TG_EVAL_RESNET && lrow) {
        float vlogit = vlogit_v;
        if (S.fc_stats)  // one 8-byte load per lane instead of the whole row
            fc_combine_stats(S.fc_stats + (size_t)uni((uint32_t)slot) * (size_t)S.fc_stride * 2, S.fc_blocks, lmx, linv, clog ? &vlogit : nullptr);
        else if (live) softmax_stats_wave(lrow, S.P, lmx, linv);
        e = tanhf(vlogit);
    } else if (S.evaluator == TG_EVAL_RESNET) e = S.eval[slot];
    else if (S.evaluator == TG_EVAL_HASH) { hsh = S.leaf_hash[slot]; e = hash_eval(hsh); }
    else e = 0.0f;
    if (!live) return;  // (terminal leaf: backed up concretely by the select; skipped game)
    const uint32_t my_idx = (uint32_t)lane < nchild ? raw_idx : 0xFFFFu;
    const uint32_t my_nd = lane == 0 ? root : raw_nd;
    TG_TSTAMP(g, 1);  // independent loads done
    // round 2: priors of the leaf's children (devirtualize_path, mcts.rs:80-84)
    bool bad = false;
    for (uint32_t i = lane; i < nchild; i += 64) {
        const uint32_t idx = i == (uint32_t)lane ? my_idx : i == (uint32_t)lane + 64u ? raw_idx2 : (uint32_t)pidx[i];
        float p;
        if (idx == 0xFFFFu) { bad = true; p = 0.0f; }
        else if (S.evaluator == TG_EVAL_RESNET) {
            if (clog) p = stat_exp((i == (uint32_t)lane ? clog_v : i == (uint32_t)lane + 64u ? clog_v2 : clog[i]) - lmx) * linv;
            else p = !lrow ? pol[idx] : S.fc_stats ? stat_exp(lrow[idx] - lmx) * linv : expf(lrow[idx] - lmx) * linv;
        }
        else if (S.evaluator == TG_EVAL_HASH) p = hash_policy(hsh, idx);
        else p = 1.0f;
        hot[cb + i].prior = p;
    }
    if (__ballot(bad)) flag(S, ERRF_MOVE);
    TG_TSTAMP(g, 2);  // priors written
    uint32_t rv = 0, rvv = 0;
    for (int d = lane; d <= L; d += 64) {
        uint32_t nd = d == lane ? my_nd : path[d - 1];
        NodeHot h = hot[nd];
        h.virt -= 1;
        float ev = ((L - d) & 1) ? e : -e;  // the leaf sees -eval, its parent +eval, …
        update_concrete(h, ev);
        // the prior of this node may just have been rewritten above only if it is a child of the leaf,
        // which it is not (it lies on the path), so writing the whole record back is safe
        hot[nd].q = h.q;
        hot[nd].visits = h.visits;
        hot[nd].virt = h.virt;
        if (d == 0) { rv = h.visits; rvv = h.virt; }
    }
    if (pre) {  // lane 0 handled the root (d = 0)
        pre->vis = uni(rv);
        pre->vv = uni(rvv);
        pre->hot_known = true;
    }
}

}  // namespace tg
