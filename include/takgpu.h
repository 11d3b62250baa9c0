/*
 * takgpu.h — C ABI of libtakgpu.so, the MI355X (gfx950) batched Tak self-play engine.
 *
 * This is the drop-in boundary for the ONE hot path of ViliamVadocz/tak: batched AlphaZero
 * self-play (board move-gen / step / terminal / encode, policy-value resnet forward, MCTS).
 * Every entry point names the reference interface it replaces (paths relative to the
 * reference repo).  Plain pointers and sizes only; no torch / tch types cross this line.
 *
 * Conventions
 *   - every function returns TG_OK (0) or a negative TgStatus; tg_last_error() gives the
 *     thread-local message of the last failure.  Nothing aborts, nothing throws.
 *   - "host" entry points take host pointers, do H2D, run the HIP kernels, D2H, and
 *     synchronise before returning.  "_dev" entry points take device pointers that must stay
 *     valid until the engine's stream is synchronised (tg_sync) and do not synchronise.
 *   - the caller owns every buffer it passes; the engine never frees caller memory.
 *   - one engine handle per GPU / per process; calls on one handle must be serialised by the
 *     caller (same contract as `&NET` in reference train/src/self_play.rs:96).
 *   - there is NO CPU fallback: if no HIP device is present every compute entry point fails
 *     with TG_ERR_NO_DEVICE.
 */
#ifndef TAKGPU_H
#define TAKGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TG_ABI_VERSION 5

/* The library is built with -fvisibility=hidden: the entry points below are ALL it exports. */
#if defined(__GNUC__) || defined(__clang__)
#define TG_API __attribute__((visibility("default")))
#else
#define TG_API
#endif

/* ---------------------------------------------------------------------------------------
 * Status codes.  TG_PLAY_* mirror reference tak/src/error.rs:4-15 (PlayError) and
 * :55-58 / :72-76 (StackError / TakeError) one to one.
 * ------------------------------------------------------------------------------------- */
typedef enum TgStatus {
    TG_OK = 0,
    TG_ERR_INVALID_ARG = -1,
    TG_ERR_NO_DEVICE = -2,
    TG_ERR_HIP = -3,
    TG_ERR_WEIGHTS = -4,       /* missing / wrongly sized tensor at tg_net_finalize            */
    TG_ERR_ARENA_OVERFLOW = -5,/* the MCTS node pool is exhausted (TgSearchConfig.arena_nodes)     */
    TG_ERR_NAN = -6,           /* reference panics "tried comparing nan" (search/mcts.rs:110)   */
    TG_ERR_STATE = -7,         /* call sequence violated (e.g. search before weights)          */
    TG_ERR_ILLEGAL_MOVE = -8,  /* a move in a batch failed; per-item code in the status array  */
    TG_ERR_LIMIT = -9          /* one of the fixed capacities below (TG_LIMIT_*) was exceeded      */
} TgStatus;

/* Fixed capacities of the search / self-play engine (the reference's heap structures have none).
 * Self-play (tg_selfplay_*): a game that exceeds one is RETIRED — its staged examples are discarded, its slot restarts a
 * fresh game (next generation, as after a finished game), TgSelfPlayStats.aborted_games counts it — and every other game
 * keeps running: one runaway game does not stop the other 4095.
 * Caller-driven search (tg_search_run: Player, pit): exceeding one sets a sticky error on the engine (TG_ERR_LIMIT from
 * the next polling call) until tg_search_reset / tg_search_create / tg_selfplay_create. */
#define TG_LIMIT_DEPTH 256          /* longest selection path (plies below the root)                     */
#define TG_LIMIT_VISITS (1 << 22)   /* visits + virtual visits of one node (exploration-rate table)      */
#define TG_LIMIT_GAME_PLIES 512     /* examples staged per self-play game = plies of one game            */
/* The move-list capacity TG_MAX_MOVES (512, below) is one of these capacities wherever a list is staged: a position INSIDE a search
 * tree (a node the selection expands, a root the self-play driver scans for an instant win) with more legal moves is treated as the
 * three above — the game retired in self-play, the sticky TG_ERR_LIMIT in a caller-driven search and in tg_reanalyse.  A position a
 * caller HANDS IN with a longer list (tg_movegen, tg_solve, a frontier of tg_perft at depth >= 2) is TG_ERR_INVALID_ARG; inside the
 * forced-win solver a longer list is a give-up (tg_solve below).  Such positions exist: on 6x6 eight stacks of six stones topped by
 * the mover in the interior give 1076 moves, on 5x5 eight stacks of five give 531.  Ordinary play is not known to reach them. */

typedef enum TgPlayError { /* per-item result of tg_play, 0 = Ok(()) */
    TG_PLAY_OK = 0,
    TG_PLAY_OUT_OF_BOUNDS = 1,
    TG_PLAY_ALREADY_OCCUPIED = 2,
    TG_PLAY_NO_CAPSTONE = 3,
    TG_PLAY_NO_STONES = 4,
    TG_PLAY_OPENING_NON_FLAT = 5,
    TG_PLAY_EMPTY_SQUARE = 6,
    TG_PLAY_STACK_NOT_OWNED = 7,
    TG_PLAY_STACK_WALL = 8,      /* StackError::Wall  */
    TG_PLAY_STACK_CAP = 9,       /* StackError::Cap   */
    TG_PLAY_TAKE_ZERO = 10,      /* TakeError::Zero   */
    TG_PLAY_TAKE_CARRY_LIMIT = 11,
    TG_PLAY_TAKE_STACK_SIZE = 12,
    TG_PLAY_SPREAD_OUT_OF_BOUNDS = 13
} TgPlayError;

/* reference tak/src/game_result.rs:3-8 (GameResult) flattened to one byte */
typedef enum TgResult {
    TG_ONGOING = 0,
    TG_WHITE_ROAD = 1,
    TG_WHITE_FLAT = 2,
    TG_BLACK_ROAD = 3,
    TG_BLACK_FLAT = 4,
    TG_DRAW = 5,            /* Draw { reversible_plies: false } */
    TG_DRAW_REVERSIBLE = 6  /* Draw { reversible_plies: true }  */
} TgResult;

/* ---------------------------------------------------------------------------------------
 * Packed game state (replaces the non-POD `Game<N>` of reference tak/src/game.rs:24-35,
 * `Board<N>` board.rs:7-10 and `Tile` tile.rs:6-10).
 *
 * Square index sq = row * N + col (row = y, col = x, same as board.rs:24-27 data[y][x]).
 * stack[sq]: colours bottom→top, bit i = colour of the i-th stone from the bottom,
 *            0 = white, 1 = black; bits ≥ height are zero.  Max height 2·(stones+caps) ≤ 62.
 * meta[sq]:  bits 0..5 = height (number of stones), bits 6..7 = piece type of the TOP stone
 *            (0 flat, 1 wall, 2 cap); 0 when the square is empty (Tile::default()).
 * Two layouts: N ≤ 5 → TgState5 (256 B, 25 slots; for N < 5 only the first N·N are used),
 *              N = 6 → TgState6 (384 B, 36 slots).  tg_state_bytes(N) tells which.
 * Within a state the fields are arrays over squares (SoA): a 64-lane wavefront loads one
 * game with lane = square, fully coalesced.
 * ------------------------------------------------------------------------------------- */
typedef struct TgHeader {
    uint8_t n;                 /* board size 3..6                                      */
    uint8_t to_move;           /* 0 white, 1 black (Game::to_move)                     */
    uint16_t ply;
    uint8_t white_stones, white_caps, black_stones, black_caps;
    int8_t half_komi;
    uint8_t reversible_plies;
    uint8_t reserved[6];
} TgHeader; /* 16 bytes */

typedef struct TgState5 {
    uint64_t stack[25];
    uint8_t meta[25];
    uint8_t pad[15];
    TgHeader h;
} TgState5; /* 256 bytes */

typedef struct TgState6 {
    uint64_t stack[36];
    uint8_t meta[36];
    uint8_t pad[44];
    TgHeader h;
} TgState6; /* 384 bytes */

#define TG_STATE5_BYTES 256
#define TG_STATE6_BYTES 384
#define TG_META(height, top) ((uint8_t)((height) | ((top) << 6)))
#define TG_META_HEIGHT(m) ((m) & 63)
#define TG_META_TOP(m) ((m) >> 6)

/* size in bytes of one packed state for board size n (256 for n ≤ 5, 384 for n = 6) */
TG_API size_t tg_state_bytes(int n);

/* ---------------------------------------------------------------------------------------
 * Move code (replaces takparse 0.5.5 `Move{square, kind}`; reference call sites
 * tak/src/game.rs:121-125, move_gen.rs:19-75):
 *   bits  0..5   square index row*N+col
 *   bits  6..7   place: piece (0 flat, 1 wall, 2 cap);  spread: direction
 *                (0 Up=row+1 '+', 1 Down=row-1 '-', 2 Left=col-1 '<', 3 Right=col+1 '>')
 *   bits  8..15  0 for a placement; for a spread the 8-bit drop pattern, MSB first, one bit
 *                per carried stone in drop order, 1 = this stone is the last one dropped on
 *                its square (so popcount = squares covered, 8 - ctz = stones picked up).
 *                drops [2,1] → 0b0110_0000.  (takparse `Pattern::mask()` layout as used by
 *                reference alpha-tak/src/search/move_map.rs:35; see DESIGN.md "unpinned".)
 * ------------------------------------------------------------------------------------- */
typedef uint16_t TgMove;
#define TG_MAX_MOVES 512 /* capacity of one move list in tg_movegen */

/* ---------------------------------------------------------------------------------------
 * Engine
 * ------------------------------------------------------------------------------------- */
typedef struct TgEngine TgEngine;

typedef enum TgPolicyHead {
    TG_HEAD_FC5 = 0,  /* Net5: Linear(F*25 → 1575), legacy move LUT (net5.rs:56-61, move_map.rs:21-24) */
    TG_HEAD_CONV = 1  /* Net6: conv3x3(F → 3+4(2^N-2)), index ch*N²+row*N+col (net6.rs:56, move_map.rs:26-46) */
} TgPolicyHead;

typedef enum TgEvaluator {
    TG_EVAL_RESNET = 0, /* the policy/value resnet (needs weights)                           */
    TG_EVAL_DUMMY = 1,  /* DummyNet of alpha-tak/src/search/tests.rs:29-34: policy 1.0, eval 0 */
    TG_EVAL_HASH = 2    /* test evaluator: deterministic pseudo-random policy/eval from the state */
} TgEvaluator;

typedef struct TgConfig {
    int32_t abi_version;   /* TG_ABI_VERSION */
    int32_t device;        /* HIP device ordinal */
    int32_t board_size;    /* 3..6 */
    int32_t res_blocks;    /* RES_BLOCKS (net5.rs:16 / net6.rs:16), runtime here */
    int32_t filters;       /* FILTERS (net5.rs:17), multiple of 32 */
    int32_t policy_head;   /* TgPolicyHead */
    int32_t evaluator;     /* TgEvaluator */
    int32_t max_batch;     /* largest n passed to tg_policy_eval / number of concurrent games */
} TgConfig;

TG_API int tg_engine_create(const TgConfig* cfg, TgEngine** out);
TG_API void tg_engine_destroy(TgEngine* e);
TG_API const char* tg_last_error(void);
TG_API int tg_sync(TgEngine* e);
/* the hipStream_t the engine launches on (as void*), for callers timing with HIP events */
TG_API void* tg_stream(TgEngine* e);

/* Which card the engine runs on, as the HIP runtime names it — so that a multi-process launch (one rank per GPU, reference
 * train/src/self_play.rs:98,102-104: one shard per process) can show that its N ranks sat on N DISTINCT devices: two ranks that
 * were handed the same card report the same pci_bus_id. */
typedef struct TgDeviceInfo {
    int32_t hip_device;     /* TgConfig.device: the ordinal inside this process (after HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES) */
    int32_t cu_count;       /* hipDeviceProp_t.multiProcessorCount: 256 on an MI355X                              */
    int32_t clock_khz;      /* hipDeviceProp_t.clockRate                                                           */
    int32_t reserved;
    uint64_t total_mem;     /* bytes of device memory                                                              */
    char pci_bus_id[32];    /* hipDeviceGetPCIBusId: "domain:bus:device.function"                                   */
    char name[128];         /* hipDeviceProp_t.name                                                                 */
    char arch[64];          /* hipDeviceProp_t.gcnArchName, e.g. "gfx950:sramecc+:xnack-"                          */
} TgDeviceInfo;
TG_API int tg_device_info(TgEngine* e, TgDeviceInfo* out);

/* sizes — reference alpha-tak/src/repr/game.rs:12-15 (input_channels) and repr/moves.rs:6-31
 * (possible_moves / output_size).  policy_size depends on the head. */
TG_API int tg_input_channels(int n);
TG_API int tg_policy_size(int n, int policy_head);

/* ---------------------------------------------------------------------------------------
 * Board operators on batches (host buffers).  `states` is n packed states of
 * tg_state_bytes(board_size) each.
 * ------------------------------------------------------------------------------------- */

/* Game::possible_moves (tak/src/move_gen.rs:7-30), same order.  moves: n*TG_MAX_MOVES codes,
 * counts: n.  A position with more than TG_MAX_MOVES moves yields TG_ERR_INVALID_ARG. */
TG_API int tg_movegen(TgEngine* e, int n, const void* states, TgMove* moves, int32_t* counts);

/* Game::play (tak/src/game.rs:121-130) in place; status[i] = TgPlayError.  Returns
 * TG_ERR_ILLEGAL_MOVE if any item failed (failed items are left unchanged — the behaviour of
 * Game::safe_play, game.rs:136-145). */
TG_API int tg_play(TgEngine* e, int n, void* states, const TgMove* moves, uint8_t* status);

/* Game::result (tak/src/game.rs:220-267); results[i] = TgResult */
TG_API int tg_result(TgEngine* e, int n, const void* states, uint8_t* results);

/* game_repr (alpha-tak/src/repr/game.rs:19-51): planes n × C_in × N × N f32, NCHW like the
 * reference tensor (index c*N² + row*N + col). */
TG_API int tg_encode(TgEngine* e, int n, const void* states, float* planes);

/* move_index (alpha-tak/src/search/move_map.rs:19-48) for k moves; -1 where the reference
 * would panic ("could not map turn to index"). */
TG_API int tg_move_index(TgEngine* e, int k, const TgMove* moves, int32_t* index);

/* Example::to_tensors (alpha-tak/src/example.rs:62-78) over Symmetry (tak/src/symm.rs:7-97): the 8 dihedral
 * images of n examples.  In: n states, per example n_moves[i] (move, visits) pairs in rows of TG_MAX_MOVES.
 * Out: 8n packed states (image order of symm.rs:11-20; feed them to tg_encode for the input planes) and 8n
 * policy targets of P floats: visits/total at move_index of the transformed move, 0 elsewhere. */
TG_API int tg_augment_examples(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves,
                        const uint32_t* visits, void* out_states, float* pi);

/* perft of tak/tests/perft.rs:3-18 evaluated on the GPU: one count per input state.
 * depth ≥ 0.  Expands level by level on the device (movegen+play+result kernels).  The positions a level expands are staged
 * in rows of TG_MAX_MOVES moves: at depth >= 2 an ongoing position with a longer list on a level that is expanded makes the call
 * return TG_ERR_INVALID_ARG (tg_movegen's rule; the message names the root it lies below) before that level is expanded.  The
 * last level is only counted, so depth 1 returns the true count of any position. */
TG_API int tg_perft(TgEngine* e, int n, const void* states, int depth, uint64_t* counts);

/* ---------------------------------------------------------------------------------------
 * Network (replaces Network<N>, alpha-tak/src/model/network.rs:26-35, without tch types)
 * ------------------------------------------------------------------------------------- */

/* Provide one tensor in tch/libtorch layout (conv OIHW, linear [out,in], BN vectors).
 * Names: "conv0.weight" "conv0.bias" "bn0.weight" "bn0.bias" "bn0.running_mean"
 * "bn0.running_var"; "res{i}.conv1.weight" … "res{i}.bn2.running_var" (i = 0..R-1);
 * "policy.weight" "policy.bias" (FC5: [1575, F*25]; CONV: [ch, F, 3, 3]); "value.weight"
 * "value.bias" ([1, F*N*N]).  Creation order of net5.rs:29-62 / net6.rs:29-57. */
TG_API int tg_net_set_tensor(TgEngine* e, const char* name, const float* data, size_t count);
/* Network::default() (net5.rs:29-73 / net6.rs:29-69): fill every tensor with tch's default initialisers (conv: weight
 * U(±1/sqrt(fan_in)), bias 0; BatchNorm: weight U(0,1), bias 0, mean 0, var 1; linear: weight and bias U(±1/sqrt(in))),
 * drawn from Philox(seed).  The reference draws from libtorch's global generator: same distribution, other values. */
TG_API int tg_net_init_random(TgEngine* e, uint64_t seed);
/* read back a tensor (tch layout) as last set / initialised / committed by the trainer — what Network::save writes */
TG_API int tg_net_get_tensor(TgEngine* e, const char* name, float* out, size_t count);
/* Fold BN (eval mode, eps 1e-5) into the convs, re-layout for the MFMA kernels, upload. */
TG_API int tg_net_finalize(TgEngine* e);
/* Arithmetic of the residual tower (call before tg_net_finalize).
 * TG_PRECISION_F32 (default): f32 operands on v_mfma_f32_16x16x4_f32 — exact f32 fmaf chains.
 * TG_PRECISION_BF16X3: every f32 operand is carried as hi + lo bf16 halves and a product is the sum of three bf16
 *   MFMAs (hi·hi + lo·hi + hi·lo) accumulated in f32 — 16 mantissa bits per operand, 3/16 of the f32 MFMA time.
 *   Measured deviation from the f32 forward ≤ 1e-5 relative on the policy and ≤ 3e-6 on the eval, inside the 1e-4 the
 *   reference comparison allows; supported for 5×5 (64 / 128 filters) and 6×6 (128 filters).  Heads stay f32. */
typedef enum TgPrecision { TG_PRECISION_F32 = 0, TG_PRECISION_BF16X3 = 1 } TgPrecision;
TG_API int tg_net_set_precision(TgEngine* e, int precision);

/* Network::policy_eval (net5.rs:120-130 / net6.rs:124-138): n states → policy n×P
 * (full softmax, not masked) and eval n (tanh).  n = 0 is allowed (returns TG_OK). */
TG_API int tg_policy_eval(TgEngine* e, int n, const void* states, float* policy, float* eval);

/* Network::forward_mcts (net5.rs:106-111) on already-encoded planes (n × C_in × N × N, NCHW,
 * host).  Same outputs as tg_policy_eval. */
TG_API int tg_forward_mcts(TgEngine* e, int n, const float* planes, float* policy, float* eval);

/* Device-resident variants used by bench.py: d_states / d_policy / d_eval are device
 * pointers; no synchronisation. */
TG_API int tg_policy_eval_dev(TgEngine* e, int n, const void* d_states, float* d_policy, float* d_eval);

/* Symmetry ensemble of tg_policy_eval: the mean of the network's output over chosen dihedral images of every state, mapped
 * back to the state's own orientation.  No counterpart in the reference, which uses the symmetries of tak/src/symm.rs:11-20
 * for training examples only (alpha-tak/src/example.rs:62-78); this is the same group, in the same order, at the evaluation.
 *   mask: bit s set = image s (tg_augment_examples' order, s = 0 the identity) takes part; 0xFF = the whole group.  mask = 0
 *     or a bit above 7 → TG_ERR_INVALID_ARG.  The engine must use TG_EVAL_RESNET with finalized weights, else TG_ERR_STATE.
 *     n = 0 returns TG_OK.
 *   With k = popcount(mask), p_s / v_s = what tg_policy_eval returns for image s of state i (in tg_net_set_precision's
 *   arithmetic), and perm[s][j] = the policy slot of the image under s of the move whose slot is j (tables built on the device
 *   at tg_net_finalize from the move transform and move index of tg_augment_examples):
 *       policy[i][j] = (Σ_s p_s[i][perm[s][j]]) · (1/k)        eval[i] = (Σ_s v_s[i]) · (1/k)
 *   ORDER: both sums run in f32 over ASCENDING s, starting from the first selected image (no zero is added in front of it);
 *   the product with the f32 constant 1.0f / (float)k comes last.  So mask = 1 << s is tg_policy_eval of image s de-permuted,
 *   and mask = 0x01 is tg_policy_eval bit for bit.  A state's outputs do not depend on the other states of the call.
 *   The host variant slices by ⌊max_batch / k⌋ states itself and synchronises (max_batch < k → TG_ERR_INVALID_ARG); the _dev
 *   variant takes device pointers, requires n · k ≤ max_batch and does not synchronise, like tg_policy_eval_dev. */
TG_API int tg_policy_eval_symm(TgEngine* e, int n, const void* states, uint32_t mask, float* policy, float* eval);
TG_API int tg_policy_eval_symm_dev(TgEngine* e, int n, const void* d_states, uint32_t mask, float* d_policy, float* d_eval);
/* The device's permutation tables as tg_net_finalize built them: 8 × P int32, perm[s·P + j] (−1 = slot j has no image; none is
 * expected).  No counterpart in the reference (tak/src/symm.rs:11-20 is the group).  Diagnostic read for tests; synchronises. */
TG_API int tg_symm_perm_read(TgEngine* e, int32_t* perm);

/* ---------------------------------------------------------------------------------------
 * Search (replaces Node + Node::{virtual_rollout, devirtualize_path, select, apply_dirichlet,
 * pick_move, play}, alpha-tak/src/search/{node,mcts,noise,play}.rs) for `games` independent
 * trees stepped in lock-step, `batch` leaves per game per iteration (1 = the loop body of
 * train/src/self_play.rs:181-210; 16 = Player::rollout, player.rs:77-110).
 * ------------------------------------------------------------------------------------- */
typedef struct TgSearchConfig {
    int32_t games;            /* concurrent games (≤ cfg.max_batch)                          */
    int32_t arena_nodes;      /* AVERAGE node budget per game: all trees live in ONE pool of games × arena_nodes nodes
                                 (24 B each) handed out in chunks, so a single tree may be far larger than this while
                                 others are small.  A rollout adds one node per legal move of the expanded leaf (≈ 45 on
                                 5×5, ≈ 80 on 6×6); the subtree under the move played is kept (tree reuse) and the rest
                                 returns to the pool.  The reference's own workload — 32 games × 10 000 rollouts on 6×6 —
                                 peaks at ≈ 2^20 per game (31 M nodes, 0.75 GB in all: profiles/r02_soak_reference_workload.log); 4096 5×5 games at 400 rollouts ≈ 2^16 – 2^17.
                                 Headroom for re-rooting: on a move the kept subtree is copied into fresh chunks BEFORE the old
                                 tree's chunks are reusable (they are published at the next launch), so the pool must hold,
                                 for every game that moves in the same call, its old tree plus its kept subtree (≤ the old
                                 tree) — there is no per-game guarantee that a kept subtree fits, only the pool total.
                                 Exhausting the pool → TG_ERR_ARENA_OVERFLOW (sticky until reset).
                                 0 = auto: half of the free device memory, at most 2^22 nodes per game and 2^32 in all */
    float exploration_base;   /* EXPLORATION_BASE 500 (mcts.rs:7) */
    float exploration_init;   /* EXPLORATION_INIT 4   (mcts.rs:8) */
    uint64_t seed;            /* counter-based RNG key (noise, move sampling, openings)      */
    uint32_t slot_base;       /* global index of this engine's first game: RNG streams are keyed by
                                 (seed, slot_base + g, …) so shards on different GPUs play different,
                                 reproducible games (rank r of a sharded run passes r * games)        */
    uint32_t batch;           /* virtual rollouts per tree and iteration before the one network call — the batching of
                                 `Player` (player.rs:77-93; pit.rs BATCH_SIZE 16).  0 = 1 (self_play_parallel: one leaf per game).
                                 games × batch ≤ TgConfig.max_batch.  IGNORED by tg_selfplay_create, whatever it holds: the
                                 self-play driver takes its batch from TgSelfPlayConfig.batch */
    int32_t visit_limit;      /* entries of the exploration-rate table = largest visits + virtual visits of one node;
                                 0 = TG_LIMIT_VISITS (16 MB).  Smaller values serve tests of the limit handling */
    int32_t reserved;
} TgSearchConfig;

TG_API int tg_search_create(TgEngine* e, const TgSearchConfig* cfg);
/* (re)start every tree as Node::default() with the given root states (host, games packed states).  The states are checked
 * on the host (board size, heights, colour bits, reserves): one no game can reach → TG_ERR_INVALID_ARG naming it. */
TG_API int tg_search_reset(TgEngine* e, const void* states);
/* run `iters` lock-step iterations (virtual_rollout → policy_eval → devirtualize_path).
 * active: optional host mask (games bytes, 0 = skip this game), NULL = all. */
TG_API int tg_search_run(TgEngine* e, int iters, const uint8_t* active);
/* One pseudo-random dihedral image per evaluated leaf (AlphaGo Zero's scheme).  No counterpart in the reference, whose search
 * shows the network every position in the orientation it arose in; the group and its order are tak/src/symm.rs:11-20.
 *   TG_SYMM_HASHED: a leaf that goes to the network goes there as its image under
 *       s = philox4x32_10(TgSearchConfig.seed; hash_lo, hash_hi, 0x73796d6d, 0)[0] & 7,
 *     hash = the 64-bit hash of the leaf's packed state (the one TG_EVAL_HASH evaluates), and its children's priors come back
 *     through the inverse permutation (tg_policy_eval_symm's tables).  s depends on the position and the seed only — not on the
 *     slot, the iteration or the batch pass — so transpositions agree and a sharded run equals the full run.  The value needs
 *     no mapping.
 *   Set it after tg_search_create / tg_selfplay_create and before the next iteration runs; it is sticky for that search object —
 *   tg_search_run and tg_selfplay_step (dense and compacted iterations, any batch) — and the next tg_search_create /
 *   tg_selfplay_create resets it to TG_SYMM_OFF.  tg_pit creates its own searches: it takes over the mode each of its two
 *   engines holds when it is called (set it on each engine before the call; an engine without a search keeps the mode for that
 *   purpose).  Requires TG_EVAL_RESNET (else TG_ERR_STATE); an unknown mode → TG_ERR_INVALID_ARG.  TG_SYMM_OFF (the default)
 *   launches nothing and changes nothing.
 *   tg_search_get_symmetry: the mode, and the engine's count of leaves sent to the network under s ≠ 0 since the engine was
 *   created (synchronises). */
typedef enum TgSearchSymmetry { TG_SYMM_OFF = 0, TG_SYMM_HASHED = 1 } TgSearchSymmetry;
TG_API int tg_search_set_symmetry(TgEngine* e, int mode);
TG_API int tg_search_get_symmetry(TgEngine* e, int* mode, uint64_t* leaves_transformed);
/* Proven values inside the tree (the MCTS-solver backup of Winands et al.).  No counterpart in the reference, whose tree keeps
 * the result of a finished position in its node (mcts.rs:35-38) and never draws the conclusion one level up.
 *   Node status, from the result code of a node (TgNodeRecord.result): W for TG_WHITE_ROAD, TG_WHITE_FLAT, TG_PROVEN_WHITE; B
 *     likewise for black; D for TG_DRAW, TG_DRAW_REVERSIBLE, TG_PROVEN_DRAW; unknown otherwise (an uninitialised child is
 *     unknown).  The TG_PROVEN_* codes are node-record codes, never a game's result: tg_result, the examples and the self-play
 *     statistics never carry them.  They name colours, not "win / loss".
 *   The rule, for an initialised ongoing node X whose side to move has colour c: some child has status c → X becomes
 *     TG_PROVEN_c; else, if no child is unknown, X becomes TG_PROVEN_DRAW if some child is D and TG_PROVEN_(opponent of c)
 *     otherwise; else nothing.  A proven node keeps its child count and its children.
 *   TG_PROOF_ON: a rollout that has just initialised a finished position applies the rule to the path upward from that
 *     node's parent, stopping at the first node that stays unknown; the root may be proven.  Nothing else changes a status.
 *     A rollout that reaches a proven node ends there and backs up ±1 / 0 by its colour, like a finished position's; the
 *     node's q and visits are not rewritten when it is proven.  With batch > 1 the passes of an iteration run in order, and a
 *     status written by one pass is seen by the next.  At every return of tg_search_run / tg_selfplay_step the tree of a game
 *     searched under TG_PROOF_ON since its last reset is closed under the rule: every proven node satisfies it and no
 *     unproven initialised node does.  tg_search_play carries the statuses with the subtree.
 *   The mode may be set at any time; on a tree that already has visits the statuses appear only from the next rollout that
 *     initialises a finished position on, so the closure holds only for trees searched under TG_PROOF_ON from their reset.
 *     Back to TG_PROOF_OFF: the rollouts of the off mode know the TgResult codes alone and would back a proven node up as a
 *     draw, so once an iteration has run under TG_PROOF_ON the mode is turned off only after a tg_search_reset (before the next
 *     iteration) or by a new create; otherwise TG_ERR_STATE and the mode stays on.  A self-play object has no reset: create anew.
 *     It is sticky for the search / self-play object — tg_search_run and tg_selfplay_step, any evaluator, any batch, dense and
 *     compacted iterations — and the next tg_search_create / tg_selfplay_create resets it to TG_PROOF_OFF (the default: the
 *     engine without any of this).  tg_pit creates its own searches and runs them with TG_PROOF_OFF.
 *     Without a search object TG_ERR_STATE; an unknown mode → TG_ERR_INVALID_ARG.
 *   Self-play under TG_PROOF_ON picks its move proof-aware.  With m the root's colour to move:
 *     1. if some root child has status m, the move is, among those children, the most visited, the LAST on ties, whatever
 *        the temperature;
 *     2. otherwise the candidates are the children whose status is not the opponent's colour, all children if that leaves
 *        none, and pick_move (play.rs:49-67) runs on the candidates: exploit → most visited, last on ties; explore → the
 *        draw over the visits with the other children's visits taken as 0; candidates without any visit → exploit over them.
 *     The example keeps the root's real visits.
 *   tg_search_get_proof: the mode, the nodes proven and the rollouts that ended on a proven node since tg_search_create /
 *     tg_selfplay_create (synchronises; any pointer may be NULL).
 *   tg_search_proof: root_status: games bytes, the result code of every root; child_status: games × TG_MAX_MOVES bytes, the
 *     code of every root child in possible_moves order (0, a TgResult or a TgProven), zero past counts[g]; counts: games.
 *     Any pointer may be NULL.  Synchronises. */
typedef enum TgProven { TG_PROVEN_WHITE = 8, TG_PROVEN_BLACK = 9, TG_PROVEN_DRAW = 10 } TgProven;
typedef enum TgSearchProof { TG_PROOF_OFF = 0, TG_PROOF_ON = 1 } TgSearchProof;
TG_API int tg_search_set_proof(TgEngine* e, int mode);
TG_API int tg_search_get_proof(TgEngine* e, int* mode, uint64_t* nodes_proven, uint64_t* rollouts_ended_on_proven);
TG_API int tg_search_proof(TgEngine* e, uint8_t* root_status, uint8_t* child_status, int32_t* counts);
/* Node::apply_dirichlet (noise.rs:6-16) on every active root with engine RNG
 * (stream = (seed, game, ply)). */
TG_API int tg_search_apply_dirichlet(TgEngine* e, float alpha, float ratio, const uint8_t* active);
/* Node::apply_dirichlet with caller-supplied noise (games × TG_MAX_MOVES f32, row g holds one
 * sample per child of root g) — lets a test feed the same samples to the oracle. */
TG_API int tg_search_apply_noise(TgEngine* e, const float* noise, float ratio, const uint8_t* active);
/* Node::improved_policy (play.rs:13-21) + root stats: per game the root's children in
 * possible_moves order.  moves/visits/prior/q: games × TG_MAX_MOVES; counts: games;
 * root_visits / root_q: games (any pointer may be NULL). */
TG_API int tg_search_root(TgEngine* e, TgMove* moves, uint32_t* visits, float* prior, float* q,
                   int32_t* counts, uint32_t* root_visits, float* root_q);
/* Node::play (play.rs:26-43) + Game::play: advance each active game by moves[g] with tree reuse: the chosen child's
 * subtree is copied breadth-first into fresh chunks of the shared node pool and the game's old chunks return to the pool.
 * The returned chunks become available to allocators only at the next launch, so WHILE a move is played the pool holds the
 * old trees and the kept subtrees at once (see arena_nodes: headroom). */
TG_API int tg_search_play(TgEngine* e, const TgMove* moves, const uint8_t* active);
/* current root states (games packed states) */
TG_API int tg_search_states(TgEngine* e, void* states);
/* canonical serialisation of game g's whole tree, depth-first in child order, one record per
 * initialised node: {move u16, n_children u16, visits u32, virtual u32, result u32,
 * prior f32 bits, q f32 bits}.  result: TG_ONGOING, the TgResult of a finished position, or under TG_PROOF_ON a TgProven
 * code.  Returns record count through *n_records (cap = capacity). */
typedef struct TgNodeRecord {
    uint16_t move;
    uint16_t n_children;
    uint32_t visits;
    uint32_t virtual_visits;
    uint32_t result;
    uint32_t prior_bits;
    uint32_t q_bits;
} TgNodeRecord;
TG_API int tg_search_dump(TgEngine* e, int game, TgNodeRecord* records, size_t capacity, size_t* n_records);
/* Node::debug(depth) (alpha-tak/src/search/debug.rs:9-51) of every game's root, computed on the device.
 *   moves / visits / reward (= q) / policy (= prior): games × TG_MAX_MOVES, the root's children sorted by visits descending,
 *     ties by child index DESCENDING (a stable ascending sort followed by reverse(); the reference's sort_unstable_by_key +
 *     reverse gives the same order for ≤ 20 children and leaves it unspecified beyond).  counts: games.
 *   eval: games, NodeDebugInfo::eval in f32: total = (float)(u32 sum of visits), acc = +0.0f, acc = acc + reward_i *
 *     ((float)visits_i / total) in the sorted order, no contraction.  No children → +0.0; children but no visits → NaN.
 *   cont_moves / cont_visits: games × top_k × depth, cont_len: games × top_k — Node::continuation(depth) of the first top_k
 *     sorted children: while the node is initialised (visits or virtual visits ≠ 0) and has children, step to its most
 *     visited child (the LAST one on ties, pick_move(true)) and record (move, that child's visits).
 * Entries past counts[g] or cont_len are zero.  Any pointer may be NULL.  0 ≤ depth ≤ TG_DEBUG_MAX_DEPTH and
 * 0 ≤ top_k ≤ TG_MAX_MOVES, else TG_ERR_INVALID_ARG.  The games run in slices whose device scratch stays within
 * TG_DEBUG_SCRATCH_BYTES (one game needs at most ≈ 200 KB); one synchronisation per slice. */
#define TG_DEBUG_MAX_DEPTH 64
#define TG_DEBUG_SCRATCH_BYTES (1 << 26)
TG_API int tg_search_debug(TgEngine* e, int depth, int top_k,
                           TgMove* moves, uint32_t* visits, float* reward, float* policy,
                           int32_t* counts, float* eval,
                           TgMove* cont_moves, uint32_t* cont_visits,
                           int32_t* cont_len);
/* counters since tg_search_create: expansions = completed rollouts (terminal ones included,
 * as in the reference's ROLLOUTS loop), evals = leaves sent to the network */
TG_API int tg_search_counters(TgEngine* e, uint64_t* expansions, uint64_t* evals);
/* occupancy of the node pool (for sizing TgSearchConfig.arena_nodes): nodes the pool holds, nodes in chunks currently owned
 * by trees, and the largest number of nodes ever owned at once since tg_search_create / tg_search_reset.  Synchronises. */
TG_API int tg_search_pool(TgEngine* e, uint64_t* nodes_total, uint64_t* nodes_in_use, uint64_t* nodes_peak);

/* ---------------------------------------------------------------------------------------
 * Forced wins: an exact depth-limited AND/OR search over Game::possible_moves / play / result
 * (solve_kernels.hip).  A capability beside the MCTS, not a part of it: no network, no tree.
 *
 * For an ongoing position s with mover m, s_a is the position after legal move a:
 *   W(s, L) "the mover wins within L plies": false for L <= 0, else some a has result(s_a) = a win of m (road or flats) or
 *           has s_a ongoing and X(s_a, L-1).
 *   X(s, L) "the mover loses within L plies": false for L <= 0, else EVERY a has result(s_a) = a win of the opponent (a move
 *           that completes only the opponent's road) or has s_a ongoing and W(s_a, L-1).
 *   A draw (either kind, the reversible-plies rule included) proves nothing for either side.
 * move_values[a]: +1 wins at once, -1 loses at once, +(1+k) for the least k with X(s_a, k), -(1+k) for the least k with
 *   W(s_a, k), 0 if none of these holds with 1+k <= depth.
 * value: +d with d the smallest positive move value; -d with d the largest |move value| if ALL moves are negative; else 0.
 * best: the first move (possible_moves order) with the smallest positive value; in a lost position the first move with the
 *   largest |value| (the longest defence); 0 when value is 0.
 * The levels L = 1, 2, ... are deepened in turn, one launch each.  Without TG_SOLVE_ALL_MOVES a position stops at the first
 * level that decides it (some move wins, or all moves lose): move values that need more plies stay 0.  With it every level
 * up to `depth` runs and the move table is complete.  A finished position, an inactive or a dead game gives counts 0,
 * value 0, best 0.
 *
 * "Wins" means by road OR by flats.  TG_SOLVE_ROAD_ONLY asks for the road-only proof instead, the tinue of Tak players (what
 * PTN's marks ' and " stand for).  With it the definitions change in one point, the meaning of "wins":
 *   W(s, L): some a has result(s_a) = a ROAD of m, or has s_a ongoing and X(s_a, L-1).
 *   X(s, L): EVERY a has result(s_a) = a ROAD of the opponent, or has s_a ongoing and W(s_a, L-1).
 *   A move that ends the game in any other way (flats for either colour, a draw of either kind) proves nothing for either
 *   side: it gets move value 0 and ends an X test as a draw does.  A move that completes both roads is the mover's road
 *   (Game::result gives it to the mover).
 * Move values, value, best, the early stop, TG_SOLVE_ALL_MOVES, node_budget and budget_hit are defined on these two predicates
 * exactly as above.  A road-only proof is also a proof by the definitions above, of the same sign and at most as long; the
 * converse does not hold.
 * flags: TG_SOLVE_ALL_MOVES (bit 0) | TG_SOLVE_ROAD_ONLY (bit 2).  Bit 1 is not assigned: it is an unknown bit like every
 * higher one and is rejected.
 *
 * node_budget: positions one work item = (position, root move, level) may create before it gives up that level; the move
 *   stays unproven at that level and may be proven at a later one.  budget_hit[i] = 1 if any item of position i gave up.
 *   With budget_hit 0 the outputs are exactly the definitions above.  With budget_hit 1 every non-zero entry is still a
 *   sound proof: the sign of the exact answer at the same depth, |d| >= the exact |d|; nothing else is promised.
 *   nodes[i] (positions created by play for position i) <= counts[i] * depth * (node_budget + TG_MAX_MOVES).
 *   Move-list capacity inside the tree: a position BELOW a root with more than TG_MAX_MOVES moves is a give-up of the same kind.
 *   Its list is the first TG_MAX_MOVES moves of possible_moves.  X on such a position does not hold (nothing can be said of
 *   "every move") and no move of it is played; W on it tries those TG_MAX_MOVES moves and holds if one of them wins, else it does
 *   not hold.  In both failing cases the item is marked as given up, and unlike the node budget the search of the item goes on:
 *   budget_hit[i] = 1 if a test that failed on a cut list was reached at any level that ran for position i (tests are tried in
 *   move order and stop at the first move that decides them, so a cut list behind that move is never reached).  The promise
 *   above holds: every non-zero entry is a sound proof.  A ROOT with more than TG_MAX_MOVES moves is TG_ERR_INVALID_ARG naming
 *   the position, returned before any level is searched.
 *   0 = TG_SOLVE_DEFAULT_BUDGET, which exists so that no launch on a shared card can run away; values above 2^31 - 1
 *   count as 2^31 - 1.  The default is 2^10, fixed by scripts/bench_solve.py on an MI355X (profiles/r18_b_solve.json): the
 *   largest power of two that keeps the longest level launch at depth 5 on its two inputs of 4096 positions under
 *   100 ms — 69 ms (mid-game) and 45 ms (near the end) at 2^10, 156 ms and 86 ms at 2^11.  At the default most unproven
 *   depth-5 positions report budget_hit; a caller who can wait passes a larger budget (2^22 gave up nowhere on those
 *   inputs: 3.3 to 4.1 s per 4096 positions).  The default was tuned on the default mode and holds for road-only proofs too.
 *
 * moves / move_values: n x TG_MAX_MOVES, zero past counts[i]; every other output: n.  Any output pointer may be NULL.
 * tg_solve validates the states on the host as tg_search_reset does; it needs no network and no search object.
 * tg_search_solve solves the current roots of the live search / self-play object in place (no host copy of the states,
 * the trees are not touched); without such an object TG_ERR_STATE.  active: games mask or NULL = all.
 * Both synchronise before they return.  TG_ERR_INVALID_ARG names the field: depth outside 1 .. TG_SOLVE_MAX_DEPTH, unknown
 * flags, non-zero reserved, NULL states with n > 0.
 * ------------------------------------------------------------------------------------- */
#define TG_SOLVE_MAX_DEPTH 6
#define TG_SOLVE_ALL_MOVES 1u
#define TG_SOLVE_ROAD_ONLY 4u  /* (4, not 2: bit 1 stays unassigned and rejected) */
#define TG_SOLVE_DEFAULT_BUDGET (1 << 10)
typedef struct TgSolveConfig {
    int32_t depth;         /* 1 .. TG_SOLVE_MAX_DEPTH */
    uint32_t flags;        /* TG_SOLVE_ALL_MOVES | TG_SOLVE_ROAD_ONLY */
    uint64_t node_budget;  /* positions a single (position, root move, level) work item may create before it gives up; 0 = default */
    int32_t reserved[4];   /* must be 0 */
} TgSolveConfig;
TG_API int tg_solve(TgEngine* e, int n, const void* states, const TgSolveConfig* cfg,
                    int8_t* value, TgMove* best, int32_t* counts, TgMove* moves, int8_t* move_values,
                    uint8_t* budget_hit, uint64_t* nodes);
TG_API int tg_search_solve(TgEngine* e, const TgSolveConfig* cfg, const uint8_t* active,
                           int8_t* value, TgMove* best, int32_t* counts, TgMove* moves, int8_t* move_values,
                           uint8_t* budget_hit, uint64_t* nodes);

/* ---------------------------------------------------------------------------------------
 * Self-play driver (replaces self_play_parallel, train/src/self_play.rs:96-262).
 * All compile-time constants of the reference (self_play.rs:10-19,94) are runtime here.
 * ------------------------------------------------------------------------------------- */
typedef struct TgSelfPlayConfig {
    int32_t rollouts;        /* ROLLOUTS per move (reference 10_000; BASELINE 400 / 100)     */
    int32_t noise_plies;     /* NOISE_PLIES 80   */
    int32_t exploit_plies;   /* EXPLOIT_PLIES 40 */
    float noise_alpha;       /* NOISE_ALPHA 0.2  */
    float noise_ratio;       /* NOISE_RATIO 0.3  */
    int32_t komi;            /* Game::with_komi(2) */
    int32_t total_games;     /* SELF_PLAY_GAMES: finished games are replaced until
                                completed + games ≥ total_games (self_play.rs:151,237); 0 = endless */
    int32_t max_examples;    /* capacity of the device example ring drained by tg_selfplay_drain */
    int32_t max_game_plies;  /* a game is retired (see TG_LIMIT_*) when it would stage more examples than this;
                                0 = TG_LIMIT_GAME_PLIES, the size of the per-game staging area (the largest value allowed) */
    int32_t batch;           /* virtual rollouts per game and iteration (Player's batching, player.rs:77-110; the reference's
                                self_play uses BATCH_SIZE 32, train/src/self_play.rs:11): every iteration hands the network
                                games × batch leaves.  0 = 1 (this field was `reserved`: a zeroed one behaves as before).
                                0 ≤ batch ≤ 4096, and games × batch ≤ TgConfig.max_batch with the resnet evaluator, else
                                TG_ERR_INVALID_ARG */
} TgSelfPlayConfig;

/* One training example, fixed-size record (reference alpha-tak/src/example.rs:29-33):
 * the position before the move, the visit count of every legal move in possible_moves
 * order, and the final result from the mover's perspective (self_play.rs:245-251). */
typedef struct TgExampleHeader {
    int32_t game_id;      /* global id of the game this example came from */
    int32_t n_moves;
    float result;         /* +1 / -1 / 0 from the perspective of the side to move */
    int32_t reserved;
} TgExampleHeader;

TG_API int tg_selfplay_create(TgEngine* e, const TgSearchConfig* scfg, const TgSelfPlayConfig* cfg);
/* run `plies` lock-step plies of self_play_parallel's outer loop (opening → instant-win scan
 * → noise → rollouts → pick/play/recycle).  Asynchronous; tg_sync() to wait.
 * One ply at TgSelfPlayConfig.batch = B:
 *   - opening, instant-win scan, finish and re-root as at B = 1;
 *   - games under noise_plies run ONE iteration of B virtual rollouts (one network call, B de-virtualisations in rollout
 *     order) and then receive Dirichlet noise — Player::add_noise, which consumes a batch and then applies the noise;
 *   - every live game runs `rollouts` iterations of B virtual rollouts, each with one network call of games × B leaves and
 *     B de-virtualisations in rollout order; between two iterations the de-virtualisations of one and the virtual rollouts
 *     of the next share one kernel launch;
 *   - pick, play and recycle as at B = 1.
 * TgSelfPlayStats.expansions counts rollouts, so it grows B-fold.  A game that runs into a TG_LIMIT_* capacity in the
 * middle of a batch is retired as at B = 1; the remaining rollouts of that batch are skipped.
 * Not reproduced: the one batch `Player` keeps in flight across add_noise and play_move (its pipelining), as in tg_pit.
 * With a rollout schedule on (tg_selfplay_set_schedule) the call waits once per ply for that ply's first `rollouts`
 * iterations — the number of boosted games sizes the launches that follow — and still returns before the ply has ended. */
TG_API int tg_selfplay_step(TgEngine* e, int plies);

/* Rollout schedule of the self-play driver: QUAD_ROLLOUT_PLIES (train/src/self_play.rs:19,63 — a move gets four times the
 * rollouts while game.ply < QUAD_ROLLOUT_PLIES).  Game::ply is the `ply` of the packed state's header, so after the two
 * opening moves the first searched move is ply 2: with boost_plies = 10 the moves at plies 2..9 of every game are boosted.
 * A boosted game's tree after the ply is, bit for bit, the tree of boost_factor × rollouts plain iterations. */
typedef struct TgRolloutSchedule {
    int32_t boost_plies;   /* QUAD_ROLLOUT_PLIES 10: a game whose header ply < boost_plies is "boosted" on this move; 0 = off */
    int32_t boost_factor;  /* 4: a boosted game runs boost_factor × TgSelfPlayConfig.rollouts iterations; 1 = off           */
    int32_t reserved[2];   /* must be 0 */
} TgRolloutSchedule;
/* Set the schedule (train/src/self_play.rs:19,63; ply rule above).  Valid after tg_selfplay_create and before the first
 * tg_selfplay_step, else TG_ERR_STATE; tg_selfplay_create clears it.  0 ≤ boost_plies ≤ TG_LIMIT_GAME_PLIES,
 * 1 ≤ boost_factor ≤ 64, reserved zero, rollouts × boost_factor within int32, else TG_ERR_INVALID_ARG naming the field.
 * Off (boost_plies = 0 or boost_factor = 1) behaves exactly as an engine that never called this.
 * Per ply with a schedule on: all games run `rollouts` iterations as without one; then the games that are alive, not retired
 * and under boost_plies are listed on the device, and the remaining (boost_factor − 1) × rollouts iterations run over that
 * list alone, the network on (listed games) × batch leaves.  The host reads the list's length to size those launches:
 * tg_selfplay_step waits once per ply for that ply's first `rollouts` iterations, and still returns before the ply ends. */
TG_API int tg_selfplay_set_schedule(TgEngine* e, const TgRolloutSchedule* s);
/* Counters of the schedule (train/src/self_play.rs:19,63; ply rule above) since tg_selfplay_create; synchronises.
 * boosted_moves: game-plies that received the boosted budget; compact_iterations: iterations that ran on a compacted list
 * (fewer than all games boosted); compact_leaves: leaves handed to the network in those iterations.  All 0 with the schedule
 * off.  (The one wait per ply of tg_selfplay_step described above is the schedule's only host synchronisation.) */
TG_API int tg_selfplay_schedule_stats(TgEngine* e, uint64_t* boosted_moves, uint64_t* compact_iterations, uint64_t* compact_leaves);
/* statistics: finished games, emitted examples, expansions, network evals */
typedef struct TgSelfPlayStats {
    uint64_t games_finished;
    uint64_t examples;
    uint64_t expansions;
    uint64_t evals;
    uint64_t plies;
    uint64_t white_wins, black_wins, draws;
    uint64_t instant_wins;
    uint64_t dropped_examples; /* finished examples overwritten in the output ring before tg_selfplay_drain fetched them
                                  (max_examples too small for the drain interval); 0 in a loss-free run */
    uint64_t aborted_games;    /* games retired because they exceeded a TG_LIMIT_* capacity (not in games_finished, no examples) */
    uint64_t alive_games;      /* slots still playing: 0 once every slot has retired (completed + games ≥ total_games) —
                                  the end of self_play_parallel's `while` loop (self_play.rs:107) */
} TgSelfPlayStats;
TG_API int tg_selfplay_stats(TgEngine* e, TgSelfPlayStats* out);
/* copy out up to `cap` finished examples (headers + states + moves + visits) and remove them
 * from the ring.  states: cap packed states; moves/visits: cap × TG_MAX_MOVES.  Examples the ring has already
 * overwritten (more than max_examples finished since the last drain) are skipped and counted in
 * TgSelfPlayStats.dropped_examples: size max_examples ≥ games × expected plies per drain interval. */
TG_API int tg_selfplay_drain(TgEngine* e, int cap, TgExampleHeader* headers, void* states, TgMove* moves,
                      uint32_t* visits, int32_t* n_out);

/* ---------------------------------------------------------------------------------------
 * Training step (replaces Network::train / train_inner, alpha-tak/src/model/network.rs:37-97, and the
 * forward_training of net5.rs:113-118 / net6.rs:111-122).  SURVEY.md §8(f) N2 / config C5.
 * The master parameters live on the device in tch layout; every chunk is augmented with the 8 symmetries
 * (Example::to_tensors), encoded, run forward with BatchNorm in training mode (batch statistics, running
 * statistics updated with momentum), and back-propagated with hand-written HIP kernels; gradients accumulate
 * over `chunks_in_step` chunks, then one Adam step (L2 weight decay, as tch's nn::Adam{wd}).
 * Data parallel: after tg_train_comm_init every optimiser step all-reduces (RCCL, sum, f32) the flat gradient
 * buffer and divides by the world size — the only collective of the whole build.
 * ------------------------------------------------------------------------------------- */
typedef struct TgTrainConfig {
    float learning_rate;    /* LEARNING_RATE 1e-4 (network.rs:14) */
    float weight_decay;     /* WEIGHT_DECAY 1e-4 (network.rs:15)  */
    float beta1, beta2, eps;/* tch Adam defaults 0.9, 0.999, 1e-8 */
    float bn_momentum;      /* tch BatchNormConfig default 0.1 */
    float bn_eps;           /* 1e-5 */
    int32_t chunk_size;     /* CHUNK_SIZE 500 examples; ×8 symmetries = positions per forward/backward */
    int32_t chunks_in_step; /* CHUNKS_IN_STEP 20 */
    int32_t reserved;
} TgTrainConfig;

/* Adam{wd}.build(vs, lr) (network.rs:40-45): creates the trainer from the tensors given to tg_net_set_tensor
 * (all of them, as for tg_net_finalize) with zero optimiser state and zero gradients. */
TG_API int tg_train_create(TgEngine* e, const TgTrainConfig* cfg);
/* train_inner (network.rs:58-97) on one chunk of n ≤ chunk_size examples (layout of tg_selfplay_drain:
 * states, n_moves, rows of TG_MAX_MOVES moves / visits; results = Example::result).  Returns the two losses
 * the reference prints (loss_p, loss_z); *stepped = 1 when this chunk completed an optimiser step.  Examples are validated on
 * the host (a reachable state, 1 ≤ n_moves ≤ TG_MAX_MOVES, at least one visit) → TG_ERR_INVALID_ARG. */
TG_API int tg_train_chunk(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves, const uint32_t* visits,
                   const float* results, float* loss_p, float* loss_z, int32_t* stepped);
/* Network::train (network.rs:37-56): fresh Adam state and zeroed gradients, shuffle (Philox keyed by seed; the reference
 * uses thread_rng), chunks_exact(chunk_size) → tg_train_chunk each.  mean losses over the chunks are returned.  Every
 * example is validated (state, move count, visit sum — the checks of tg_train_chunk) before the first chunk, and with a
 * communicator or a reduction hook attached the ranks exchange their verdicts through it (one 16-byte all-reduce): if any
 * rank refuses its examples EVERY rank returns TG_ERR_INVALID_ARG and none trains, so an argument error cannot strand the
 * others in a collective.  All ranks must therefore call tg_train together.  tg_train_chunk validates only its own chunk — a
 * data-parallel caller of tg_train_chunk must agree on errors across ranks itself before the chunk that completes an
 * optimiser step.
 * Execution: the weight gradients of a chunk run on a stream of their own beside the data-gradient chain
 * (TG_TRAIN_ONE_STREAM=1: on the chain's stream); while chunk k runs, tg_train gathers and uploads chunk k + 1 on a copy stream and
 * enqueues it behind chunk k.  The chunks still execute one after the other: the result is that of tg_train_chunk per chunk, bit for bit. */
TG_API int tg_train(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves, const uint32_t* visits,
             const float* results, uint64_t seed, float* mean_loss_p, float* mean_loss_z, int32_t* steps);
/* opt.step(); opt.zero_grad() now (network.rs:92-96), whatever the chunk counter says */
TG_API int tg_train_step(TgEngine* e);
/* the permutation tg_train(seed) visits n examples in (refs.shuffle, network.rs:49-50 — Philox here, thread_rng there): chunk k of
 * tg_train = examples order[k·chunk_size … (k+1)·chunk_size) handed to tg_train_chunk in that order.  Host only, no engine. */
TG_API int tg_train_order(uint64_t seed, int n, int32_t* order);
/* forward_training (net5.rs:113-118): n ≤ 8·chunk_size states → log_softmax policy (n × P) and eval (n),
 * BatchNorm on the statistics of this batch (running statistics are updated, as in libtorch). */
TG_API int tg_train_forward(TgEngine* e, int n, const void* states, float* logp, float* eval);
/* current value of a parameter / BN buffer (names of tg_net_set_tensor) and of its accumulated gradient */
TG_API int tg_train_get_tensor(TgEngine* e, const char* name, float* out, size_t count);
TG_API int tg_train_get_grad(TgEngine* e, const char* name, float* out, size_t count);
/* Intermediate tensors of the training step, for parity tests and error budgets (no counterpart in the reference; libtorch users
 * would register hooks).  tg_train_debug_read: what = "planes" (NHWC input [rows][cin_pad]); "z" / "y" (conv output / activation
 * of conv layer `layer` = 0 conv0, 1 + 2i res{i}.conv1, 2 + 2i res{i}.conv2; [rows][filters]); "mean" / "invstd" (the batch
 * statistics that layer's BatchNorm normalised with; [filters]) — all of the last forward pass; "dy" / "dz" / "dx" (gradient
 * w.r.t. y before the ReLU mask, w.r.t. z, and the data gradient handed to the layer below — for conv1 of a block with the skip
 * path's gradient added; [rows][filters]) of the layer armed with tg_train_debug_capture BEFORE the chunk (layer < 0 disarms;
 * three device copies per chunk while armed).  count = floats to read (≤ the tensor). */
TG_API int tg_train_debug_capture(TgEngine* e, int layer);
TG_API int tg_train_debug_read(TgEngine* e, const char* what, int layer, float* out, size_t count);
/* make the trained parameters the ones tg_policy_eval / search / self-play use (tg_net_set_tensor of every
 * tensor + tg_net_finalize).  With a communicator the BN running statistics are averaged over the ranks first. */
TG_API int tg_train_commit(TgEngine* e);
/* Held-out evaluation: the losses of the DEPLOYED network — the folded-BatchNorm inference network that tg_policy_eval, the
 * search and self-play run, as tg_net_finalize / tg_train_commit last installed it, in tg_net_set_precision's arithmetic — on
 * examples (layout of tg_selfplay_drain / tg_train_chunk, host).  No counterpart in the reference, which prints the training
 * losses of network.rs:86 only: those use batch statistics, on the batch just fitted.  Running statistics here, never batch
 * statistics; no parameter, running statistic or trainer state changes; a search or self-play run on the same engine keeps its
 * trees, example ring and counters.  The engine must use TG_EVAL_RESNET with finalized weights, else TG_ERR_STATE.
 *   n ≥ 0 is any size: the call slices by TgConfig.max_batch itself and synchronises; n = 0 gives zero sums.
 *   Every example is checked on the host before the first launch as by tg_train_chunk (a reachable state, 1 ≤ n_moves ≤
 *     TG_MAX_MOVES, at least one visit) → TG_ERR_INVALID_ARG naming the example.
 *   symmetries = 1: the 8 dihedral images of every example in tg_augment_examples' order, position 8i + s; states and moves
 *     are transformed on the device, no dense policy target is built.
 *   Both arg-maxes of top1 run over the example's LISTED moves in list order, the first maximum wins.
 *   rows (optional): positions × 4 floats {loss_p, loss_z, top1 (0 / 1), v}.  A row depends on its own position only, and the
 *     f64 sums are taken in position order: the same bits for any max_batch.  Adding the sums of several calls keeps the
 *     integer fields exact and the f64 fields up to the caller's own addition order. */
typedef struct TgExampleMetrics {   /* SUMS over positions, so ranks and calls can be added */
    double loss_p;        /* Σ −Σ_m π(m)·log softmax(logits)[move_index(m)],  π = visits/Σvisits   (network.rs:81-84) */
    double loss_z;        /* Σ (z − v)²,  v = tanh(value head), z = Example::result                 */
    double target_entropy;/* Σ −Σ_m π(m)·log π(m)  (0·log 0 = 0): loss_p − this = KL(π‖p)           */
    uint64_t top1;        /* positions where the network's best LEGAL move is the most visited move  */
    uint64_t sign_ok;     /* positions with z ≠ 0 and v·z > 0                                        */
    uint64_t decided;     /* positions with z ≠ 0                                                    */
    uint64_t positions;   /* n, or 8n with symmetries                                                */
} TgExampleMetrics;
TG_API int tg_eval_examples(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves,
                            const uint32_t* visits, const float* results, int symmetries /* 0 or 1 */,
                            TgExampleMetrics* sums, float* rows /* optional: positions × 4 = loss_p, loss_z, top1, v */);
/* RCCL communicator for the gradient all-reduce: rank 0 calls tg_comm_unique_id (128 bytes) and hands the id
 * to every rank (any host transport); then every rank calls tg_train_comm_init. */
TG_API int tg_comm_unique_id(void* id128);
TG_API int tg_train_comm_init(TgEngine* e, int rank, int world_size, const void* id128);
/* The same reduction through a caller-supplied function instead of RCCL — ranks that share one GPU (RCCL refuses duplicate
 * devices), a host transport (gloo, MPI, a socket from Rust), or a test.  The optimiser step calls
 * fn(ctx, d_buf, count, stream) with the flat gradient buffer (device memory, `count` floats); on return — or, if fn only
 * enqueues work, in the order of `stream` (the engine's hipStream_t, tg_stream) — d_buf must hold the SUM over all world_size ranks.
 * The step then applies Adam to d_buf / world_size, so every rank that saw the same sum ends with bit-identical parameters.
 * tg_train_commit reduces the BatchNorm running statistics through the same function.  fn returns 0 or an error code
 * (→ TG_ERR_STATE).  fn = NULL removes the hook.  Mutually exclusive with tg_train_comm_init. */
typedef int (*TgAllReduceFn)(void* ctx, float* d_buf, size_t count, void* hip_stream);
TG_API int tg_train_set_allreduce(TgEngine* e, TgAllReduceFn fn, void* ctx, int world_size);
/* device address and length (floats) of the flat gradient buffer the reduction operates on: parameters in the creation
 * order of tg_net_set_tensor's names, BatchNorm buffers excluded */
TG_API int tg_train_grad_buffer(TgEngine* e, float** d_grads, size_t* count);
/* Measurement: every gradient all-reduce an optimiser step issues (RCCL or the hook) is bracketed
 * with HIP events on the engine stream; this call synchronises the stream and returns their total duration in
 * milliseconds and their number since tg_train_create.  Zero reductions on a single-rank trainer. */
TG_API int tg_train_comm_stats(TgEngine* e, double* ms_total, int64_t* reductions);

/* What is attached to the optimiser step's reduction, as the library itself sees it — so that a launch log can answer "did
 * RCCL see N ranks, and which RCCL": ncclCommCount / ncclCommUserRank of the communicator, ncclGetVersion, and the file
 * ncclAllReduce was bound from (dladdr).  One copy of RCCL per process: a librccl.so.1 the process has already mapped
 * (PyTorch's, when the host uses torch.distributed) is bound in preference to loading another (lib_was_mapped = 1). */
typedef struct TgCommInfo {
    int32_t attached;       /* 0 nothing, 1 RCCL communicator (tg_train_comm_init), 2 caller's function (tg_train_set_allreduce) */
    int32_t world_size;     /* as given to tg_train_comm_init / tg_train_set_allreduce; 1 if nothing is attached */
    int32_t rank;
    int32_t nccl_count;     /* ncclCommCount(comm), -1 without a communicator */
    int32_t nccl_rank;      /* ncclCommUserRank(comm), -1 without a communicator */
    int32_t nccl_version;   /* ncclGetVersion, -1 if librccl was never loaded */
    int32_t lib_was_mapped; /* 1: the bound librccl.so.1 was already in the process when libtakgpu first needed it */
    int32_t reserved;
    char lib_path[256];     /* the shared object ncclAllReduce resolves into; "" if librccl was never loaded */
} TgCommInfo;
TG_API int tg_train_comm_info(TgEngine* e, TgCommInfo* out);
/* Preflight of the reduction the optimiser step will use (RCCL communicator or the caller's function), before the first chunk:
 * every rank contributes 1.0f, ONE float is summed over the ranks on the engine stream, and the call returns when the result is
 * back on the host — TG_ERR_STATE if it is not world_size.  *ms = wall-clock milliseconds of that round trip (the first
 * collective on a communicator also pays RCCL's connection set-up: ring / tree construction over xGMI).  A launch that
 * cannot form a ring stops HERE, with nothing of a training step enqueued, and reads differently from a step that hangs.
 * Collective: every rank must call it.  Single-rank trainer (nothing attached): *ms = 0, returns TG_OK. */
TG_API int tg_train_comm_preflight(TgEngine* e, double* ms);

/* ---------------------------------------------------------------------------------------
 * Example window (the `examples` of training_loop, train/src/main.rs:26,56-123): one ring of `capacity` example rows in
 * device memory, owned by the engine.  The reference keeps one Vec<Example>, extends it with every self-play round and with
 * the `.data` files it loads (main.rs:58-80), truncates it to the latest MAX_EXAMPLES = 400_000 (main.rs:110-115) and trains
 * a fresh copy of the network on all of it each round.  Here the examples stay where they are born and consumed: they enter
 * from the self-play ring (tg_window_absorb) or from the host (tg_window_push) and leave as training chunks
 * (tg_window_train) or as a host copy (tg_window_read).
 * Logical index 0 is the oldest example kept; a new example evicts the oldest once the window is full.  Rows have the layout
 * of tg_selfplay_drain and are canonical: moves and visits past n_moves are zero.
 * Every entry point returns TG_ERR_INVALID_ARG for a null engine and TG_ERR_STATE for an engine without a window (before
 * tg_window_create, or after tg_window_create(e, 0)); an engine exists only where a device does (tg_engine_create:
 * TG_ERR_NO_DEVICE).  Host-side counters and cursors are not thread safe, as the rest of an engine.
 * Data parallel: every rank owns the window of its own engine and fills it from its own games (or its own share of the
 * files); nothing of a window crosses ranks, only the gradients of tg_window_train do.
 * ------------------------------------------------------------------------------------- */
typedef struct TgWindowInfo {
    uint64_t capacity;  /* rows                                                                  */
    uint64_t count;     /* examples kept: min(entered, capacity)                                 */
    uint64_t entered;   /* examples that entered since tg_window_create / tg_window_clear        */
    uint64_t evicted;   /* of those, no longer kept: entered - count                             */
} TgWindowInfo; /* 32 bytes */
/* (Re)create an empty window of `capacity` examples (main.rs:26 MAX_EXAMPLES); capacity = 0 frees it.  The window outlives
 * tg_selfplay_create, tg_search_create, tg_train_create, tg_net_finalize, tg_train_commit and tg_pit (the loop of
 * main.rs:82-122 recreates self-play after every pit) and dies with the engine.  capacity < 0, or a byte size beyond size_t
 * -> TG_ERR_INVALID_ARG; a failed allocation -> TG_ERR_HIP and an engine without a window, never half of one.  Synchronises
 * when a window is replaced. */
TG_API int tg_window_create(TgEngine* e, int capacity);
/* the counters above (main.rs:110-115: what the truncation has dropped is `evicted`); out = NULL -> TG_ERR_INVALID_ARG */
TG_API int tg_window_info(TgEngine* e, TgWindowInfo* out);
/* forget every example and zero the counters (no counterpart in main.rs:56-123: a new `examples` vector) */
TG_API int tg_window_clear(TgEngine* e);
/* examples.extend(new_examples) + the truncation (main.rs:106-115) without the host: every finished example of the
 * self-play ring moves into the window on the device, in ring order — exactly the examples, in the order, that one
 * tg_selfplay_drain with unlimited cap would return, zeros past n_moves included, game_id as drain reports it.  Shares
 * drain's cursor: the two may be mixed on one engine and each example goes to exactly one of them; examples the ring has
 * already overwritten are skipped and counted in TgSelfPlayStats.dropped_examples as drain counts them.  When one call
 * brings more than `capacity` examples only the newest `capacity` are copied; the others count as entered and evicted.
 * Synchronises once, as drain does, to learn how many there are; the copy itself is asynchronous on the engine's stream.
 * *n_absorbed (optional) = how many entered.  Without tg_selfplay_create -> TG_ERR_STATE; device errors of the search as
 * from tg_sync. */
TG_API int tg_window_absorb(TgEngine* e, int32_t* n_absorbed);
/* The same rows from the host: the `.data` files of main.rs:58-80 through tg_parse_example (layout of tg_train: states,
 * n_moves, rows of TG_MAX_MOVES moves / visits, results; game_ids optional, NULL = 0).  Every example is checked first, as
 * tg_train_chunk checks its own (a reachable state, 1 <= n_moves <= TG_MAX_MOVES, at least one visit): a bad one ->
 * TG_ERR_INVALID_ARG naming its index, and the window is untouched.  Rows are made canonical on the way (whatever stands
 * past n_moves is not copied).  n > capacity: the newest `capacity` are kept, as in tg_window_absorb.  n < 0 or a null array
 * with n > 0 -> TG_ERR_INVALID_ARG.  Synchronises. */
TG_API int tg_window_push(TgEngine* e, int n, const void* states, const int32_t* n_moves, const TgMove* moves,
                          const uint32_t* visits, const float* results, const int32_t* game_ids /* NULL = 0 */);
/* logical [first, first + n) -> host, in tg_selfplay_drain's output layout (n headers, n states, n x TG_MAX_MOVES moves and
 * visits): what main.rs:117-121 would write to a `.data` file, or a held-out share for tg_eval_examples.  The window is not
 * changed.  A range outside [0, count], a negative argument, or a null array with n > 0 -> TG_ERR_INVALID_ARG.
 * Synchronises. */
TG_API int tg_window_read(TgEngine* e, int first, int n, TgExampleHeader* headers, void* states, TgMove* moves, uint32_t* visits);
/* Network::train (network.rs:37-56) on logical [first, first + count) of the window (main.rs:82-95 trains on all of it:
 * first = 0, count = TgWindowInfo.count).  The result is that of tg_train(count, those examples oldest first, seed), bit for
 * bit: losses, steps, every parameter, every BatchNorm statistic, the Adam state — the same shuffle, chunks_exact (the
 * remainder is dropped; count < chunk_size trains nothing and returns zero losses), fresh optimiser per call, and the same
 * two-set pipeline, with one gather kernel per chunk on the copy stream in place of the host gather and its five copies.
 * The window is not changed.  Its examples were checked when they entered, so there is no validation pass and NO exchange
 * of verdicts between ranks: with a communicator or a reduction hook attached every rank must pass a `count` that gives
 * the same number of chunks (count / chunk_size), or the ranks wait for each other in an optimiser step's all-reduce —
 * the contract callers of tg_train_chunk already have.
 * Without tg_train_create -> TG_ERR_STATE; a range outside [0, count] or a negative argument -> TG_ERR_INVALID_ARG; after an
 * error in the middle nothing of the trainer is left running.  Synchronises. */
TG_API int tg_window_train(TgEngine* e, int first, int count, uint64_t seed, float* mean_loss_p, float* mean_loss_z, int32_t* steps);

/* ---------------------------------------------------------------------------------------
 * Reanalyse: refresh the policy targets of window rows by search, on the device.  No counterpart in the reference:
 * training_loop trains on the whole window each round (train/src/main.rs:82-95), and every row keeps the visit counts
 * (Node::improved_policy, alpha-tak/src/search/play.rs:13-21) of the search that produced it, so in a long run most rows carry
 * the targets of networks many generations old.  tg_reanalyse searches the positions of logical rows [first, first + count)
 * again with the network the engine holds now and writes the new root visit counts into the rows in place (MuZero's Reanalyse,
 * restricted to the policy target).  Off unless called.
 * Search object: the call runs on the engine's live caller-driven search object (tg_search_create) and takes from it the
 * number of slots (`games`) and `batch`, the exploration constants, the seed, the arena, and the sticky modes of
 * tg_search_set_symmetry and tg_search_set_proof.  It DESTROYS that object's trees: afterwards the object holds the trees of
 * the last slice, and the caller resets it (tg_search_reset) before using it again.
 * Slices: the rows are processed `games` at a time.  For each slice (1) every slot's root state is copied from its row on the
 * device and its tree becomes Node::default(); the slots beyond a short last slice are dead, as retired self-play slots, and
 * cost nothing in the tree kernels; (2) with noise_alpha > 0: one iteration, then Node::apply_dirichlet(noise_alpha,
 * noise_ratio) — Player::add_noise's order, as the self-play driver; (3) `rollouts` iterations of `batch` virtual rollouts, the
 * schedule of tg_search_run without a mask (TG_SYMM_HASHED and TG_PROOF_ON honoured); (4) a row's visits are overwritten only
 * if the root's child count equals the row's n_moves, every child's move equals the row's move at the same index, and the
 * children's visits sum to more than 0: then visits[i] = the real visit count of child i and the entries past n_moves stay
 * zero (the row stays canonical).  Otherwise the row is left byte for byte as it was and counted as `mismatched`
 * (tg_window_push does not check that a pushed move list is possible_moves; a finished position has no children) or as
 * `unvisited` (under TG_PROOF_ON a proven root collects no visits).  State, moves, n_moves, result and game_id of a row are
 * never written, and no row outside the range is.
 * Noise key: the k-th example that ever entered the window is at cursor k, logical index i is cursor TgWindowInfo.evicted + i,
 * and for the duration of a slice the object's slot_base is the low 32 bits of its first row's cursor.  A row's noise is
 * gamma_sample(alpha, seed, (uint32_t)cursor, generation 0, ply, i): a function of the row and the seed, whatever `games` is
 * and however the range was sliced.  The object's own slot_base is back in place when the call returns.
 * Determinism: without noise a row's new visits depend on its state, the network, the search configuration and the seed
 * only — not on `games`, the slicing or the row's neighbours.
 * Errors: a null engine or cfg, first or count negative, a range outside [0, TgWindowInfo.count], rollouts < 1,
 * noise_alpha < 0, noise_ratio outside [0, 1], flags or a reserved field not 0 -> TG_ERR_INVALID_ARG naming the field; no
 * window, no search object, or a self-play object (its games would be destroyed) -> TG_ERR_STATE.  After any of these the
 * window and the search are untouched.  count = 0 -> TG_OK, zero stats.  A search error in the middle
 * (TG_ERR_ARENA_OVERFLOW, TG_ERR_LIMIT, TG_ERR_NAN) is returned: the slices stored before it keep their new visits, the
 * failing slice and those behind it are unchanged, and *out counts what was stored.
 * Host traffic: synchronises before it returns (and once per slice, for the error word).  Only lengths, flags and counters
 * reach the host: no state, move or visit of a row does.
 * ------------------------------------------------------------------------------------- */
typedef struct TgReanalyseConfig {
    int32_t rollouts;     /* search iterations per row (each `batch` virtual rollouts of the search object); >= 1 */
    float noise_alpha;    /* 0 = no Dirichlet noise */
    float noise_ratio;
    uint32_t flags;       /* must be 0 */
    int32_t reserved[4];  /* must be 0 */
} TgReanalyseConfig;      /* 32 bytes */
typedef struct TgReanalyseStats {
    uint64_t rows;        /* count */
    uint64_t updated;     /* rows whose visits were rewritten */
    uint64_t mismatched;  /* rows left as they were: root's children != the row's move list (count or any move) */
    uint64_t unvisited;   /* rows left as they were: no root child got a visit */
    uint64_t expansions, evals;  /* the search counters' growth over the call */
} TgReanalyseStats;       /* 48 bytes */
TG_API int tg_reanalyse(TgEngine* e, int first, int count, const TgReanalyseConfig* cfg, TgReanalyseStats* out /* optional */);

/* ---------------------------------------------------------------------------------------
 * Pit (replaces `pit`, train/src/pit.rs:15-96): the new network against the old one,
 * `pairs` openings × both colours, all 2·pairs games concurrently — one engine handle per weight set, each
 * holding one tree per game (the reference gives each side its own `Player`).  The side to move runs `rollouts`
 * iterations of `batch` virtual rollouts + one evaluation (reference: ROLLOUTS 50 × Player::rollout with BATCH_SIZE 16),
 * the waiting side `idle_rollouts` iterations (the batch a `Player` keeps in flight, player.rs:65-66), moves are
 * pick_move(exploit = true).  Openings: a1, a random far corner, `random_plies` random Flat/Cap placements
 * (pit.rs:33-63), drawn from Philox(seed).  All games run at once, so the early exit of pit.rs:20-23 cannot save any
 * work; its effect on the counts is reproduced in the ref_* fields (the tallies of the openings the reference's loop would
 * have played before breaking, in its order).  Not reproduced: the exact interleaving of the waiting player's stale batch
 * with the moves.  The caller applies the gate
 * (main.rs:102: win_rate > 0.55).  Both engines' search / self-play state is replaced (tg_search_create is called on
 * each); 2·pairs·batch ≤ max_batch of both engines.
 * ------------------------------------------------------------------------------------- */
typedef struct TgPitConfig {
    int32_t pairs;          /* PIT_GAMES 128 */
    int32_t rollouts;       /* ROLLOUTS 50 iterations per move */
    int32_t idle_rollouts;  /* 1 */
    int32_t random_plies;   /* RANDOM_PLIES 2 */
    int32_t komi;           /* Game::with_komi(2) */
    int32_t max_plies;      /* safety cap on the game length, 0 = none */
    int32_t arena_nodes;    /* per-game tree arena of both engines, 0 = 16384 */
    int32_t batch;          /* BATCH_SIZE 16 virtual rollouts per iteration; 0 = 1 */
    uint64_t seed;
} TgPitConfig;
typedef struct TgPitResult {
    uint32_t wins, losses, draws; /* from the new network's point of view (PitResult, pit.rs:98-103) */
    uint32_t unfinished;          /* games cut by max_plies */
    uint32_t plies;               /* lock-step plies played */
    uint32_t reserved;
    double win_rate;              /* wins / (wins + losses), pit.rs:105-110 */
    /* The same with pit.rs:20-23 applied: openings are counted in order (White game, then Black game of each) until
     * wins > pairs + pairs/10 or losses > pairs - pairs/10 holds before an opening — what `pit` returns. */
    uint32_t ref_wins, ref_losses, ref_draws;
    uint32_t ref_pairs;           /* openings counted (= pairs when the loop never breaks) */
    double ref_win_rate;
} TgPitResult;
TG_API int tg_pit(TgEngine* e_new, TgEngine* e_old, const TgPitConfig* cfg, TgPitResult* out);

/* ---------------------------------------------------------------------------------------
 * Text formats at the edge of the path (host only).  PTN moves / TPS positions follow takparse 0.5.5's
 * Display + FromStr as used by tak/src/game.rs:79 and tak/src/tps.rs:7-96; the example line follows
 * alpha-tak/src/example.rs:81-133 ("{tps};{w_stones};{w_caps};{b_stones};{b_caps};{half_komi};{result};
 * {move:visits,…}"), so drained examples can be written as the reference's `_examples/{time}.data` files.
 * format functions return the text length (≥ 0) or a negative TgStatus.
 * ------------------------------------------------------------------------------------- */
TG_API int tg_format_move(int n, TgMove mv, char* buf, size_t cap);
TG_API int tg_parse_move(int n, const char* text, TgMove* out);
TG_API int tg_format_tps(int n, const void* state, char* buf, size_t cap);
TG_API int tg_parse_tps(int n, const char* text, void* state); /* reserves derived from the board, half_komi 0 */
TG_API int tg_format_example(int n, const void* state, int n_moves, const TgMove* moves, const uint32_t* visits, float result,
                      char* buf, size_t cap);
TG_API int tg_parse_example(int n, const char* line, void* state, int cap_moves, TgMove* moves, uint32_t* visits,
                     int32_t* n_moves, float* result);

/* ---------------------------------------------------------------------------------------
 * Measurement hooks (no reference counterpart: the reference has no profiling).
 * While enabled, every `sample_every`-th network forward brackets each residual-tower 3×3 conv
 * launch with HIP events on the engine stream; tg_profile_read synchronises and returns the totals.
 * ------------------------------------------------------------------------------------- */
typedef struct TgProfile {
    uint64_t conv_launches;   /* residual-tower conv launches timed (F→F 3×3, the dominant kernel) */
    double conv_ms;           /* their summed duration                                           */
    uint64_t forwards;        /* network forwards timed end to end                               */
    double forward_ms;
    int64_t conv_rows;        /* M = positions × N² of the timed launches (all equal)            */
    int64_t conv_flops;       /* algorithmic FLOPs of one timed launch: 2·M·9·F·F (per-layer path) or, for the fused
                                 tower, 2·M·9·(C_in·F + 2R·F·F) — every input plane counted as data                */
    int64_t conv_flops_executed; /* FLOPs of the MFMAs the timed launch issues: less than conv_flops when the fused tower
                                 takes the per-position constant input planes (reserves, colour, fcd) as a bias and sums
                                 layer 0 from the set board planes' weight rows, without an MFMA — price the MFMA pipe
                                 against THIS figure                                                                */
} TgProfile;
TG_API int tg_profile_enable(TgEngine* e, int sample_every); /* 0 disables */
/* Board-path micro-benchmark: uploads n states + one legal move each, then runs `reps`
 * fused passes (Game::play → Game::result → possible_moves count → game_repr planes, all on the device,
 * inputs resident in HBM) bracketed by HIP events.  Returns the average pass time; out_* (host, optional)
 * receive the outputs of the last pass: stepped states, results, move counts. */
TG_API int tg_board_pass_bench(TgEngine* e, int n, const void* states, const TgMove* moves, int reps, double* avg_ms,
                        void* out_states, uint8_t* out_results, int32_t* out_counts);
TG_API int tg_profile_read(TgEngine* e, TgProfile* out);     /* synchronises; resets the totals */

/* A/B switches.  The library reads a fixed set of TG_* environment variables (every one is read through ONE
 * function: a switch is on when the variable is set to anything but "" or "0"; the numeric one, TG_WGRAD_PW, takes its
 * value, 0 = off).  tg_debug_switches writes the switches that are ON in this process's
 * environment as "NAME=value NAME=value …" into buf (always NUL-terminated, truncated to cap) and returns their number:
 * 0 on a measured run — bench.py prints the list as config.switches_set.  Needs no engine and no GPU. */
TG_API int tg_debug_switches(char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TAKGPU_H */
