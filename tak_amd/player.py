"""`Player` (reference alpha-tak/src/player.rs:22-199) on top of the engine's search entry points — the API shape bots and
the analysis tools use for ONE game: rollout / add_noise / pick_move / play_move / get_examples / debug / get_analysis.

The reference overlaps a rollout thread with the network call (one batch of virtual rollouts always in flight).  Here the
tree lives on the GPU and `rollout` is one iteration of the one-game search with TgSearchConfig.batch = `batch`: `batch` virtual
rollouts in the tree, one network call for the leaves that are not terminal, de-virtualisation in order — the same tree
updates as Player::rollout (player.rs:77-110, 125-128), without the thread.  The engine's max_batch must be ≥ batch.  Several
Players can share one engine only one at a time (the engine holds one search state)."""
import numpy as np

from .analysis import MAX_BRANCH_LENGTH, Analysis, NodeDebugInfo, root_eval
from .engine import TG_MAX_MOVES, node_status

# node_budget of a Player's solver calls.  The library's default (2^10) is sized so that a launch over thousands of positions stays
# short on a shared card; it cannot finish the proof of a loss two plies deep (every reply × every answer: ≈ 60² positions).  A
# player solves ONE root, about a hundred work items: 2^16 positions each finish any depth-3 proof and bound a level at a fraction
# of a second.
TACTICS_BUDGET = 1 << 16


class Player:
    def __init__(self, engine, batch, save_examples, game, arena_nodes=1 << 16, seed=0, create_analysis=False, symmetry=None, tactics=0,
                 tactics_budget=TACTICS_BUDGET, proof=None, tactics_road_only=False):
        """Player::new(network, batch, save_examples, create_analysis, &game); `game` is a packed state.
        symmetry: "hashed" / SYMM_HASHED = every evaluated leaf goes to the network as a hashed dihedral image (Engine.search_set_symmetry)
        tactics: D > 0 = the analysis annotates every played move that has info with the forced-win solver at depth D (Analysis.annotate_tactics);
        0 (default) = no solver call anywhere
        tactics_budget: node_budget of this player's solver calls (pick_move's and the annotation's)
        tactics_road_only: this player's solver calls prove roads only (Engine.solve's road_only, the tinuë): pick_move plays a forced
        road and avoids moves into one, the annotation writes PTN's road marks
        proof: "on" / PROOF_ON / True = proven values in the tree (Engine.search_set_proof) and the proof-aware pick_move"""
        self.e = engine
        self.tactics = int(tactics)
        self.tactics_budget = int(tactics_budget)
        self.tactics_road_only = bool(tactics_road_only)
        self.last_tactics = None  # the Engine.search_solve result of the last pick_move(…, tactics > 0)
        self.proof = proof is not None and proof not in (0, False, "off")
        self.last_proof = None  # with proof: the Engine.search_proof result of the last pick_move
        self.batch = int(batch)
        self.save_examples = bool(save_examples)
        self.create_analysis = bool(create_analysis)
        self.examples = []  # IncompleteExample: (state, moves, visits)
        game = np.ascontiguousarray(game, np.uint8).reshape(-1)
        # Analysis::new(N, game.half_komi, game.ply) (player.rs:58) from the packed header (TgHeader: ply u16 at 2, half_komi i8 at 8)
        hdr = game[engine.sb - 16:]
        self.analysis = Analysis(engine.n, int(hdr[8:9].view(np.int8)[0]), int(hdr[2:4].view("<u2")[0]))
        self.rng = np.random.default_rng(seed)
        engine.search_create(1, arena_nodes=arena_nodes, seed=seed, batch=self.batch, symmetry=symmetry, proof=proof)
        engine.search_reset(np.ascontiguousarray(game, np.uint8).reshape(1, -1))
        self.rollout()  # the reference requests the first batch in the constructor (player.rs:65-66)

    def state(self):
        return self.e.search_states()[0]

    def rollout(self, game=None):
        """One batch of `batch` virtual rollouts from the current root (player.rs:125-128)."""
        self.e.search_run(1)

    def add_noise(self, alpha, ratio, game=None):
        """Node::apply_dirichlet on the root (player.rs:118-122)."""
        self.e.search_apply_dirichlet(alpha, ratio)

    def improved_policy(self):
        """Node::improved_policy: [(move, visits)] of the root's children."""
        r = self.e.search_root()
        c = int(r["counts"][0])
        return r["moves"][0, :c].copy(), r["visits"][0, :c].copy()

    def pick_move(self, exploitation, tactics=0):
        """Node::pick_move (play.rs:49-67): most visited (last on ties) or sampled ∝ visits.
        tactics = D > 0: first solve the root at depth D (Engine.search_solve).  A proven win returns its `best` move; otherwise
        the moves with a proven loss leave the candidates (unless every move is one).  0: no solver call, the reference's pick.
        With proof (after the tactics step, on what it left): a move into a position the tree has decided for the mover is played —
        the most visited such move, the last on ties, whatever `exploitation`; otherwise the moves decided for the opponent leave
        the candidates (unless every move is one), and candidates without any visit are picked from by exploitation."""
        moves, visits = self.improved_policy()
        if len(moves) == 0:
            raise RuntimeError("pick_move on a root without children")
        status = None
        if self.proof:
            p = self.last_proof = self.e.search_proof()
            if int(p["counts"][0]) != len(moves):
                raise RuntimeError("pick_move: the root's children are not the proof's status list")
            status = node_status(p["child_status"][0, : len(moves)])
        if tactics > 0:
            road = {"road_only": True} if self.tactics_road_only else {}
            r = self.last_tactics = self.e.search_solve(int(tactics), node_budget=self.tactics_budget, **road)
            if int(r["value"][0]) > 0:
                return int(r["best"][0])
            c = int(r["counts"][0])
            if c != len(moves) or not np.array_equal(r["moves"][0, :c], moves):
                raise RuntimeError("pick_move: the root's children are not the solver's move list")
            keep = r["move_values"][0, :c] >= 0
            if keep.any():
                moves, visits = moves[keep], visits[keep]
                status = status[keep] if status is not None else None
        if status is not None:
            mover = int(self.state()[self.e.sb - 16 + 1])
            mine = status == mover
            if mine.any():
                moves, visits = moves[mine], visits[mine]
                return int(moves[len(visits) - 1 - int(np.argmax(visits[::-1]))])
            keep = status != (mover ^ 1)
            if keep.any():
                moves, visits = moves[keep], visits[keep]
            exploitation = exploitation or int(visits.sum()) == 0
        if exploitation:
            return int(moves[len(visits) - 1 - int(np.argmax(visits[::-1]))])
        total = int(visits.sum())
        if total == 0:
            raise RuntimeError("pick_move: no visits to sample from")  # WeightedIndex panics in the reference
        return int(moves[int(self.rng.choice(len(moves), p=visits / total))])

    def debug(self, depth):
        """Node::debug(depth) of the root (player.rs:113-115): one tg_search_debug call, every child's continuation"""
        r = self.e.search_debug(depth, TG_MAX_MOVES)
        return NodeDebugInfo.from_search_debug(self.e.n, r, 0)

    def root_eval(self, ensemble=True):
        """(policy [P], eval) of the network on the current root; ensemble: the mean over all 8 dihedral images (analysis.root_eval)"""
        p, v = root_eval(self.e, self.state(), ensemble=ensemble)
        return p[0], float(v[0])

    def play_move(self, move, game=None, with_info=True):
        """Advance the tree (tree reuse) and the game; record an IncompleteExample and update the analysis (player.rs:136-166)."""
        if self.save_examples and with_info:
            moves, visits = self.improved_policy()
            self.examples.append((self.state().copy(), moves, visits))
        if self.create_analysis:
            if with_info:
                self.analysis.update(self.debug(MAX_BRANCH_LENGTH), move)
                if self.tactics > 0:
                    self.analysis.annotate_tactics(self.e, self.state(), move, self.tactics, node_budget=self.tactics_budget,
                                                   road_only=self.tactics_road_only)
            else:
                self.analysis.add_move_without_info(move)
        self.e.search_play(np.array([move], np.uint16))
        self.rollout()  # refill: the new root is expanded like the batch the reference keeps in flight

    def get_analysis(self):
        """the game's Analysis (player.rs:196-198); like std::mem::take the Player keeps an empty default one"""
        a, self.analysis = self.analysis, Analysis.default(self.e.n)
        return a

    def get_examples(self, result):
        """Complete the collected examples with the game result (TgResult code) from each mover's perspective
        (player.rs:170-193) → (states, n_moves, moves, visits, results) in the layout of tg_selfplay_drain / tg_train."""
        if result == 0:
            raise ValueError("cannot complete examples with an ongoing game")
        white = 1.0 if result in (1, 2) else -1.0 if result in (3, 4) else 0.0
        k = len(self.examples)
        sb = self.e.sb
        states = np.zeros((k, sb), np.uint8)
        n_moves = np.zeros(k, np.int32)
        moves = np.zeros((k, TG_MAX_MOVES), np.uint16)
        visits = np.zeros((k, TG_MAX_MOVES), np.uint32)
        results = np.zeros(k, np.float32)
        for i, (st, mv, vs) in enumerate(self.examples):
            states[i] = st
            n_moves[i] = len(mv)
            moves[i, : len(mv)] = mv
            visits[i, : len(mv)] = vs
            to_move = st[sb - 16 + 1]
            results[i] = white if to_move == 0 else -white
        self.examples = []
        return states, n_moves, moves, visits, results
