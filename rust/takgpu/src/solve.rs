//! Forced wins (tg_solve, tg_search_solve): an exact depth-limited AND/OR search over `Game::possible_moves` / `play` /
//! `result` on the device.  The reference has one ply of this inside `self_play_parallel` (train/src/self_play.rs:118-171,
//! the instant-win scan); the definitions of the deeper search are in `include/takgpu.h`.  "Forced win" means by road OR by
//! flats within `depth` plies, not a road-only tinuë.
use tak::{Game, Move};

use crate::{check, net::GpuNet, pack, sys};

/// `TG_SOLVE_ALL_MOVES` (an unsigned literal in the header, which the generated constants leave out)
pub const SOLVE_ALL_MOVES: u32 = 1;
/// `TG_SOLVE_ROAD_ONLY`: only roads win (the tinuë); a move that ends the game any other way proves nothing.  Bit 1 is not assigned.
pub const SOLVE_ROAD_ONLY: u32 = 4;

/// What the solver proved about one position.
#[derive(Clone, Debug)]
pub struct Solved {
    /// +d: the mover wins within d plies; -d: loses within d (longest defence); 0: nothing proven within the depth
    pub value: i8,
    /// the first winning move of the least distance; in a lost position the first move of the longest defence
    pub best: Option<Move>,
    /// every legal move in `possible_moves` order with its value (+1 wins at once, -1 loses at once, ±(1+k), 0 unproven)
    pub moves: Vec<(Move, i8)>,
    /// a work item ran out of `node_budget`: non-zero entries are still sound proofs, zeros may be missed ones
    pub budget_hit: bool,
    /// positions created by `play`
    pub nodes: u64,
}

fn config(depth: i32, flags: u32, node_budget: u64) -> sys::TgSolveConfig {
    sys::TgSolveConfig { depth: depth, flags: flags, node_budget: node_budget, reserved: [0; 4] }
}

fn all_moves_flag(all_moves: bool) -> u32 {
    if all_moves { SOLVE_ALL_MOVES } else { 0 }
}

struct Arrays {
    value: Vec<i8>,
    best: Vec<sys::TgMove>,
    counts: Vec<i32>,
    moves: Vec<sys::TgMove>,
    move_values: Vec<i8>,
    budget_hit: Vec<u8>,
    nodes: Vec<u64>,
}

impl Arrays {
    fn new(k: usize) -> Self {
        let m = sys::TG_MAX_MOVES as usize;
        Arrays {
            value: vec![0; k], best: vec![0; k], counts: vec![0; k], moves: vec![0; k * m], move_values: vec![0; k * m],
            budget_hit: vec![0; k], nodes: vec![0; k],
        }
    }

    fn unpack<const N: usize>(&self) -> Vec<Solved> {
        let m = sys::TG_MAX_MOVES as usize;
        (0..self.value.len())
            .map(|i| {
                let c = self.counts[i] as usize;
                Solved {
                    value: self.value[i],
                    best: (self.value[i] != 0).then(|| pack::move_from_code::<N>(self.best[i])),
                    moves: (0..c).map(|k| (pack::move_from_code::<N>(self.moves[i * m + k]), self.move_values[i * m + k])).collect(),
                    budget_hit: self.budget_hit[i] != 0,
                    nodes: self.nodes[i],
                }
            })
            .collect()
    }
}

impl<const N: usize> GpuNet<N> {
    /// tg_solve on `games`: needs no weights and no search.  `depth` 1 ..= TG_SOLVE_MAX_DEPTH; `all_moves` completes the move
    /// table instead of stopping at the level that decides a position; `node_budget` 0 = the library's default.
    pub fn solve(&self, games: &[Game<N>], depth: i32, all_moves: bool, node_budget: u64) -> Result<Vec<Solved>, crate::TgError> {
        self.solve_flags(games, depth, all_moves_flag(all_moves), node_budget)
    }

    /// `solve` with TgSolveConfig.flags spelled out: `SOLVE_ALL_MOVES | SOLVE_ROAD_ONLY` (road-only proofs, the tinuë)
    pub fn solve_flags(&self, games: &[Game<N>], depth: i32, flags: u32, node_budget: u64) -> Result<Vec<Solved>, crate::TgError> {
        if games.is_empty() {
            return Ok(Vec::new());
        }
        let sb = pack::state_bytes(N);
        let mut states = vec![0u8; sb * games.len()];
        for (g, chunk) in games.iter().zip(states.chunks_mut(sb)) {
            pack::pack_game(g, chunk);
        }
        let cfg = config(depth, flags, node_budget);
        let mut a = Arrays::new(games.len());
        check(unsafe {
            sys::tg_solve(self.e, games.len() as i32, states.as_ptr() as *const _, &cfg, a.value.as_mut_ptr(), a.best.as_mut_ptr(),
                          a.counts.as_mut_ptr(), a.moves.as_mut_ptr(), a.move_values.as_mut_ptr(), a.budget_hit.as_mut_ptr(),
                          a.nodes.as_mut_ptr())
        })?;
        Ok(a.unpack::<N>())
    }

    /// tg_search_solve: the current roots of the engine's live search / self-play object (`games` of them), solved in place on
    /// the device; games outside `active` and dead games come back with no moves.  The trees are not touched.
    pub fn search_solve(&self, games: usize, active: Option<&[u8]>, depth: i32, all_moves: bool, node_budget: u64)
                        -> Result<Vec<Solved>, crate::TgError> {
        self.search_solve_flags(games, active, depth, all_moves_flag(all_moves), node_budget)
    }

    /// `search_solve` with TgSolveConfig.flags spelled out (`SOLVE_ALL_MOVES | SOLVE_ROAD_ONLY`)
    pub fn search_solve_flags(&self, games: usize, active: Option<&[u8]>, depth: i32, flags: u32, node_budget: u64)
                              -> Result<Vec<Solved>, crate::TgError> {
        assert!(active.map_or(true, |m| m.len() == games), "one mask byte per game");
        let cfg = config(depth, flags, node_budget);
        let mut a = Arrays::new(games);
        check(unsafe {
            sys::tg_search_solve(self.e, &cfg, active.map_or(std::ptr::null(), <[u8]>::as_ptr), a.value.as_mut_ptr(), a.best.as_mut_ptr(),
                                 a.counts.as_mut_ptr(), a.moves.as_mut_ptr(), a.move_values.as_mut_ptr(), a.budget_hit.as_mut_ptr(),
                                 a.nodes.as_mut_ptr())
        })?;
        Ok(a.unpack::<N>())
    }

    /// tg_search_set_proof: `sys::TG_PROOF_ON` / `TG_PROOF_OFF` for the engine's live search / self-play object — proven values
    /// inside the tree (the MCTS-solver backup; takgpu.h states the rule).  Sticky until the next create.
    pub fn search_set_proof(&self, mode: i32) -> Result<(), crate::TgError> {
        check(unsafe { sys::tg_search_set_proof(self.e, mode) })
    }

    /// tg_search_get_proof: (mode, nodes proven, rollouts that ended on a proven node) since the search was created
    pub fn search_get_proof(&self) -> Result<(i32, u64, u64), crate::TgError> {
        let (mut mode, mut proven, mut ended) = (0i32, 0u64, 0u64);
        check(unsafe { sys::tg_search_get_proof(self.e, &mut mode, &mut proven, &mut ended) })?;
        Ok((mode, proven, ended))
    }

    /// tg_search_proof: per game the result code of the root and of each of its children in `possible_moves` order (0, a
    /// TgResult or a `sys::TG_PROVEN_*` code)
    pub fn search_proof(&self, games: usize) -> Result<Vec<(u8, Vec<u8>)>, crate::TgError> {
        let mut root = vec![0u8; games];
        let mut child = vec![0u8; games * pack::MAX_MOVES];
        let mut counts = vec![0i32; games];
        check(unsafe { sys::tg_search_proof(self.e, root.as_mut_ptr(), child.as_mut_ptr(), counts.as_mut_ptr()) })?;
        Ok((0..games).map(|g| (root[g], child[g * pack::MAX_MOVES..g * pack::MAX_MOVES + counts[g] as usize].to_vec())).collect())
    }
}
