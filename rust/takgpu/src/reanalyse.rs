//! Reanalyse (tg_reanalyse): the policy targets of window rows refreshed by a search with the network the engine holds now, on
//! the device.  No counterpart in the reference: `training_loop` trains on the whole window each round
//! (train/src/main.rs:82-95) with the `improved_policy` (alpha-tak/src/search/play.rs:13-21) of whichever network searched an
//! example when it was born.  `include/takgpu.h` states which rows are rewritten and which are left as they were.
use crate::{check, net::GpuNet, sys};

impl<const N: usize> GpuNet<N> {
    /// tg_search_create: the caller-driven search object [`GpuNet::reanalyse`] runs on — `games` rows per slice, `batch`
    /// virtual rollouts per iteration (games × batch ≤ max_batch), `arena_nodes` per slot on average (0 = automatic).  It
    /// REPLACES a live self-play driver: create it between rounds, as main.rs:82-122 recreates self-play after every pit.
    pub fn reanalyse_search_create(&mut self, games: i32, batch: u32, arena_nodes: i32, seed: u64) -> Result<(), crate::TgError> {
        let scfg = sys::TgSearchConfig {
            games: games,
            arena_nodes: arena_nodes,
            exploration_base: 500.0, // EXPLORATION_BASE, alpha-tak/src/search/mcts.rs:7
            exploration_init: 4.0,   // EXPLORATION_INIT, mcts.rs:8
            seed: seed,
            slot_base: 0, // tg_reanalyse keys a row's noise by the row's cursor, not by this
            batch: batch,
            visit_limit: 0, // TG_LIMIT_VISITS
            reserved: 0,
        };
        check(unsafe { sys::tg_search_create(self.e, &scfg) })
    }

    /// Logical window rows `[first, first + count)` (0 = oldest) searched again for `rollouts` iterations each and their visit
    /// counts rewritten in place; `noise_alpha` 0 = no Dirichlet noise.  The search object's trees are destroyed.  Returns the
    /// counts: rows, updated, mismatched, unvisited, and the growth of the search counters.
    pub fn reanalyse(&mut self, first: i32, count: i32, rollouts: i32, noise_alpha: f32, noise_ratio: f32)
                     -> Result<sys::TgReanalyseStats, crate::TgError> {
        let cfg = sys::TgReanalyseConfig { rollouts: rollouts, noise_alpha: noise_alpha, noise_ratio: noise_ratio, flags: 0, reserved: [0; 4] };
        let mut out = sys::TgReanalyseStats { rows: 0, updated: 0, mismatched: 0, unvisited: 0, expansions: 0, evals: 0 };
        check(unsafe { sys::tg_reanalyse(self.e, first, count, &cfg, &mut out) })?;
        Ok(out)
    }
}
