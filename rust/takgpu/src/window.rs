//! The `examples` of `training_loop` (train/src/main.rs:26,56-123) on the device: one window of the latest `capacity`
//! examples owned by the engine (tg_window_*).  Self-play rounds are absorbed into it without leaving the GPU, `.data` files
//! are pushed into it, and the network trains on all of it — the reference's `Vec<Example>` with its truncation to
//! MAX_EXAMPLES (main.rs:110-115), without 1.3 GB of rows on the host.
//!
//! An engine has at most one window and owns it, so these are methods of [`GpuNet`], not a handle of their own: what changes
//! the window takes `&mut self`, there is nothing to drop out of order, and the window lives until `window_create(0)` or the
//! network's own end — across `tg_selfplay_create`, trainers, commits and pits.
use alpha_tak::Example;

use crate::{check, net::GpuNet, pack, sys};

impl<const N: usize> GpuNet<N> {
    /// `let mut examples = Vec::new()` with MAX_EXAMPLES = `capacity` (main.rs:26,56): (re)creates an EMPTY window — the examples
    /// of an earlier one are gone; 0 frees it.
    pub fn window_create(&mut self, capacity: i32) -> Result<(), crate::TgError> {
        check(unsafe { sys::tg_window_create(self.e, capacity) })
    }

    /// capacity, count, entered, evicted
    pub fn window_info(&self) -> Result<sys::TgWindowInfo, crate::TgError> {
        let mut out = sys::TgWindowInfo { capacity: 0, count: 0, entered: 0, evicted: 0 };
        check(unsafe { sys::tg_window_info(self.e, &mut out) })?;
        Ok(out)
    }

    pub fn window_clear(&mut self) -> Result<(), crate::TgError> {
        check(unsafe { sys::tg_window_clear(self.e) })
    }

    /// `examples.extend(new_examples)` + the truncation (main.rs:106-115) for everything the self-play ring has finished,
    /// on the device; shares `tg_selfplay_drain`'s cursor.  Returns how many entered.
    pub fn window_absorb(&mut self) -> Result<i32, crate::TgError> {
        let mut n = 0i32;
        check(unsafe { sys::tg_window_absorb(self.e, &mut n) })?;
        Ok(n)
    }

    /// The examples of a `.data` file (main.rs:58-80), validated before any of them enters
    pub fn window_push(&mut self, examples: &[Example<N>]) -> Result<(), crate::TgError> {
        let refs: Vec<&Example<N>> = examples.iter().collect();
        let a = pack::pack_examples::<N>(&refs);
        check(unsafe {
            sys::tg_window_push(self.e, refs.len() as i32, a.states.as_ptr() as *const _, a.n_moves.as_ptr(), a.moves.as_ptr(),
                                a.visits.as_ptr(), a.results.as_ptr(), std::ptr::null())
        })
    }

    /// Logical `[first, first + n)` (0 = oldest) back on the host: what main.rs:117-121 writes to a `.data` file
    pub fn window_read(&self, first: i32, n: i32) -> Result<Vec<Example<N>>, crate::TgError> {
        let (k, sb) = (n.max(0) as usize, pack::state_bytes(N));
        let mut headers = vec![sys::TgExampleHeader { game_id: 0, n_moves: 0, result: 0.0, reserved: 0 }; k];
        let mut states = vec![0u8; k * sb];
        let mut moves = vec![0u16; k * pack::MAX_MOVES];
        let mut visits = vec![0u32; k * pack::MAX_MOVES];
        check(unsafe {
            sys::tg_window_read(self.e, first, n, headers.as_mut_ptr(), states.as_mut_ptr() as *mut _, moves.as_mut_ptr(),
                                visits.as_mut_ptr())
        })?;
        Ok((0..k)
            .map(|i| {
                pack::unpack_example::<N>(&headers[i], &states[i * sb..(i + 1) * sb], &moves[i * pack::MAX_MOVES..(i + 1) * pack::MAX_MOVES],
                                          &visits[i * pack::MAX_MOVES..(i + 1) * pack::MAX_MOVES])
            })
            .collect())
    }

    /// `Network::train` (network.rs:37-56) on logical `[first, first + count)` — the trainer is created on first use, as in
    /// `try_train` — then the commit `try_train` makes: (mean loss_p, mean loss_z, optimiser steps).
    /// Data parallel: every rank passes a `count` with the same count / chunk_size (no verdicts are exchanged).
    pub fn window_train(&mut self, first: i32, count: i32, seed: u64) -> Result<(f32, f32, i32), crate::TgError> {
        let e = self.trainer_handle()?;
        let (mut lp, mut lz, mut steps) = (0f32, 0f32, 0i32);
        check(unsafe { sys::tg_window_train(e, first, count, seed, &mut lp, &mut lz, &mut steps) })?;
        check(unsafe { sys::tg_train_commit(e) })?;
        Ok((lp, lz, steps))
    }
}
