#!/usr/bin/env python3
"""End-to-end rehearsal of config C5 on one GPU: self-play → examples → Network::train → commit → self-play again.
Everything runs through the C ABI (no CPU checker involved).  Prints timings of the training step.

    python scripts/train_loop.py [--blocks 10 --filters 128 --games 1024 --rollouts 32 --examples 4000]

--holdout FRACTION (default 0: nothing changes) harvests FRACTION x examples more per round, keeps a seeded share of that
size out of tg_train and prints the deployed network's losses on it (tg_eval_examples: folded BatchNorm, running statistics)
before training and for the candidate after tg_train_commit, beside the pit line.  Under a launcher (RANK / WORLD_SIZE) every
rank plays and holds out its own games and the sums are added over the ranks (tak_amd.dist.reduce_example_sums).

--window N (default 0: the loop exactly as it is) is the training_loop of train/src/main.rs:56-123: the examples stay on the
device.  Every round's harvest is absorbed from the self-play ring into a window of the latest N examples (tg_window_absorb) and
the network trains on the whole window (tg_window_train), not on the fresh harvest only; nothing is drained, concatenated or
uploaded.  With --holdout the newest share of the window is read back (tg_window_read) for tg_eval_examples and kept out by
training on the range before it; it is trained on from the next round on, when newer examples have taken its place.

--reanalyse-rows N (default 0: the loop as it was; needs --window) refreshes the policy targets of the OLDEST min(N, count) rows of
the window every round, after the absorb and before the training: tg_reanalyse searches their positions again with the network that
has just played, --reanalyse-rollouts iterations each (0 = --rollouts), on a search object created for the purpose, and writes
the new visit counts into the rows on the device.  That object replaces the self-play driver, so self-play is created anew at
the end of the round, as it is after a pit.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def holdout_split(n, hold, seed):
    """(train indices, held-out indices) of a harvest of n examples: `hold` of them, drawn by a permutation seeded with
    `seed`, are kept out of training; both lists keep the harvest's order.  hold = 0 → (every index, none)."""
    if hold <= 0:
        return np.arange(n), np.zeros(0, np.int64)
    held = np.sort(np.random.default_rng(seed).permutation(n)[:hold])
    keep = np.ones(n, bool)
    keep[held] = False
    return np.flatnonzero(keep), held


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--board", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--rollouts", type=int, default=32)
    ap.add_argument("--examples", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--chunks-in-step", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--pit-pairs", type=int, default=0, help="> 0: gate every round with tg_pit (train/src/main.rs:98-106)")
    ap.add_argument("--pit-rollouts", type=int, default=50, help="batches per move (pit.rs ROLLOUTS)")
    ap.add_argument("--pit-batch", type=int, default=16, help="virtual rollouts per batch (pit.rs BATCH_SIZE)")
    ap.add_argument("--pit-arena", type=int, default=0, help="average node budget per pit game (TgPitConfig.arena_nodes); 0 = the library's "
                    "16384, as before — --pit-rollouts x --pit-batch = 800 expansions per move exhaust that within a few moves: pass 262144")
    ap.add_argument("--holdout", type=float, default=0.0, help="> 0: harvest this fraction of --examples more, keep it out of training and "
                    "print the network's losses on it before training and after the commit (tg_eval_examples)")
    ap.add_argument("--holdout-seed", type=int, default=0, help="seed of the held-out share (round r uses [seed, r])")
    ap.add_argument("--boost-plies", type=int, default=0, help="> 0: moves below this ply get --boost-factor times the rollouts "
                    "(QUAD_ROLLOUT_PLIES, train/src/self_play.rs:19,63: 10); 0 = off")
    ap.add_argument("--boost-factor", type=int, default=1, help="rollout multiple of a boosted move (the reference: 4); 1 = off")
    ap.add_argument("--symmetry", choices=("off", "hashed"), default="off", help="hashed: self-play and the pit send every leaf to the "
                    "network as a pseudo-random dihedral image (tg_search_set_symmetry); with --holdout the report also carries the "
                    "network's distance from equivariance")
    ap.add_argument("--proof", choices=("off", "on"), default="off", help="on: self-play keeps proven values in its trees and picks "
                    "its moves proof-aware (tg_search_set_proof); the pit is not affected")
    ap.add_argument("--window", type=int, default=0, help="> 0: keep the latest N examples in a window on the device and train on all of "
                    "it every round (MAX_EXAMPLES, train/src/main.rs:26: 400000); 0 = train on the fresh harvest only")
    ap.add_argument("--reanalyse-rows", type=int, default=0, help="> 0: every round, search the oldest N rows of the window again with the "
                    "current network and rewrite their visit counts on the device (tg_reanalyse); needs --window; 0 = off")
    ap.add_argument("--reanalyse-rollouts", type=int, default=0, help="search iterations per reanalysed row; 0 = --rollouts")
    args = ap.parse_args(argv)
    if args.reanalyse_rows < 0 or args.reanalyse_rollouts < 0:
        ap.error("--reanalyse-rows and --reanalyse-rollouts must not be negative")
    if args.reanalyse_rows and not args.window:
        ap.error("--reanalyse-rows refreshes rows of the example window: it needs --window")
    if args.window < 0:
        ap.error("--window must be 0 (off) or a number of examples")
    if not 0 <= args.boost_plies <= 512:
        ap.error("--boost-plies must be in 0..512 (TG_LIMIT_GAME_PLIES)")
    if not 1 <= args.boost_factor <= 64:
        ap.error("--boost-factor must be in 1..64")
    if args.rollouts * args.boost_factor > 2**31 - 1:
        ap.error("--rollouts x --boost-factor must fit an int32")
    if not 0.0 <= args.holdout < 1.0:
        ap.error("--holdout must be in [0, 1)")
    if args.window and args.window <= int(round(args.holdout * args.examples)):
        ap.error("--window must hold more than the held-out share (--holdout x --examples)")
    return args


def main():
    args = parse_args()

    import tak_amd
    import torch_ref  # random-init weights in tch layout (PyTorch default init)
    from tak_amd import dist as tdist

    hold = int(round(args.holdout * args.examples))
    harvest = args.examples + hold
    rank, world, group = 0, 1, None
    if hold:  # the held-out sums of all ranks are added; without --holdout the loop stays the single-process rehearsal it was
        rank, world, _ = tdist.env_rank()
        group = tdist.init("gloo", rank, world)
    head = "fc5" if args.board == 5 else "conv"
    net = torch_ref.make_net(args.board, args.blocks, args.filters, head, seed=0, randomize_bn=False)
    eng = tak_amd.Engine(args.board, res_blocks=args.blocks, filters=args.filters, evaluator=tak_amd.EVAL_RESNET, max_batch=args.games)
    tensors = torch_ref.abi_tensors(net)
    eng.load_state_dict(tensors)
    eng.train_create(chunk_size=args.chunk, chunks_in_step=args.chunks_in_step)
    if args.window:
        eng.window_create(args.window)  # outlives every selfplay_create / train_create / commit / pit below
    old = None
    if args.pit_pairs:
        old = tak_amd.Engine(args.board, res_blocks=args.blocks, filters=args.filters, evaluator=tak_amd.EVAL_RESNET,
                             max_batch=2 * args.pit_pairs * args.pit_batch)
        old.load_state_dict(tensors)
    schedule = dict(boost_plies=args.boost_plies, boost_factor=args.boost_factor, symmetry=args.symmetry, proof=args.proof)
    eng.selfplay_create(args.games, arena_nodes=1 << 13, seed=0, rollouts=args.rollouts, max_examples=4 * harvest,
                        slot_base=tdist.slot_base(rank, args.games), **schedule)
    report = []
    for rnd in range(args.rounds):
        t0 = time.perf_counter()
        held_out = None
        if args.window:
            entered = 0
            while entered < harvest:  # examples.extend(new_examples) + the truncation (main.rs:106-115), on the device
                eng.selfplay_step(4)
                entered += eng.window_absorb()
            t_sp = time.perf_counter() - t0
            n_train = eng.window_info()["count"] - hold  # the newest `hold` examples are the held-out share
            if hold:
                h_hdr, h_states, h_moves, h_visits = eng.window_read(n_train, hold)
                held_ex = (h_states, h_hdr["n_moves"], h_moves, h_visits, h_hdr["result"])
        else:
            got = [np.zeros((0,), tak_amd.engine.EXAMPLE_HEADER), np.zeros((0, eng.sb), np.uint8), np.zeros((0, 512), np.uint16), np.zeros((0, 512), np.uint32)]
            while len(got[0]) < harvest:
                eng.selfplay_step(4)
                eng.sync()
                part = eng.selfplay_drain(harvest)
                got = [np.concatenate([a, b]) for a, b in zip(got, part)]
            t_sp = time.perf_counter() - t0
            hdr, states, moves, visits = [a[:harvest] for a in got]
            if hold:
                keep, held = holdout_split(harvest, hold, [args.holdout_seed, rnd])
                held_ex = (states[held], hdr["n_moves"][held], moves[held], visits[held], hdr["result"][held])
                hdr, states, moves, visits = hdr[keep], states[keep], moves[keep], visits[keep]
            n_train = len(hdr)
        if hold:

            def held_means():  # the sums of every rank's held-out examples, then the means
                return tak_amd.engine.example_means(tdist.reduce_example_sums(group, eng.evaluate_examples(*held_ex)["sums"]))

            def equivariance():  # mean |p − p̄| and |v − v̄| between the plain and the 8-image ensembled evaluation, over every rank's share
                p, v = eng.policy_eval(held_ex[0])
                pe, ve = eng.policy_eval(held_ex[0], symmetries=0xFF)
                mine = [float(np.abs(p - pe).sum(dtype=np.float64)), float(p.size), float(np.abs(v - ve).sum(dtype=np.float64)), float(v.size)]
                dp, n_p, dv, n_v = (sum(col) for col in zip(*tdist.gather(group, mine)))  # the ranks' sums in f64, then the means
                return {"mean_abs_dp": dp / n_p if n_p else None, "mean_abs_dv": dv / n_v if n_v else None}

            held_out = {"examples": hold * world, "before": held_means(), "equivariance_before": equivariance()}
        reanalysed = None
        if args.reanalyse_rows:
            # the oldest rows carry the targets of the oldest networks.  A search object of its own (it replaces the self-play
            # driver: what the ring had not yet handed to the window is dropped, as at the pit's re-creation below)
            t0 = time.perf_counter()
            eng.search_create(args.games, arena_nodes=1 << 13, seed=rnd, symmetry=args.symmetry, proof=args.proof)
            reanalysed = eng.reanalyse(0, min(args.reanalyse_rows, eng.window_info()["count"]), args.reanalyse_rollouts or args.rollouts)
            reanalysed["seconds"] = time.perf_counter() - t0
            print(json.dumps({"round": rnd, "reanalyse": reanalysed}), flush=True)
        t0 = time.perf_counter()
        if args.window:
            # A fresh optimiser on the whole window (main.rs:82-95).  tg_window_train exchanges no verdicts between ranks: this loop
            # attaches no communicator, so each rank's own n_train is fine.  With one attached, the ranks' windows fill differently
            # until they are full, and every rank must pass a count with the same count // chunk (agree on the minimum first), or
            # the ranks wait for each other in an optimiser step's all-reduce.
            lp, lz, steps = eng.window_train(0, n_train, seed=rnd)
        else:
            lp, lz, steps = eng.train(states, hdr["n_moves"], moves, visits, hdr["result"], seed=rnd)
        t_tr = time.perf_counter() - t0
        t0 = time.perf_counter()
        eng.train_commit()
        t_commit = time.perf_counter() - t0
        if held_out is not None:  # the candidate, as the pit is about to play it
            held_out["after"] = held_means()
            held_out["equivariance_after"] = equivariance()
        gate = None
        if old is not None:  # training_loop: keep the new network only if it beats the old one (WIN_RATE_THRESHOLD 0.55)
            t0 = time.perf_counter()
            gate = tak_amd.pit(eng, old, pairs=args.pit_pairs, rollouts=args.pit_rollouts, batch=args.pit_batch, idle_rollouts=1, seed=rnd, max_plies=200,
                               arena_nodes=args.pit_arena, symmetry=args.symmetry)
            gate["seconds"] = time.perf_counter() - t0
            new_tensors = {k: eng.train_get_tensor(k, v.shape) for k, v in tensors.items()}
            if gate["win_rate"] > 0.55:
                tensors = new_tensors
                old.load_state_dict(tensors)
            else:  # drop the trained copy: back to the old parameters, fresh trainer
                eng.load_state_dict(tensors)
                eng.train_create(chunk_size=args.chunk, chunks_in_step=args.chunks_in_step)
            gate["accepted"] = gate["win_rate"] > 0.55
        if old is not None or args.reanalyse_rows:  # the pit and the reanalysis both replaced the self-play driver
            eng.selfplay_create(args.games, arena_nodes=1 << 13, seed=rnd + 1, rollouts=args.rollouts, max_examples=4 * harvest,
                                slot_base=tdist.slot_base(rank, args.games), **schedule)
        chunks = n_train // args.chunk if args.window else args.examples // args.chunk
        report.append({"round": rnd, "selfplay_s": t_sp, "examples": int(n_train), "train_s": t_tr, "chunks": chunks, "steps": steps,
                       "ms_per_chunk": 1e3 * t_tr / max(chunks, 1), "positions_per_s": chunks * args.chunk * 8 / t_tr,
                       "loss_p": lp, "loss_z": lz, "commit_s": t_commit, "pit": gate, "stats": eng.selfplay_stats()})
        if held_out is not None:
            report[-1]["holdout"] = held_out
        if args.window:
            report[-1]["window"] = eng.window_info()
        if reanalysed is not None:
            report[-1]["reanalyse"] = reanalysed
        print(json.dumps(report[-1]), flush=True)
    eng.close()
    if old is not None:
        old.close()


if __name__ == "__main__":
    main()
