#!/usr/bin/env python3
"""The example window beside the host path it replaces, one job, the two arms alternating round by round on one engine:

  (a) selfplay_step -> tg_selfplay_drain -> np.concatenate per drain -> tg_train            (the loop as it was)
  (b) selfplay_step -> tg_window_absorb                              -> tg_window_train      (the examples never leave the device)

Configuration: 5x5, 10 blocks x 128 filters (the C5 network), 1024 games, 20 000 examples per round, chunk_size 500.  Per arm
and round: the harvest phase (stepping until the examples are there, transfers included), the share of it spent inside drain +
concatenate / absorb with the engine already synchronised (the transfer alone), and the training phase; then per arm the median
and the spread (max - min) between its own rounds.  The chunks' GPU work is the same in both arms, so the expectation is equal
training time within arm (a)'s own spread; `train_b_minus_a_ms` against `train_spread_a_ms` says whether that held, and
`window_train_slower_beyond_spread` says so in one word.  No speed is claimed by this script.  Prints one JSON line.

    python scripts/bench_window.py [--rounds 3 --examples 20000 --games 1024 --rollouts 8]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="per arm (one more of each runs first and is dropped)")
    ap.add_argument("--examples", type=int, default=20000)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--rollouts", type=int, default=8)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--filters", type=int, default=128)
    ap.add_argument("--chunk", type=int, default=500)
    ap.add_argument("--chunks-in-step", type=int, default=4)
    args = ap.parse_args()

    import tak_amd
    import torch_ref

    n_ex = args.examples
    eng = tak_amd.Engine(5, res_blocks=args.blocks, filters=args.filters, evaluator=tak_amd.EVAL_RESNET, max_batch=args.games)
    eng.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(5, args.blocks, args.filters, "fc5", seed=0, randomize_bn=False)))
    eng.train_create(chunk_size=args.chunk, chunks_in_step=args.chunks_in_step)
    eng.window_create(n_ex)
    eng.selfplay_create(args.games, arena_nodes=1 << 13, seed=0, rollouts=args.rollouts, max_examples=4 * n_ex)

    def arm_a(seed):
        t0 = time.perf_counter()
        got, transfer = None, 0.0
        while got is None or len(got[0]) < n_ex:
            eng.selfplay_step(4)
            eng.sync()
            t = time.perf_counter()
            part = eng.selfplay_drain(n_ex)
            got = part if got is None else [np.concatenate([x, y]) for x, y in zip(got, part)]
            transfer += time.perf_counter() - t
        hdr, states, moves, visits = [a[:n_ex] for a in got]
        harvest = time.perf_counter() - t0
        t0 = time.perf_counter()
        losses = eng.train(states, hdr["n_moves"], moves, visits, hdr["result"], seed=seed)
        return harvest, transfer, time.perf_counter() - t0, losses

    def arm_b(seed):
        t0 = time.perf_counter()
        entered, transfer = 0, 0.0
        while entered < n_ex:
            eng.selfplay_step(4)
            eng.sync()
            t = time.perf_counter()
            entered += eng.window_absorb()
            transfer += time.perf_counter() - t
        eng.sync()  # the last absorb's copy kernel belongs to the harvest
        harvest = time.perf_counter() - t0
        t0 = time.perf_counter()
        losses = eng.window_train(0, n_ex, seed=seed)
        return harvest, transfer, time.perf_counter() - t0, losses

    runs = {"a": [], "b": []}
    for rnd in range(args.rounds + 1):  # the first round of each arm warms up and is dropped
        for arm, fn in (("a", arm_a), ("b", arm_b)):
            res = fn(rnd)
            if rnd:
                runs[arm].append(res)

    def summary(rows):
        out = {}
        for k, name in enumerate(("harvest_ms", "transfer_ms", "train_ms")):
            v = [1e3 * r[k] for r in rows]
            out[name] = {"rounds": v, "median": statistics.median(v), "spread": max(v) - min(v)}
        out["losses"] = [[float(x) for x in r[3]] for r in rows]
        return out

    a, b = summary(runs["a"]), summary(runs["b"])
    chunks = n_ex // args.chunk
    diff = b["train_ms"]["median"] - a["train_ms"]["median"]
    print(json.dumps({
        "bench": "window", "topology": f"5x5 {args.blocks}x{args.filters} fc5", "games": args.games, "rollouts": args.rollouts,
        "examples": n_ex, "chunk_size": args.chunk, "chunks": chunks, "rounds_per_arm": args.rounds,
        "a_drain_concatenate_train": a, "b_absorb_window_train": b,
        "train_ms_per_chunk": {"a": a["train_ms"]["median"] / chunks, "b": b["train_ms"]["median"] / chunks},
        "train_b_minus_a_ms": diff, "train_spread_a_ms": a["train_ms"]["spread"],
        "window_train_slower_beyond_spread": bool(diff > a["train_ms"]["spread"]),
        "transfer_b_minus_a_ms": b["transfer_ms"]["median"] - a["transfer_ms"]["median"],
        "window": eng.window_info(), "device": eng.device_info()["name"], "switches_set": tak_amd.debug_switches(),
    }), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
