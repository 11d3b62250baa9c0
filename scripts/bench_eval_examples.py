#!/usr/bin/env python3
"""Throughput of tg_eval_examples beside the plain forward (tg_policy_eval) on the same drained self-play examples, one job,
alternating: C2 topology (5x5, 6 blocks, 64 filters, FC head), 32 768 examples, with and without symmetries.  Prints one JSON line:
seconds (median of --reps) and positions per second of each, and the ratios of the per-position times to tg_policy_eval's — the
figure of merit: the transforms, the metric kernel and the sums should be a small share of the forward.  (tg_policy_eval also
copies the n x P probabilities to the host, which tg_eval_examples does not: a ratio below 1 is that copy.)

    python scripts/bench_eval_examples.py [--examples 32768 --max-batch 4096 --reps 5]
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
    ap.add_argument("--examples", type=int, default=32768)
    ap.add_argument("--max-batch", type=int, default=4096)
    ap.add_argument("--games", type=int, default=2048)
    ap.add_argument("--rollouts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="f32", choices=["f32", "bf16x3"])
    args = ap.parse_args()

    import tak_amd
    import torch_ref

    eng = tak_amd.Engine(5, res_blocks=6, filters=64, evaluator=tak_amd.EVAL_RESNET, max_batch=args.max_batch)
    if args.precision != "f32":
        eng.set_precision(args.precision)
    eng.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(5, 6, 64, "fc5", seed=0, randomize_bn=False)))
    eng.selfplay_create(args.games, arena_nodes=1 << 12, seed=0, rollouts=args.rollouts, max_examples=2 * args.examples)
    got = None
    t0 = time.perf_counter()
    while got is None or len(got[0]) < args.examples:
        eng.selfplay_step(8)
        eng.sync()
        part = eng.selfplay_drain(args.examples)
        got = part if got is None else [np.concatenate([a, b]) for a, b in zip(got, part)]
    t_selfplay = time.perf_counter() - t0
    hdr, states, moves, visits = [np.ascontiguousarray(a[: args.examples]) for a in got]
    ex = (states, np.ascontiguousarray(hdr["n_moves"]), moves, visits, np.ascontiguousarray(hdr["result"]))

    def timed(fn):
        t = time.perf_counter()
        out = fn()
        return time.perf_counter() - t, out

    runs = {"policy_eval": [], "eval_examples": [], "eval_examples_symmetries": []}
    plain = symm = None
    for rep in range(args.reps + 1):  # the first round warms up and is dropped
        a, _ = timed(lambda: eng.policy_eval(states))
        b, plain = timed(lambda: eng.evaluate_examples(*ex))
        c, symm = timed(lambda: eng.evaluate_examples(*ex, symmetries=True))
        if rep:
            runs["policy_eval"].append(a)
            runs["eval_examples"].append(b)
            runs["eval_examples_symmetries"].append(c)
    n = args.examples
    med = {k: statistics.median(v) for k, v in runs.items()}
    per_pos = {"policy_eval": med["policy_eval"] / n, "eval_examples": med["eval_examples"] / n,
               "eval_examples_symmetries": med["eval_examples_symmetries"] / (8 * n)}
    print(json.dumps({
        "bench": "eval_examples", "topology": "C2 5x5 6x64 fc5", "precision": args.precision, "examples": n, "max_batch": args.max_batch,
        "reps": args.reps, "selfplay_s": t_selfplay, "seconds_median": med, "seconds_all": runs,
        "positions_per_s": {k: 1.0 / v for k, v in per_pos.items()},
        "ratio_to_policy_eval_per_position": {k: per_pos[k] / per_pos["policy_eval"] for k in ("eval_examples", "eval_examples_symmetries")},
        "means": {k: plain[k] for k in ("loss_p", "loss_z", "kl", "top1", "value_sign")},
        "means_symmetries": {k: symm[k] for k in ("loss_p", "loss_z", "kl", "top1", "value_sign")},
        "device": eng.device_info()["name"], "switches_set": tak_amd.debug_switches(),
    }), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
