#!/usr/bin/env python3
"""Cost of tg_search_debug (Node::debug of every root, k_search_debug) on grown trees, against one lock-step search iteration of the
same width.  Run it once plain (host-to-host time per call) and once under `rocprofv3 --kernel-trace --stats -- python ...` for the
device time of k_search_debug.

    python scripts/bench_search_debug.py [--quick]

Configurations: C2 trees (5×5, 6 × 64 FC5 network, 4096 games after 400 iterations) with (depth 10, top_k 10) and (depth 10, top_k 512);
the same at 16 384 games; 32 games of the reference's 6×6 constants (16 × 128 conv network, 10 000 iterations)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tak_amd  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def _roots(n, games, seed):
    sts = orc.random_positions(n, games * 2, seed=seed, max_plies=8, half_komi=4)
    sts = sts[orc.result(n, sts) == 0][:games]
    assert len(sts) == games
    return sts


def _time(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e3


def run(name, n, blocks, filters, head, games, iters, reps):
    h = tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV
    e = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=h, evaluator=tak_amd.EVAL_RESNET, max_batch=games)
    e.init_random(seed=1)
    e.search_create(games, arena_nodes=0, seed=1)
    e.search_reset(_roots(n, games, seed=5))
    t0 = time.perf_counter()
    e.search_run(iters)
    e.sync()
    grow_ms = (time.perf_counter() - t0) * 1e3
    iter_ms = _time(lambda: (e.search_run(1), e.sync()), reps)
    out = dict(config=name, games=games, board=n, net=f"{blocks}x{filters} {head}", iterations=iters, grow_ms=round(grow_ms, 1),
               one_iteration_ms=round(iter_ms, 4))
    for depth, top_k in ((10, 10), (10, 512)):
        ms = _time(lambda: e.search_debug(depth, top_k), reps)
        r = e.search_debug(depth, top_k)
        out[f"debug_d{depth}_k{top_k}_ms_host_to_host"] = round(ms, 4)
        out[f"debug_d{depth}_k{top_k}_mean_children"] = round(float(r["counts"].mean()), 1)
        out[f"debug_d{depth}_k{top_k}_mean_cont_len"] = round(float(r["cont_len"][:, :10].mean()), 2)
    e.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, no 16 384-game run")
    a = ap.parse_args()
    reps = 3 if a.quick else 10
    run("C2", 5, 6, 64, "fc5", 4096, 400, reps)
    if not a.quick:
        run("C2x4", 5, 6, 64, "fc5", 16384, 400, reps)
    run("reference_constants", 6, 16, 128, "conv", 32, 10_000 if not a.quick else 2000, reps)


if __name__ == "__main__":
    main()
