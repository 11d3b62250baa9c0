#!/usr/bin/env python3
"""What refreshing the window's policy targets costs, beside the round trip through the host it replaces: one job, the two arms
alternating on one engine and one window:

  (a) tg_reanalyse(0, rows, rollouts)                                                       (the rows never leave the device)
  (b) tg_window_read -> tg_search_reset -> tg_search_run -> tg_search_root                  (the entry points that were there)

Configuration: config C2's network (5x5, 6 blocks x 64 filters, FC head), a window of 4096 rows filled by self-play, 4096 search
slots (one slice), 100 rollouts per row.  Arm (b) stops at search_root: the clear + tg_window_push that would put the new visits
back (and lose the ring position) is not timed.  Host clocks around each call, every one of which ends synchronised.  The
expectation to check: the searches cost the same, and (a) saves (b)'s transfers.  Beside it the cost of one self-play ply at the
same number of games and rollouts, per game, so that a row's re-search has something to stand against.  No speed is claimed and
no threshold is set.  Prints one JSON line.

    python scripts/bench_reanalyse.py [--rows 4096 --rollouts 100 --runs 2]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096, help="window rows, and search slots: one slice")
    ap.add_argument("--rollouts", type=int, default=100)
    ap.add_argument("--runs", type=int, default=2, help="per arm (one more of each runs first and is dropped)")
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--filters", type=int, default=64)
    ap.add_argument("--fill-rollouts", type=int, default=8, help="sims per move of the self-play that fills the window")
    ap.add_argument("--arena", type=int, default=1 << 14)
    args = ap.parse_args()

    import tak_amd
    import torch_ref

    rows = args.rows
    eng = tak_amd.Engine(5, res_blocks=args.blocks, filters=args.filters, evaluator=tak_amd.EVAL_RESNET, max_batch=rows)
    eng.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(5, args.blocks, args.filters, "fc5", seed=0, randomize_bn=False)))
    eng.window_create(rows)
    eng.selfplay_create(rows, arena_nodes=1 << 13, seed=0, rollouts=args.fill_rollouts, max_examples=4 * rows)
    t0 = time.perf_counter()
    while eng.window_info()["entered"] < rows:
        eng.selfplay_step(4)
        eng.window_absorb()
    fill_s = time.perf_counter() - t0

    # one self-play ply at the same games and rollouts (the middle of the games the fill has left behind would be another
    # workload: a fresh driver, a few plies in)
    eng.selfplay_create(rows, arena_nodes=args.arena, seed=1, rollouts=args.rollouts, max_examples=4 * rows)
    eng.selfplay_step(4)
    eng.sync()
    t0 = time.perf_counter()
    eng.selfplay_step(4)
    eng.sync()
    ply_ms = 1e3 * (time.perf_counter() - t0) / 4

    eng.search_create(rows, arena_nodes=args.arena, seed=2)

    def arm_a():
        t0 = time.perf_counter()
        stats = eng.reanalyse(0, rows, args.rollouts)
        return {"total_ms": 1e3 * (time.perf_counter() - t0), "stats": stats}

    def arm_b():
        out, t = {}, time.perf_counter()
        hdr, states, moves, visits = eng.window_read(0, rows)
        out["window_read_ms"], t = 1e3 * (time.perf_counter() - t), time.perf_counter()
        eng.search_reset(states)
        out["search_reset_ms"], t = 1e3 * (time.perf_counter() - t), time.perf_counter()
        eng.search_run(args.rollouts)
        eng.sync()
        out["search_run_ms"], t = 1e3 * (time.perf_counter() - t), time.perf_counter()
        root = eng.search_root()
        out["search_root_ms"] = 1e3 * (time.perf_counter() - t)
        out["total_ms"] = sum(out.values())
        out["transfers_ms"] = out["total_ms"] - out["search_run_ms"]
        # the window holds arm (a)'s visits of the same positions under the same seed: the two arms computed the same thing
        out["rows_equal_to_the_window"] = int((root["visits"] == visits).all(axis=1).sum())
        return out

    runs = {"a": [], "b": []}
    for rnd in range(args.runs + 1):  # the first run of each arm warms up and is dropped
        for arm, fn in (("a", arm_a), ("b", arm_b)):
            res = fn()
            if rnd:
                runs[arm].append(res)
    a_ms = float(np.median([r["total_ms"] for r in runs["a"]]))
    b_ms = float(np.median([r["total_ms"] for r in runs["b"]]))
    b_run = float(np.median([r["search_run_ms"] for r in runs["b"]]))
    print(json.dumps({
        "bench": "reanalyse", "topology": f"5x5 {args.blocks}x{args.filters} fc5", "rows": rows, "slots": rows, "rollouts": args.rollouts,
        "runs_per_arm": args.runs, "a_tg_reanalyse": runs["a"], "b_read_reset_run_root": runs["b"],
        "a_median_ms": a_ms, "b_median_ms": b_ms, "b_search_run_median_ms": b_run, "a_minus_b_search_run_ms": a_ms - b_run,
        "b_minus_a_ms": b_ms - a_ms, "us_per_row": {"a": 1e3 * a_ms / rows, "b": 1e3 * b_ms / rows},
        "selfplay_ply_ms": ply_ms, "selfplay_us_per_game_ply": 1e3 * ply_ms / rows, "fill_s": fill_s,
        "window": eng.window_info(), "device": eng.device_info()["name"], "switches_set": tak_amd.debug_switches(),
    }), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
