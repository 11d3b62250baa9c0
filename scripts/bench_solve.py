#!/usr/bin/env python3
"""Times tg_solve (the forced-win solver) and fixes its default node budget.

Inputs, 4096 positions each on 5×5: mid-game positions (oracle.random_positions, plies 20 … 60) and the 400 near-end positions of
the tests (oracle.playouts(5, 400, 7)["prev"]) tiled to 4096.  Depths 1, 3 and 5, with and without TG_SOLVE_ALL_MOVES, two runs
each, HIP events on the engine's stream around the call (host copies included: the call is what a user times).  Reported per run:
positions/s, nodes/s (nodes = positions created by play, the solver's own count) and the longest single level launch, taken as
the largest step of the call time from depth L - 1 to depth L with TG_SOLVE_ALL_MOVES at the same budget (the level launches are
not timed one by one: the ABI has no hook for it).  Yardstick for nodes/s: tg_board_pass_bench (play + result + movegen + encode
per position) on the same card in the same job.

The budget ladder: the level-5 step for node_budget = 2^6 … 2^20 (every power of two from 2^8 to 2^12) on both inputs; the default is the largest power of two whose step
stays under 100 ms on both.  Whatever a wall-clock guard (--seconds) cuts off is listed under "not_measured".

    python scripts/bench_solve.py [--positions 4096] [--seconds 420] [--out profiles/r18_b_solve.json]

--road-only times TG_SOLVE_ROAD_ONLY beside the default mode instead: the same two inputs, depths 3 and 5 with the early stop, at
a budget that never gives up (2^22) and at the library's default, the arms of --arms (road, default) alternating in one job, two runs
per arm.  No ladder: the default budget was tuned on the default mode and is kept.  With TAKGPU_LIB pointing at a build of another
commit and --arms default the same job times that build's default mode.

    python scripts/bench_solve.py --road-only [--arms road,default] [--out profiles/r24_b_tinue.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import tak_amd  # noqa: E402
from oracle import oracle  # noqa: E402  (position generator only)


class Events:
    def __init__(self, engine):
        self.lib, self.stream = engine.lib, C.c_void_p(engine.stream)
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert self.lib.hipEventCreate(C.byref(self.a)) == 0 and self.lib.hipEventCreate(C.byref(self.b)) == 0

    def time_ms(self, fn):
        assert self.lib.hipEventRecord(self.a, self.stream) == 0
        out = fn()
        assert self.lib.hipEventRecord(self.b, self.stream) == 0 and self.lib.hipEventSynchronize(self.b) == 0
        ms = C.c_float(0)
        assert self.lib.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return float(ms.value), out


def inputs(count):
    sts = oracle.random_positions(5, 3 * count, seed=18, max_plies=60)
    ply = sts[:, 256 - 16 + 2 : 256 - 16 + 4].copy().view("<u2").ravel()
    mid = sts[(ply >= 20) & (oracle.result(5, sts) == 0)][:count]
    assert len(mid) == count, "not enough mid-game positions"
    end = np.tile(oracle.playouts(5, 400, 7)["prev"], ((count + 399) // 400, 1))[:count]
    return {"midgame_plies_20_60": mid, "near_end_400_tiled": np.ascontiguousarray(end)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--seconds", type=float, default=420.0)
    ap.add_argument("--out", default=None, help="default: profiles/r18_b_solve.json, with --road-only profiles/r24_b_tinue.json")
    ap.add_argument("--road-only", action="store_true", help="time TG_SOLVE_ROAD_ONLY against the default mode (no budget ladder)")
    ap.add_argument("--arms", default="road,default", help="with --road-only: the arms to time, alternating")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r24_b_tinue.json" if args.road_only else "r18_b_solve.json")
    t0 = time.time()
    e = tak_amd.Engine(5, evaluator=tak_amd.EVAL_HASH, max_batch=args.positions, policy_head=tak_amd.HEAD_FC5)
    ev = Events(e)
    sets = inputs(args.positions)
    doc = {"device": e.device_info(), "positions": args.positions, "runs": [], "ladder": [], "not_measured": []}

    # yardstick: the board pass on the same positions (every position plays its first legal move)
    mid = sets["midgame_plies_20_60"]
    moves, _ = e.movegen(mid)
    ms, *_ = e.board_pass_bench(mid, moves[:, 0], reps=20)
    doc["board_pass"] = {"ms_per_pass": ms, "positions_per_s": args.positions / ms * 1e3}
    print(f"board pass: {ms:.4f} ms per {args.positions} positions = {doc['board_pass']['positions_per_s']:.3e} positions/s", flush=True)

    def run(name, depth, all_moves, budget, road_only=False):
        road = {"road_only": True} if road_only else {}
        ms, r = ev.time_ms(lambda: e.solve(sets[name], depth, all_moves=all_moves, node_budget=budget, **road))
        nodes = int(r["nodes"].sum())
        return {"input": name, "depth": depth, "all_moves": all_moves, "node_budget": budget, "ms": ms,
                "positions_per_s": args.positions / ms * 1e3, "nodes": nodes, "nodes_per_s": nodes / ms * 1e3,
                "nodes_per_s_over_board_pass": nodes / ms * 1e3 / doc["board_pass"]["positions_per_s"],
                "budget_hit_positions": int(r["budget_hit"].sum()), "proven_positions": int((r["value"] != 0).sum())}

    big = 1 << 22
    e.solve(mid[:64], 3)  # warm-up: code objects loaded, scratch allocated
    if args.road_only:
        arms = [a for a in args.arms.split(",") if a]
        assert arms and set(arms) <= {"road", "default"}, "--arms takes road and default"
        doc.update(library="TAKGPU_LIB" if os.environ.get("TAKGPU_LIB") else "this tree", arms=arms)
        del doc["ladder"]
        if "road" in arms:
            e.solve(mid[:64], 3, road_only=True)
        for name in sets:
            for depth in (3, 5):
                for budget in (big, 0):
                    for rep in range(2):
                        for arm in arms:
                            if time.time() - t0 > args.seconds:
                                doc["not_measured"].append(f"run {name} depth {depth} node_budget {budget} arm {arm} rep {rep}")
                                continue
                            row = dict(run(name, depth, False, budget, arm == "road"), arm=arm, rep=rep)
                            doc["runs"].append(row)
                            print(json.dumps(row), flush=True)
        doc["seconds"] = time.time() - t0
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"wrote {args.out}", flush=True)
        e.close()
        return
    for name in sets:
        for all_moves in (False, True):
            for depth in (1, 3, 5):
                for rep in range(2):
                    if time.time() - t0 > args.seconds:
                        doc["not_measured"].append(f"run {name} depth {depth} all_moves {all_moves} rep {rep}")
                        continue
                    row = dict(run(name, depth, all_moves, big), rep=rep)
                    doc["runs"].append(row)
                    print(json.dumps(row), flush=True)
    # the ladder: step of the call time from depth 4 to depth 5 = the level-5 launch (and its fold)
    for shift in (6, 8, 9, 10, 11, 12, 14, 16, 18, 20):  # every power of two around the 100 ms line, steps of 4 away from it
        for name in sets:
            if time.time() - t0 > args.seconds:
                doc["not_measured"].append(f"ladder {name} node_budget 2^{shift}")
                continue
            d4, d5 = run(name, 4, True, 1 << shift), run(name, 5, True, 1 << shift)
            row = {"input": name, "node_budget": 1 << shift, "depth4_ms": d4["ms"], "depth5_ms": d5["ms"], "level5_step_ms": d5["ms"] - d4["ms"],
                   "budget_hit_positions": d5["budget_hit_positions"], "proven_positions": d5["proven_positions"], "nodes": d5["nodes"]}
            doc["ladder"].append(row)
            print(json.dumps(row), flush=True)
    ok = {}
    for row in doc["ladder"]:
        ok.setdefault(row["node_budget"], []).append(row["level5_step_ms"] < 100.0)
    fits = [b for b, v in ok.items() if len(v) == len(sets) and all(v)]
    doc["default_budget_by_the_rule"] = max(fits) if fits else None
    doc["seconds"] = time.time() - t0
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"default budget by the rule: {doc['default_budget_by_the_rule']}; wrote {args.out}", flush=True)
    e.close()


if __name__ == "__main__":
    main()
