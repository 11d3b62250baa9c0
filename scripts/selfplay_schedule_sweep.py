#!/usr/bin/env python3
"""What the rollout schedule (tg_selfplay_set_schedule: QUAD_ROLLOUT_PLIES, train/src/self_play.rs:19,63) costs and what it is
given for it, at config C2 (5x5, 6 x 64, FC head, 4096 games, 400 rollouts per move).

    python scripts/selfplay_schedule_sweep.py --parent-tree DIR [--warm 120] [--plies 20] [--rounds 2] [--out profiles/<name>.json]

Three arms, every run in a child process of its own (one process, one library), alternating for `--rounds` rounds because other
people's work shares the host:
    parent   schedule off on the parent commit's library (--parent-tree: a BUILT tree of that commit)
    off      schedule off on this build
    boost    boost_plies 10, boost_factor 4 on this build
A run plays `--warm` plies first — a lock-step start has every game on the same ply, so its lists are everything or nothing;
partial lists need slots that have restarted — and then times `--plies` plies, a host clock around work that ends in a device
synchronise.  Per run: expansions/s, wall time per ply, and for `boost` the counters of tg_selfplay_schedule_stats over the timed
plies: mean compacted width (compact_leaves / compact_iterations / batch) and the share of iterations that were compacted.
The summary holds
    off_vs_parent    the two medians and the parent's own spread between its runs of this job ((max - min) / median): the margin
                     within which `off` has to agree with `parent`, and whether it does
    extra_rollout    what a boosted game-rollout beyond the plain budget cost — the boost arm's extra time per ply over its extra
                     expansions per ply, both against `off` — beside the dense cost per rollout of `off`: reported, not gated
A child that fails or overruns its time limit ends the sweep: nothing further is started."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARD, BLOCKS, FILTERS, GAMES, ROLLOUTS = 5, 6, 64, 4096, 400
BOOST_PLIES, BOOST_FACTOR = 10, 4


def worker(a):
    sys.path.insert(0, a.tree)
    sys.path.insert(0, os.path.join(a.tree, "tests"))
    import torch_ref

    import tak_amd

    assert os.path.dirname(os.path.abspath(tak_amd.__file__)) == os.path.join(os.path.abspath(a.tree), "tak_amd"), tak_amd.__file__
    e = tak_amd.Engine(BOARD, res_blocks=BLOCKS, filters=FILTERS, policy_head=tak_amd.HEAD_FC5, evaluator=tak_amd.EVAL_RESNET,
                       max_batch=a.games)
    e.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(BOARD, BLOCKS, FILTERS, "fc5", seed=0, randomize_bn=False)))
    schedule = dict(boost_plies=BOOST_PLIES, boost_factor=BOOST_FACTOR) if a.arm == "boost" else {}
    e.selfplay_create(a.games, seed=0, rollouts=a.rollouts, max_examples=1 << 14, **schedule)
    e.selfplay_step(a.warm)
    e.sync()
    s0 = e.selfplay_stats()
    c0 = e.selfplay_schedule_stats() if a.arm == "boost" else None
    t0 = time.perf_counter()
    e.selfplay_step(a.plies)
    e.sync()
    dt = time.perf_counter() - t0
    s1 = e.selfplay_stats()
    out = {"what": "run", "arm": a.arm, "games": a.games, "rollouts": a.rollouts, "warm_plies": a.warm, "plies": a.plies, "seconds": dt,
           "expansions": s1["expansions"] - s0["expansions"], "expansions_per_s": (s1["expansions"] - s0["expansions"]) / dt,
           "ms_per_ply": 1e3 * dt / a.plies, "games_finished_before": s0["games_finished"], "aborted_games": s1["aborted_games"]}
    if c0 is not None:
        c1 = e.selfplay_schedule_stats()
        d = {k: c1[k] - c0[k] for k in c1}
        plain = a.plies * (a.rollouts + 1)  # iterations every arm runs: the noise iteration and the plain budget
        total = plain + (BOOST_FACTOR - 1) * a.rollouts * a.plies
        out.update(boosted_moves=d["boosted_moves"], compact_iterations=d["compact_iterations"], compact_leaves=d["compact_leaves"],
                   mean_compacted_width=d["compact_leaves"] / d["compact_iterations"] if d["compact_iterations"] else None,
                   compacted_share_of_iterations=d["compact_iterations"] / total)
    e.close()
    print(json.dumps(out), flush=True)


def child(args, limit):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"{' '.join(args)}: no result within {limit} s; nothing further is started")
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(f"{' '.join(args)}: exit status {r.returncode}; nothing further is started")
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def summarise(runs):
    by = {arm: [r for r in runs if r["arm"] == arm] for arm in ("parent", "off", "boost")}
    med = {arm: statistics.median(r["ms_per_ply"] for r in rs) for arm, rs in by.items() if rs}
    out = {"what": "summary", "ms_per_ply_median": med,
           "expansions_per_s_median": {arm: statistics.median(r["expansions_per_s"] for r in rs) for arm, rs in by.items() if rs}}
    if by["parent"] and by["off"]:
        p = [r["ms_per_ply"] for r in by["parent"]]
        margin = (max(p) - min(p)) / med["parent"]
        diff = (med["off"] - med["parent"]) / med["parent"]
        out["off_vs_parent"] = {"parent_spread": margin, "off_minus_parent": diff, "within_the_parents_spread": abs(diff) <= margin,
                                "parent_runs": len(p)}
    if by["boost"] and by["off"]:
        per_ply = lambda rs, k: statistics.median(r[k] / r["plies"] for r in rs)  # noqa: E731
        extra_ms = med["boost"] - med["off"]
        extra_exp = per_ply(by["boost"], "expansions") - per_ply(by["off"], "expansions")
        width = [r["mean_compacted_width"] for r in by["boost"] if r["mean_compacted_width"]]
        out["extra_rollout"] = {"extra_ms_per_ply": extra_ms, "extra_expansions_per_ply": extra_exp,
                                "us_per_extra_rollout": 1e3 * extra_ms / extra_exp if extra_exp else None,
                                "us_per_dense_rollout": 1e3 * med["off"] / per_ply(by["off"], "expansions"),
                                "mean_compacted_width": statistics.median(width) if width else None,
                                "compacted_share_of_iterations": statistics.median(r["compacted_share_of_iterations"] for r in by["boost"])}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", help="a built tree of the parent commit (tak_amd/libtakgpu.so, tests/torch_ref.py); without it the parent arm is left out")
    ap.add_argument("--games", type=int, default=GAMES)
    ap.add_argument("--rollouts", type=int, default=ROLLOUTS)
    ap.add_argument("--warm", type=int, default=120, help="plies played before the timed ones")
    ap.add_argument("--plies", type=int, default=20, help="timed plies per run")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--limit", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--out", help="also write the runs and the summary to this file")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--arm", choices=("parent", "off", "boost"), default="off")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    arms = ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [("off", ROOT), ("boost", ROOT)]
    common = ["--games", str(a.games), "--rollouts", str(a.rollouts), "--warm", str(a.warm), "--plies", str(a.plies)]
    runs = []
    for _ in range(a.rounds):
        for arm, tree in arms:
            runs.append(child(["--worker", "--arm", arm, "--tree", tree, *common], a.limit))
    summary = summarise(runs)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"command": "scripts/selfplay_schedule_sweep.py " + " ".join(common + ["--rounds", str(a.rounds)]),
                       "config": f"{BOARD}x{BOARD} {BLOCKS}x{FILTERS} fc5, boost_plies {BOOST_PLIES}, boost_factor {BOOST_FACTOR}",
                       "runs": runs, "summary": summary}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
