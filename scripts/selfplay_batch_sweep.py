#!/usr/bin/env python3
"""What TgSelfPlayConfig.batch is worth in the narrow regime: the reference's own constants (6x6, `Net6` 16 x 128, conv head,
32 lock-step games; train/src/self_play.rs) with the rollouts per move scaled down so that a point takes seconds.

    python scripts/selfplay_batch_sweep.py [--batches 1,4,8,16,32] [--rollouts 40] [--plies 2] [--reps 5]
                                           [--parent-tree DIR] [--no-profile] [--trace-dir DIR] > profiles/<name>.jsonl

One JSON line per measurement, every measurement in a child process of its own (one process, one library):
  {"what": "selfplay", "batch": B, ...}   self-play at batch B: after one warm-up ply, `reps` windows of `plies` plies each, a host
      clock around work that ends in a device synchronise; expansions/s and ms per lock-step iteration (rollouts + 1 root
      evaluation per ply) as the median over the windows, with the smallest and largest window beside it.
  {"what": "tree_share", "batch": B, ...} the same run once more under `rocprofv3 --kernel-trace --stats`, a run of its own: the
      share of the summed kernel time that the tree kernels (k_select, k_backup, k_backup_select, k_backup_select_batch) take.
  {"what": "search", "tree": ..., "batch": B, ...}  with --parent-tree DIR (a BUILT tree of the parent commit, which cannot batch
      self-play): `tg_search_run(iters)` at batch 16 and 32 on both trees, this one (one fused tree kernel per iteration) and the
      parent (k_backup, then k_select), alternating between the two for `--rounds` rounds; ms per iteration per window.
A child that fails or overruns its time limit ends the sweep: nothing further is started."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARD, BLOCKS, FILTERS, GAMES = 6, 16, 128, 32
TREE_KERNELS = ("k_select", "k_backup")  # prefixes of the demangled names: k_backup covers k_backup_select and k_backup_select_batch


def _engine(tree, max_batch):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch_ref

    import tak_amd

    weights = torch_ref.abi_tensors(torch_ref.make_net(BOARD, BLOCKS, FILTERS, "conv", seed=0, randomize_bn=False))
    e = tak_amd.Engine(BOARD, res_blocks=BLOCKS, filters=FILTERS, policy_head=tak_amd.HEAD_CONV, evaluator=tak_amd.EVAL_RESNET,
                       max_batch=max_batch)
    e.load_state_dict(weights)
    return e


def _summary(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def worker_selfplay(a):
    e = _engine(a.tree, GAMES * a.batch)
    e.selfplay_create(GAMES, seed=0, rollouts=a.rollouts, max_examples=1 << 16, batch=a.batch)
    e.selfplay_step(1)
    e.sync()
    rates, per_iter = [], []
    for _ in range(a.reps):
        s0 = e.selfplay_stats()
        t0 = time.perf_counter()
        e.selfplay_step(a.plies)
        e.sync()
        dt = time.perf_counter() - t0
        s1 = e.selfplay_stats()
        rates.append((s1["expansions"] - s0["expansions"]) / dt)
        per_iter.append(1e3 * dt / (a.plies * (a.rollouts + 1)))
    e.close()
    print(json.dumps({"what": "selfplay", "batch": a.batch, "games": GAMES, "leaves_per_forward": GAMES * a.batch,
                      "rollouts": a.rollouts, "plies_per_window": a.plies, "windows": a.reps, "expansions_per_s": _summary(rates),
                      "ms_per_iteration": _summary(per_iter), "network": f"{BOARD}x{BOARD} {BLOCKS}x{FILTERS} conv"}), flush=True)


def worker_search(a):
    from oracle import oracle as orc

    batches = [int(b) for b in a.batches.split(",")]
    e = _engine(a.tree, GAMES * max(batches))
    sts = orc.random_positions(BOARD, GAMES * 3, seed=31, max_plies=40, half_komi=4)
    sts = sts[orc.result(BOARD, sts) == 0][:GAMES]
    for batch in batches:
        e.search_create(GAMES, arena_nodes=0, batch=batch, seed=2)
        per_iter = []
        for _ in range(a.reps + 1):  # the first window is the warm-up
            e.search_reset(sts)
            e.search_run(4)
            e.sync()
            t0 = time.perf_counter()
            e.search_run(a.iters)
            e.sync()
            per_iter.append(1e3 * (time.perf_counter() - t0) / a.iters)
        print(json.dumps({"what": "search", "tree": a.label, "batch": batch, "games": GAMES, "iters_per_window": a.iters,
                          "windows": a.reps, "ms_per_iteration": _summary(per_iter[1:]), "expansions": e.search_counters()[0]}), flush=True)
    e.close()


def child(args, limit, prefix=(), emit=True):
    """one measurement in a process of its own; its JSON lines are passed on.  Failure or overrun ends the sweep."""
    cmd = [*prefix, sys.executable, os.path.abspath(__file__), *args]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        sys.exit(f"{' '.join(args)}: no result within {limit} s; nothing further is started")
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        sys.exit(f"{' '.join(args)}: exit status {r.returncode}; nothing further is started")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    for ln in lines if emit else ():  # (a window timed under the profiler is no measurement of speed)
        print(ln, flush=True)
    return [json.loads(ln) for ln in lines]


def tree_share(trace_dir, batch):
    rows = []
    for p in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(p)))
    if not rows:
        sys.exit(f"no kernel_stats.csv under {trace_dir}")
    total = tree = 0.0
    names = {}
    for r in rows:
        ns = float(r["TotalDurationNs"]) if r.get("TotalDurationNs") else float(r["AverageNs"]) * float(r["Calls"])
        total += ns
        name = r["Name"].split("(")[0].split("<")[0].replace("void ", "").replace("tg::", "")
        if name.startswith(TREE_KERNELS):
            tree += ns
            names[name] = names.get(name, 0.0) + ns
    return {"what": "tree_share", "batch": batch, "tree_kernel_share": tree / total, "kernel_ms_total": total / 1e6,
            "tree_kernels_ms": {k: v / 1e6 for k, v in sorted(names.items())}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batches", default="1,4,8,16,32")
    ap.add_argument("--rollouts", type=int, default=40)
    ap.add_argument("--plies", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-tree")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--trace-dir")
    ap.add_argument("--limit", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--worker", choices=("selfplay", "search"))
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this")
    ap.add_argument("--batch", type=int, default=1)
    a = ap.parse_args()
    if a.worker == "selfplay":
        return worker_selfplay(a)
    if a.worker == "search":
        return worker_search(a)
    batches = [int(b) for b in a.batches.split(",")]
    common = ["--rollouts", str(a.rollouts), "--plies", str(a.plies)]
    for b in batches:
        child(["--worker", "selfplay", "--batch", str(b), "--reps", str(a.reps), *common], a.limit)
    if a.parent_tree:
        ab = ",".join(str(b) for b in (16, 32))
        for _ in range(a.rounds):  # alternating: other people's work shares the host
            for label, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                child(["--worker", "search", "--tree", tree, "--label", label, "--batches", ab, "--reps", str(a.reps), "--iters", str(a.iters)],
                      a.limit)
    if not a.no_profile:
        base = a.trace_dir or tempfile.mkdtemp(prefix="selfplay_batch_sweep_")
        for b in batches:
            d = os.path.join(base, f"batch{b}")
            os.makedirs(d, exist_ok=True)
            child(["--worker", "selfplay", "--batch", str(b), "--reps", "1", *common], a.limit,
                  prefix=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "kt", "--"), emit=False)
            print(json.dumps(tree_share(d, b)), flush=True)


if __name__ == "__main__":
    main()
