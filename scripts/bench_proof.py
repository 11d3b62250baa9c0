#!/usr/bin/env python3
"""What proven values in the tree cost or save, at config C2 (5x5, 6 x 64, FC head, 4096 games, 400 rollouts per move), measured
as scripts/bench_symm.py measures: warm plies, then timed plies, every run in a child process of its own, the arms alternating
for `--rounds` rounds because other people's work shares the host.

    python scripts/bench_proof.py --parent-tree DIR [--warm 120] [--plies 20] [--rounds 2] [--out profiles/<name>.json]

    parent   self-play on the parent commit's library (--parent-tree: a BUILT tree of that commit)
    off      this build, TG_PROOF_OFF (the default: the parent's kernels)
    on       this build, TG_PROOF_ON: the PROOF instantiations of the tree kernels (tree_kernels.hip) and of the pick
The summary holds
    off_vs_parent   the two medians and the parent's own spread between its runs of this job ((max - min) / median): the margin
                    within which `off` has to agree with `parent`, and whether it does
    on_vs_off       ms per ply of both and their difference; over the timed plies of the `on` runs the nodes proven and the
                    share of rollouts that ended on a proven node — first figures, reported, not gated.  The two arms do not
                    play the same games from the first proven root on, so the difference is between two self-play runs, not
                    between two ways to do the same work
A child that fails or overruns its time limit ends the job: nothing further is started, and --out still gets the runs so far,
their count per arm in the summary, `complete: false` and the reason under `ended`.  The file's `command` is the one that was run,
with PARENT standing for the parent tree's path."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOARD, BLOCKS, FILTERS, GAMES, ROLLOUTS = 5, 6, 64, 4096, 400
ARMS = ("parent", "off", "on")


def _engine(tree, max_batch):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))
    import torch_ref

    import tak_amd

    assert os.path.dirname(os.path.abspath(tak_amd.__file__)) == os.path.join(os.path.abspath(tree), "tak_amd"), tak_amd.__file__
    e = tak_amd.Engine(BOARD, res_blocks=BLOCKS, filters=FILTERS, policy_head=tak_amd.HEAD_FC5, evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch)
    e.load_state_dict(torch_ref.abi_tensors(torch_ref.make_net(BOARD, BLOCKS, FILTERS, "fc5", seed=0, randomize_bn=False)))
    return e


def worker(a):
    e = _engine(a.tree, a.games)
    e.selfplay_create(a.games, seed=0, rollouts=a.rollouts, max_examples=1 << 14, **(dict(proof="on") if a.arm == "on" else {}))
    e.selfplay_step(a.warm)
    e.sync()
    s0 = e.selfplay_stats()
    p0 = e.search_get_proof() if a.arm == "on" else None
    t0 = time.perf_counter()
    e.selfplay_step(a.plies)
    e.sync()
    dt = time.perf_counter() - t0
    s1 = e.selfplay_stats()
    rollouts = s1["expansions"] - s0["expansions"]
    out = {"what": "run", "arm": a.arm, "games": a.games, "rollouts": a.rollouts, "warm_plies": a.warm, "plies": a.plies, "seconds": dt,
           "expansions": rollouts, "expansions_per_s": rollouts / dt, "evals": s1["evals"] - s0["evals"],
           "ms_per_ply": 1e3 * dt / a.plies, "aborted_games": s1["aborted_games"], "games_finished": s1["games_finished"] - s0["games_finished"]}
    if a.arm == "on":
        p1 = e.search_get_proof()
        out["nodes_proven"] = p1[1] - p0[1]
        out["rollouts_ended_on_proven"] = p1[2] - p0[2]
        out["share_ended_on_proven"] = (p1[2] - p0[2]) / rollouts if rollouts else None
        out["nodes_proven_in_the_warm_plies"] = p0[1]
    e.close()
    print(json.dumps(out), flush=True)


class ChildFailed(Exception):
    pass


def child(arm, args, limit):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise ChildFailed(f"arm {arm}: no result within {limit} s")
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise ChildFailed(f"arm {arm}: exit status {r.returncode}")
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if not lines:
        raise ChildFailed(f"arm {arm}: no result line")
    print(lines[-1], flush=True)
    return json.loads(lines[-1])


def summarise(runs):
    by = {arm: [r for r in runs if r["arm"] == arm] for arm in ARMS}
    med = {arm: statistics.median(r["ms_per_ply"] for r in by[arm]) for arm in ARMS if by[arm]}
    out = {"what": "summary", "ms_per_ply_median": med, "runs_per_arm": {arm: len(rs) for arm, rs in by.items()}}
    if by["parent"] and by["off"]:
        p = [r["ms_per_ply"] for r in by["parent"]]
        margin = (max(p) - min(p)) / med["parent"]
        diff = (med["off"] - med["parent"]) / med["parent"]
        out["off_vs_parent"] = {"parent_spread": margin, "off_minus_parent": diff, "within_the_parents_spread": abs(diff) <= margin, "parent_runs": len(p)}
    if by["on"] and by["off"]:
        out["on_vs_off"] = {"ms_per_ply_off": med["off"], "ms_per_ply_on": med["on"], "on_minus_off_ms_per_ply": med["on"] - med["off"],
                            "on_minus_off_share": (med["on"] - med["off"]) / med["off"],
                            "evals_per_ply_off": statistics.median(r["evals"] / r["plies"] for r in by["off"]),
                            "evals_per_ply_on": statistics.median(r["evals"] / r["plies"] for r in by["on"]),
                            "nodes_proven_per_ply": statistics.median(r["nodes_proven"] / r["plies"] for r in by["on"]),
                            "share_of_rollouts_ended_on_proven": statistics.median(r["share_ended_on_proven"] for r in by["on"])}
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
    ap.add_argument("--arm", choices=ARMS, default="off")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    arms = ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [("off", ROOT), ("on", ROOT)]
    common = ["--games", str(a.games), "--rollouts", str(a.rollouts), "--warm", str(a.warm), "--plies", str(a.plies)]
    command = "scripts/bench_proof.py " + " ".join((["--parent-tree", "PARENT"] if a.parent_tree else []) + common + ["--rounds", str(a.rounds)])
    runs, ended = [], None
    try:
        for _ in range(a.rounds):
            for arm, tree in arms:
                runs.append(child(arm, ["--worker", "--arm", arm, "--tree", tree, *common], a.limit))
    except ChildFailed as err:
        ended = f"{err}; nothing further was started"
    summary = summarise(runs)
    print(json.dumps(summary), flush=True)
    if a.out:  # also after an early end: the runs so far, their counts per arm in the summary, and why the job ended
        with open(a.out, "w") as f:
            json.dump({"command": command, "config": f"{BOARD}x{BOARD} {BLOCKS}x{FILTERS} fc5", "arms": [arm for arm, _ in arms],
                       "rounds_asked": a.rounds, "complete": ended is None, "ended": ended, "runs": runs, "summary": summary}, f, indent=1)
            f.write("\n")
    if ended:
        sys.exit(ended)


if __name__ == "__main__":
    main()
