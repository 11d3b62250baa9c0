#!/usr/bin/env python3
"""What the dihedral symmetries cost, at config C2 (5x5, 6 x 64, FC head, 4096 games, 400 rollouts per move), measured as
scripts/selfplay_schedule_sweep.py measures: warm plies, then timed plies, every run in a child process of its own, the arms
alternating for `--rounds` rounds because other people's work shares the host.

    python scripts/bench_symm.py --parent-tree DIR [--warm 120] [--plies 20] [--rounds 2] [--out profiles/<name>.json]

    parent   self-play on the parent commit's library (--parent-tree: a BUILT tree of that commit)
    off      this build, TG_SYMM_OFF (the default: nothing is launched)
    hashed   this build, TG_SYMM_HASHED: k_symm_leaves in front of every forward
    eval     tg_policy_eval_symm_dev at mask 0xFF on 512 states against tg_policy_eval_dev on 4096 states: the same 4096-row
             forward with and without the image and fold kernels around it (a host clock around `--reps` calls and one synchronise)
The summary holds
    off_vs_parent     the two medians and the parent's own spread between its runs of this job ((max - min) / median): the margin
                      within which `off` has to agree with `parent`, and whether it does
    hashed_vs_off     ms per ply of both, and the difference per search iteration (a ply runs rollouts + 1 of them) in µs: what
                      k_symm_leaves and the mapped gather cost where they run — reported, not gated
    fold_overhead     µs per call of both `eval` calls and their difference
A child that fails or overruns its time limit ends the job: nothing further is started, and --out still gets the runs so far,
their count per arm in the summary, `complete: false` and the reason under `ended`. The file's `command` is the one that was run,
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
    e.selfplay_create(a.games, seed=0, rollouts=a.rollouts, max_examples=1 << 14, **(dict(symmetry="hashed") if a.arm == "hashed" else {}))
    e.selfplay_step(a.warm)
    e.sync()
    s0 = e.selfplay_stats()
    t0 = time.perf_counter()
    e.selfplay_step(a.plies)
    e.sync()
    dt = time.perf_counter() - t0
    s1 = e.selfplay_stats()
    out = {"what": "run", "arm": a.arm, "games": a.games, "rollouts": a.rollouts, "warm_plies": a.warm, "plies": a.plies, "seconds": dt,
           "expansions": s1["expansions"] - s0["expansions"], "expansions_per_s": (s1["expansions"] - s0["expansions"]) / dt,
           "ms_per_ply": 1e3 * dt / a.plies, "aborted_games": s1["aborted_games"]}
    if a.arm == "hashed":
        out["leaves_transformed"] = e.search_get_symmetry()[1]
        out["evals"] = s1["evals"] if "evals" in s1 else None
    e.close()
    print(json.dumps(out), flush=True)


def eval_worker(a):
    import numpy as np
    import torch

    e = _engine(a.tree, 4096)  # (puts the tree on the path)
    from oracle import oracle as orc

    sts = orc.random_positions(BOARD, 3 * 4096, seed=1, max_plies=60, half_komi=4)
    sts = sts[orc.result(BOARD, sts) == 0][:4096]
    assert len(sts) == 4096
    d_states = torch.from_numpy(np.ascontiguousarray(sts)).cuda()
    d_policy = torch.zeros((4096, e.psize), dtype=torch.float32, device="cuda")
    d_eval = torch.zeros(4096, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    calls = {"policy_eval_dev_4096": lambda: e.policy_eval_dev(4096, d_states.data_ptr(), d_policy.data_ptr(), d_eval.data_ptr()),
             "policy_eval_symm_dev_512x8": lambda: e.policy_eval_symm_dev(512, d_states.data_ptr(), 0xFF, d_policy.data_ptr(), d_eval.data_ptr())}
    out = {"what": "run", "arm": "eval", "reps": a.reps}
    for _ in range(2):  # the second pass is the one kept: both calls warm
        for name, call in calls.items():
            for _ in range(10):
                call()
            e.sync()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                call()
            e.sync()
            out[name + "_us"] = 1e6 * (time.perf_counter() - t0) / a.reps
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


def summarise(runs, rollouts):
    by = {arm: [r for r in runs if r["arm"] == arm] for arm in ("parent", "off", "hashed", "eval")}
    med = {arm: statistics.median(r["ms_per_ply"] for r in by[arm]) for arm in ("parent", "off", "hashed") if by[arm]}
    out = {"what": "summary", "ms_per_ply_median": med, "runs_per_arm": {arm: len(rs) for arm, rs in by.items()}}
    if by["parent"] and by["off"]:
        p = [r["ms_per_ply"] for r in by["parent"]]
        margin = (max(p) - min(p)) / med["parent"]
        diff = (med["off"] - med["parent"]) / med["parent"]
        out["off_vs_parent"] = {"parent_spread": margin, "off_minus_parent": diff, "within_the_parents_spread": abs(diff) <= margin, "parent_runs": len(p)}
    if by["hashed"] and by["off"]:
        extra = med["hashed"] - med["off"]
        out["hashed_vs_off"] = {"ms_per_ply_off": med["off"], "ms_per_ply_hashed": med["hashed"], "extra_ms_per_ply": extra,
                                "extra_us_per_iteration": 1e3 * extra / (rollouts + 1), "iterations_per_ply": rollouts + 1}
    if by["eval"]:
        a = statistics.median(r["policy_eval_dev_4096_us"] for r in by["eval"])
        b = statistics.median(r["policy_eval_symm_dev_512x8_us"] for r in by["eval"])
        out["fold_overhead"] = {"policy_eval_dev_4096_us": a, "policy_eval_symm_dev_512x8_us": b, "extra_us": b - a, "extra_share": (b - a) / a}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-tree", help="a built tree of the parent commit (tak_amd/libtakgpu.so, tests/torch_ref.py); without it the parent arm is left out")
    ap.add_argument("--games", type=int, default=GAMES)
    ap.add_argument("--rollouts", type=int, default=ROLLOUTS)
    ap.add_argument("--warm", type=int, default=120, help="plies played before the timed ones")
    ap.add_argument("--plies", type=int, default=20, help="timed plies per run")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50, help="calls per timing of the eval arm")
    ap.add_argument("--limit", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--out", help="also write the runs and the summary to this file")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--arm", choices=("parent", "off", "hashed", "eval"), default="off")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    if a.worker:
        return eval_worker(a) if a.arm == "eval" else worker(a)
    arms = ([("parent", os.path.abspath(a.parent_tree))] if a.parent_tree else []) + [("off", ROOT), ("hashed", ROOT), ("eval", ROOT)]
    common = ["--games", str(a.games), "--rollouts", str(a.rollouts), "--warm", str(a.warm), "--plies", str(a.plies), "--reps", str(a.reps)]
    command = "scripts/bench_symm.py " + " ".join((["--parent-tree", "PARENT"] if a.parent_tree else []) + common + ["--rounds", str(a.rounds)])
    runs, ended = [], None
    try:
        for _ in range(a.rounds):
            for arm, tree in arms:
                runs.append(child(arm, ["--worker", "--arm", arm, "--tree", tree, *common], a.limit))
    except ChildFailed as err:
        ended = f"{err}; nothing further was started"
    summary = summarise(runs, a.rollouts)
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
