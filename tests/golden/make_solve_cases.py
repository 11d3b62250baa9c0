#!/usr/bin/env python3
"""Rebuilds tests/golden/solve_cases.json from tests/tactics_ref.py: the depth-4, depth-5 and depth-6 cases of the forced-win solver.
Expected outputs are the reference's, levels stopping at the deciding one (no TG_SOLVE_ALL_MOVES).  Three blocks:

* the top level ("set": "p5_160", oracle.playouts(5, 160, 7)["prev"]): every position whose depth-5 value has |value| >= 3, plus
  the first 16 unproven positions and the first 16 proven at |value| <= 2, at depth 4, 5 and 6.  (Not all 44 unproven positions
  of the set: their depth-6 reference runs for more than eight minutes.)
* "tall_stacks" ("set": "s5_200", the first 100): the positions unproven at depth 5, at depth 5 and 6.
* "six" ("set": "p6_80"): every position with |value| >= 3 at depth 5, the first 8 unproven, the first 8 proven at
  |value| <= 2 and the first 2 of value -2 (the first 8 are all +1), at depth 5; at depth 6 the deep ones (the early stop makes it the same table) and the unproven positions of the
  80 whose depth-5 reference created the fewest positions (SIX_DEPTH6 of them, below SIX_DEPTH6_NODES each: depth 6 on a
  6×6 position that is not proven costs up to eighty times its depth 5; none of the six came out at −6).

About two minutes on eight cores, 230 M reference positions (the positions are spread over the cores; the result does not depend
on how), which is why the result is committed and tests/test_tactics_ref.py recomputes only a sample.

    python tests/golden/make_solve_cases.py
"""
import json
import multiprocessing
import os
import sys

os.environ["OMP_NUM_THREADS"] = "1"  # (the oracle's own threads: here the positions are spread over processes instead)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import tactics_ref as T  # noqa: E402

SIX_DEPTH6 = 6
SIX_DEPTH6_NODES = 500_000  # depth-5 reference positions of a 6×6 position that is taken to depth 6


def _one(job):
    name, i, depth = job
    ref = T.Ref(T.BOARD[name])
    value, best, moves, vals = ref.solve_one(T.positions(name)[i], depth, False)
    return {"value": int(value), "best": int(best), "moves": [int(m) for m in moves], "move_values": vals, "nodes": ref.nodes}


def solve(pool, name, indices, depth):
    """→ {index: the reference's answer at `depth`, early stop}, one position per task"""
    return dict(zip(indices, pool.map(_one, [(name, i, depth) for i in indices], chunksize=1)))


def entry(r):
    return {"value": r["value"], "best": r["best"], "move_values": r["move_values"]}


def counts_of(results):
    return {str(k): n for k, n in sorted(T.class_counts([r["value"] for r in results]).items())}


def main():
    for name in ("p5_160", "s5_200", "p6_80"):
        T.positions(name)  # (before the fork: the workers share them)
    nodes = {}
    with multiprocessing.get_context("fork").Pool(min(8, os.cpu_count() or 1)) as pool:
        # ---- 5×5 play-outs: the selection of the first version of this file, now to depth 6
        d5 = solve(pool, "p5_160", list(range(160)), 5)
        v = [d5[i]["value"] for i in range(160)]
        deep = [i for i in range(160) if abs(v[i]) >= 3]
        unproven = [i for i in range(160) if v[i] == 0][:16]
        shallow = [i for i in range(160) if 0 < abs(v[i]) <= 2][:16]
        idx = sorted(set(deep + unproven + shallow))
        d4, d6 = solve(pool, "p5_160", idx, 4), solve(pool, "p5_160", idx, 6)
        nodes["p5_160"] = {"depth4": sum(r["nodes"] for r in d4.values()), "depth5": sum(r["nodes"] for r in d5.values()),
                           "depth6": sum(r["nodes"] for r in d6.values())}
        cases = [{"index": i, "counts": len(d5[i]["moves"]), "moves": d5[i]["moves"], "depth4": entry(d4[i]), "depth5": entry(d5[i]),
                  "depth6": entry(d6[i])} for i in idx]
        # ---- 5×5 tall stacks: what depth 5 leaves open
        s5 = solve(pool, "s5_200", list(range(100)), 5)
        s_idx = [i for i in range(100) if s5[i]["value"] == 0]
        s6 = solve(pool, "s5_200", s_idx, 6)
        nodes["s5_200"] = {"depth5": sum(r["nodes"] for r in s5.values()), "depth6": sum(r["nodes"] for r in s6.values())}
        tall = [{"index": i, "counts": len(s5[i]["moves"]), "moves": s5[i]["moves"], "depth5": entry(s5[i]), "depth6": entry(s6[i])}
                for i in s_idx]
        # ---- 6×6
        p6 = solve(pool, "p6_80", list(range(80)), 5)
        w = [p6[i]["value"] for i in range(80)]
        deep6 = [i for i in range(80) if abs(w[i]) >= 3]
        open6 = [i for i in range(80) if w[i] == 0]
        light = [i for i in sorted(open6, key=lambda i: (p6[i]["nodes"], i)) if p6[i]["nodes"] <= SIX_DEPTH6_NODES][:SIX_DEPTH6]
        shallow6 = [i for i in range(80) if 0 < abs(w[i]) <= 2][:8] + [i for i in range(80) if w[i] == -2][:2]
        idx6 = sorted(set(deep6 + open6[:8] + shallow6 + light))
        p66 = solve(pool, "p6_80", sorted(set(deep6 + light)), 6)
        nodes["p6_80"] = {"depth5": sum(r["nodes"] for r in p6.values()), "depth6": sum(r["nodes"] for r in p66.values())}
        six = []
        for i in idx6:
            c = {"index": i, "counts": len(p6[i]["moves"]), "moves": p6[i]["moves"], "depth5": entry(p6[i])}
            if i in p66:
                c["depth6"] = entry(p66[i])
            six.append(c)
    doc = {"set": "p5_160", "source": "oracle.playouts(5, 160, 7)['prev']", "all_moves": False,
           "value_counts_depth5_all_160": counts_of(d5.values()), "cases": cases,
           "tall_stacks": {"set": "s5_200", "source": "oracle.playouts(5, 200, 11, style=3)['prev'][:100]",
                           "value_counts_depth5_first_100": counts_of(s5.values()), "cases": tall},
           "six": {"set": "p6_80", "source": "oracle.playouts(6, 80, 7)['prev']", "value_counts_depth5_all_80": counts_of(p6.values()),
                   "depth6_unproven": light, "cases": six}}
    with open(os.path.join(HERE, "solve_cases.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"p5_160: {len(cases)} cases; depth-5 values of the 160: {doc['value_counts_depth5_all_160']}; depth-6 values of the cases: "
          f"{counts_of(d6.values())}; reference nodes {nodes['p5_160']}")
    print(f"s5_200[:100]: {len(tall)} cases unproven at depth 5 of {doc['tall_stacks']['value_counts_depth5_first_100']}; depth-6 values: "
          f"{counts_of(s6.values())}, -6 at {[i for i in s_idx if s6[i]['value'] == -6]}; reference nodes {nodes['s5_200']}")
    print(f"p6_80: {len(six)} cases; depth-5 values of the 80: {doc['six']['value_counts_depth5_all_80']}; depth 6 on {sorted(p66)} "
          f"(unproven at depth 5: {light}, their depth-5 nodes {[p6[i]['nodes'] for i in light]}), values {counts_of(p66.values())}; "
          f"reference nodes {nodes['p6_80']}")
    found = [i for i in light if p66[i]["value"] == -6]
    print(f"6x6 positions of value -6: {found if found else 'none found'}")


if __name__ == "__main__":
    main()
