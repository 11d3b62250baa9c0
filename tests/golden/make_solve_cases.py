#!/usr/bin/env python3
"""Rebuilds tests/golden/solve_cases.json from tests/tactics_ref.py: the depth-4 and depth-5 cases of the forced-win solver.

The positions are indices into tactics_ref.positions("p5_160") (oracle.playouts(5, 160, 7)["prev"]).  The list covers every
position whose depth-5 value has |value| >= 3, plus the first 16 unproven positions and the first 16 proven at |value| <= 2.
Expected outputs are the reference's at depth 4 and at depth 5, levels stopping at the deciding one (no TG_SOLVE_ALL_MOVES).
Half a minute of CPU and 14 M positions, which is why the result is committed and tests/test_tactics_ref.py recomputes only a sample.

    python tests/golden/make_solve_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import tactics_ref as T  # noqa: E402


def main():
    states = T.positions("p5_160")
    ref = T.Ref(5)
    d5 = ref.solve(states, 5, False)
    v = d5["value"].astype(int)
    deep = [i for i in range(len(v)) if abs(v[i]) >= 3]
    unproven = [i for i in range(len(v)) if v[i] == 0][:16]
    shallow = [i for i in range(len(v)) if 0 < abs(v[i]) <= 2][:16]
    idx = sorted(set(deep + unproven + shallow))
    d4 = T.Ref(5).solve(states[idx], 4, False)
    cases = []
    for j, i in enumerate(idx):
        c = int(d5["counts"][i])
        cases.append({"index": i, "counts": c, "moves": d5["moves"][i, :c].tolist(),
                      "depth4": {"value": int(d4["value"][j]), "best": int(d4["best"][j]), "move_values": d4["move_values"][j, :c].tolist()},
                      "depth5": {"value": int(v[i]), "best": int(d5["best"][i]), "move_values": d5["move_values"][i, :c].tolist()}})
    doc = {"set": "p5_160", "source": "oracle.playouts(5, 160, 7)['prev']", "all_moves": False,
           "value_counts_depth5_all_160": {str(k): n for k, n in sorted(T.class_counts(v).items())}, "cases": cases}
    with open(os.path.join(HERE, "solve_cases.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases; depth-5 values of the 160: {doc['value_counts_depth5_all_160']}; reference nodes {ref.nodes}")


if __name__ == "__main__":
    main()
