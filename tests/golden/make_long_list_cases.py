#!/usr/bin/env python3
"""Writes tests/golden/long_list_depth4.json: the depth-4 answers of tests/tactics_ref.py (early stop, both modes) on three roots of
posgen.long_list_states — R (→ S), R_mirror (the control) and R_W (an instant road among the first 512 moves) — with the give-up rule
of include/takgpu.h.  About two minutes per mode on one core, which is why tests/test_gpu_long_move_lists.py reads the answers from
the file; tests/test_long_move_lists.py recomputes nothing of it but checks that the file belongs to the committed positions.

    python tests/golden/make_long_list_cases.py [--exact]

--exact adds, for R alone, the answer on whole lists (no capacity) in the default mode: the soundness yardstick.  It takes much
longer (every one of S's 763 moves is walked two plies deep)."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import posgen  # noqa: E402
import tactics_ref as T  # noqa: E402
import tinue_ref as R  # noqa: E402
from oracle import oracle  # noqa: E402

NAMES = ("R", "R_mirror", "R_W")
DEPTH = 4
OUT = os.path.join(HERE, "long_list_depth4.json")


def rows(out):
    return [dict(value=int(out["value"][i]), best=int(out["best"][i]), counts=int(out["counts"][i]), budget_hit=int(out["budget_hit"][i]),
                 moves=[int(x) for x in out["moves"][i, : out["counts"][i]]],
                 move_values=[int(x) for x in out["move_values"][i, : out["counts"][i]]]) for i in range(len(out["value"]))]


def main():
    fam = posgen.long_list_states(oracle, 6)
    roots = np.stack([fam["roots"][k][0] for k in NAMES])
    doc = dict(board=6, depth=DEPTH, names=list(NAMES), sha256=hashlib.sha256(roots.tobytes()).hexdigest())
    if os.path.exists(OUT):
        with open(OUT) as f:
            old = json.load(f)
        if old.get("sha256") == doc["sha256"] and "exact_R" in old:
            doc["exact_R"] = old["exact_R"]
    doc["default"] = rows(T.Ref(6).solve(roots, DEPTH, False))
    doc["road_only"] = rows(R.TinueRef(6).solve(roots, DEPTH, False))
    if "--exact" in sys.argv:
        doc["exact_R"] = rows(T.Ref(6, capacity=None).solve(roots[:1], DEPTH, False))[0]
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
