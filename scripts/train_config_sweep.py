#!/usr/bin/env python3
"""The training step on topologies the test suite does not name (no residual block, 256 filters, 3×3 and 4×4 boards):
tests/test_gpu_train.py's gradient gate — fp64 under the engine's ReLU decisions, 2e-5 per tensor — run as a sweep.  The ragged chunk
sizes and the chunks around the launchers' thresholds (33 … 257 examples on the 5×5 and 6×6 topologies) that used to be swept here are
part of the suite now: tests/test_gpu_train_brackets.py.  `python scripts/train_config_sweep.py`; prints one line per configuration,
exits 1 on a failure.  `--trained` runs the gate of tests/test_gpu_train_trained.py on the same topologies instead: a trained-like
network (test_gpu_train.trained_case), sharp targets, every tensor and every slice."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_train as T  # noqa: E402
from oracle import oracle as orc  # noqa: E402

CASES = [(5, 0, 64, "fc5", 16), (6, 0, 128, "conv", 8), (4, 2, 256, "conv", 12), (5, 1, 256, "fc5", 20), (3, 0, 32, "conv", 7),
         (4, 1, 128, "conv", 70)]
bad = 0
for cfg in CASES:
    try:
        if "--trained" in sys.argv[1:]:
            n, blocks, filters, head, count = cfg
            net, examples = T.trained_case(orc, n, blocks, filters, head, count, seed=None)
            T.chunk_gradients_against_fp64(orc, *cfg, net=net, examples=examples, slices=True)
        else:
            T.chunk_gradients_against_fp64(orc, *cfg)
        print("ok ", cfg, flush=True)
    except Exception as ex:  # noqa: BLE001
        bad += 1
        print("BAD", cfg, repr(ex)[:300], flush=True)
print("bad:", bad)
sys.exit(1 if bad else 0)
