"""bench.py --dump-outputs: what the last timed ply left, as .npy files in float32 / float64 within a fixed budget, the same
from run to run; and a plain run (no --full) that measures the headline alone."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

MAX_MOVES = 512


class FakeEngine:
    """the four calls dump_outputs makes, with the engine's shapes and dtypes (tak_amd/engine.py)"""

    def __init__(self, games, examples, sb=96, seed=0):
        from tak_amd.engine import EXAMPLE_HEADER

        rng = np.random.default_rng(seed)
        self.games, self.sb = games, sb
        self.counts = rng.integers(1, 120, games).astype(np.int32)
        self.root = dict(moves=rng.integers(0, 1 << 16, (games, MAX_MOVES)).astype(np.uint16),
                         visits=rng.integers(0, 400, (games, MAX_MOVES)).astype(np.uint32),
                         prior=rng.random((games, MAX_MOVES), np.float32), q=rng.random((games, MAX_MOVES), np.float32),
                         counts=self.counts, root_visits=rng.integers(0, 401, games).astype(np.uint32),
                         root_q=rng.random(games, np.float32))
        self.states = rng.integers(0, 256, (games, sb)).astype(np.uint8)
        self.hdr = np.zeros(examples, EXAMPLE_HEADER)
        self.hdr["game_id"] = rng.integers(0, 1 << 20, examples)
        self.hdr["n_moves"] = rng.integers(1, 90, examples)
        self.hdr["result"] = rng.choice([-1.0, 0.0, 1.0], examples)
        self.ex_states = rng.integers(0, 256, (examples, sb)).astype(np.uint8)
        self.ex_moves = rng.integers(0, 1 << 16, (examples, MAX_MOVES)).astype(np.uint16)
        self.ex_visits = rng.integers(0, 400, (examples, MAX_MOVES)).astype(np.uint32)
        self.stats = {"games_finished": 3, "examples": examples, "expansions": 123456789, "evals": 1000}

    def selfplay_stats(self):
        return dict(self.stats)

    def search_root(self):
        return {k: v.copy() for k, v in self.root.items()}

    def search_states(self):
        return self.states.copy()

    def selfplay_drain(self, cap=4096):
        k = min(cap, len(self.hdr))
        return self.hdr[:k].copy(), self.ex_states[:k].copy(), self.ex_moves[:k].copy(), self.ex_visits[:k].copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_writes_the_engine_results_exactly(tmp_path):
    eng = FakeEngine(games=64, examples=50)
    bench.dump_outputs(eng, str(tmp_path))
    got = _load(str(tmp_path))
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    k = int(eng.counts.max())
    assert np.array_equal(got["root_states"], eng.states.astype(np.float32))
    assert np.array_equal(got["root_moves"], eng.root["moves"][:, :k].astype(np.float32))
    assert np.array_equal(got["root_child_visits"], eng.root["visits"][:, :k].astype(np.float64))
    assert np.array_equal(got["root_prior"], eng.root["prior"][:, :k]) and np.array_equal(got["root_q"], eng.root["q"][:, :k])
    assert np.array_equal(got["root_visits"], eng.root["root_visits"]) and np.array_equal(got["root_value"], eng.root["root_q"])
    k = int(eng.hdr["n_moves"].max())
    assert np.array_equal(got["example_game_id"], eng.hdr["game_id"]) and np.array_equal(got["example_result"], eng.hdr["result"])
    assert np.array_equal(got["example_states"], eng.ex_states.astype(np.float32))
    assert np.array_equal(got["example_moves"], eng.ex_moves[:, :k].astype(np.float32))
    assert np.array_equal(got["example_visits"], eng.ex_visits[:, :k].astype(np.float64))
    assert got["stat_expansions"][0] == 123456789  # float64: exact beyond 2^24
    assert "root_rows" not in got and "example_rows" not in got


def test_dump_over_budget_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 1 << 20)
    eng = FakeEngine(games=2048, examples=3000)
    for d in ("a", "b"):
        bench.dump_outputs(eng, str(tmp_path / d))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a.keys() == b.keys() and all(np.array_equal(a[n], b[n]) for n in a)
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= 1 << 20
    for group, n in (("root", 2048), ("example", 3000)):
        rows = a[group + "_rows"].astype(np.int64)
        assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[-1] < n
    rows = a["root_rows"].astype(np.int64)
    assert np.array_equal(a["root_states"], eng.states[rows].astype(np.float32))
    assert len(a["root_prior"]) == len(rows)


def test_dump_per_rank_names(tmp_path):
    bench.dump_outputs(FakeEngine(games=8, examples=0), str(tmp_path), rank=1, world=2)
    names = os.listdir(tmp_path)
    assert names and all(n.startswith("rank1_") for n in names)
    assert np.load(os.path.join(tmp_path, "rank1_example_states.npy")).shape[0] == 0


SMALL = ["--games", "64", "--rollouts", "16", "--blocks", "2", "--filters", "64", "--arena", "4096"]


@pytest.mark.gpu
def test_plain_run_times_the_headline_and_dumps_the_same_outputs_twice(tmp_path):
    runs = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *SMALL,
               "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-3000:]
        lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
        assert len(lines) == 1
        runs.append(json.loads(lines[0]))
    out = runs[0]
    assert out["steps"] == 3 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["config"]["expansions_timed"] == 3 * 64 * 17  # three timed plies: (1 root evaluation + 16 rollouts) per game
    for part in ("cpu_baseline", "alt_precision", "extra"):
        assert part not in out, part  # --full only
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert a.keys() == b.keys() and {"root_states", "root_prior", "root_child_visits", "stat_expansions"} <= a.keys()
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    assert a["root_states"].shape[0] == 64
