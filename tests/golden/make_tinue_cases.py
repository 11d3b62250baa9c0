#!/usr/bin/env python3
"""Rebuilds tests/golden/tinue_positions.npz and tests/golden/tinue_cases.json from tests/tinue_ref.py: the positions and the
committed cases of the road-only forced-win solver (TG_SOLVE_ROAD_ONLY).

The positions are mined, because play-outs to a game's end give no deep road tactics: lock-step games on the oracle's rules from
new_game(n, half_komi=4); each ply a game plays, with probability 0.8, a uniformly chosen flat placement (move code < 64) when it
has one, otherwise a uniformly chosen legal move (numpy.random.default_rng(5), one generator per board size).  Of every game that
ends in a road the positions 2 to 6 plies before the end are kept (hist[-6:-1] of the positions a move was played from), in game
order.  All of them are solved road-only with the early stop, at depth 4 (5×5, GAMES5 games) and depth 3 (6×6, GAMES6 games); then

* "m5_400": every 5×5 position of value −4, 3 or −2, the first 200 of value 0, and positions of value 1 from the front until
  there are 400;
* "m6_200": every 6×6 position of value 3 or −2, the first 100 of value 0, and positions of value 1 until there are 200

go to tinue_positions.npz (numpy's stream is not a contract: the positions are committed, not only this recipe).  The cases, as in
make_solve_cases.py, are every position with |value| >= 3, the first 16 unproven, the first 16 proven at |value| <= 2 and the first
two of value −2 (on 6×6 the first 16 hold one) —
"five": selected by the depth-5 values of all of m5_400, answers at depth 4 and 5; "six": selected by the depth-4 values of all of
m6_200, answers at depth 4.  The class counts of every pass are recorded in the JSON.  If the depth-5 pass finds fewer than two
positions of value 5, raise GAMES5.

Under a minute on eight cores, 260 M reference positions (the positions are spread over the cores; the result does not depend on how).

    python tests/golden/make_tinue_cases.py
"""
import json
import multiprocessing
import os
import sys
import time

os.environ["OMP_NUM_THREADS"] = "1"  # (the oracle's own threads: here the positions are spread over processes instead)
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import tactics_ref as T  # noqa: E402
import tinue_ref as R  # noqa: E402
from oracle import oracle  # noqa: E402

GAMES5, GAMES6 = 400, 250
SEED, P_FLAT, HALF_KOMI = 5, 0.8, 4


def mine(n, games):
    """→ (positions [k, state bytes], games that ended in a road)"""
    rng = np.random.default_rng(SEED)
    cur = np.repeat(oracle.new_game(n, HALF_KOMI)[None, :], games, axis=0)
    hist = [[] for _ in range(games)]
    live = np.arange(games)
    ended = {}
    while len(live):
        moves, counts = oracle.movegen(n, cur[live])
        pick = np.zeros(len(live), np.uint16)
        for j, g in enumerate(live):
            mv = moves[j, : counts[j]]
            flats = mv[mv < 64]
            pool = flats if len(flats) and rng.random() < P_FLAT else mv
            pick[j] = pool[rng.integers(len(pool))]
            hist[g].append(cur[g].copy())
        nxt, status = oracle.play(n, cur[live], pick)
        assert not status.any()
        cur[live] = nxt
        res = oracle.result(n, nxt)
        for j, g in enumerate(live):
            if res[j]:
                ended[int(g)] = int(res[j])
        live = live[res == 0]
    roads = [g for g in range(games) if ended[g] in (1, 3)]
    keep = [s for g in roads for s in hist[g][-6:-1]]
    return np.stack(keep), len(roads)


_STATES = {}


def _one(job):
    name, i, depth = job
    ref = R.TinueRef(R.BOARD[name])
    value, best, moves, vals = ref.solve_one(_STATES[name][i], depth, False)
    return {"value": int(value), "best": int(best), "moves": [int(m) for m in moves], "move_values": vals, "nodes": ref.nodes}


def solve(pool, name, indices, depth):
    t = time.time()
    out = dict(zip(indices, pool.map(_one, [(name, i, depth) for i in indices], chunksize=1)))
    print(f"{name} depth {depth}: {len(indices)} positions, {sum(r['nodes'] for r in out.values())} reference positions, "
          f"{time.time() - t:.0f} s", flush=True)
    return out


def entry(r):
    return {"value": r["value"], "best": r["best"], "move_values": r["move_values"]}


def counts_of(results):
    return {str(k): n for k, n in sorted(T.class_counts([r["value"] for r in results]).items())}


def choose(values, deep, zeros, total):
    """rows of the mined set that are committed, in mined order"""
    v = np.asarray(values)
    rows = set(np.nonzero(np.isin(v, deep))[0].tolist()) | set(np.nonzero(v == 0)[0][:zeros].tolist())
    ones = np.nonzero(v == 1)[0]
    rows |= set(ones[: max(total - len(rows), 0)].tolist())
    return sorted(rows)


def select(values):
    k = len(values)
    deep = [i for i in range(k) if abs(values[i]) >= 3]
    unproven = [i for i in range(k) if values[i] == 0][:16]
    shallow = [i for i in range(k) if 0 < abs(values[i]) <= 2][:16] + [i for i in range(k) if values[i] == -2][:2]
    return sorted(set(deep + unproven + shallow))


def main():
    ctx = multiprocessing.get_context("fork")
    workers = min(8, os.cpu_count() or 1)
    _STATES["mined5"], roads5 = mine(5, GAMES5)
    _STATES["mined6"], roads6 = mine(6, GAMES6)
    R.BOARD.update(mined5=5, mined6=6, m5_400=5, m6_200=6)
    with ctx.Pool(workers) as pool:  # (forked after the mining: the workers share the positions)
        a5 = solve(pool, "mined5", list(range(len(_STATES["mined5"]))), 4)
        a6 = solve(pool, "mined6", list(range(len(_STATES["mined6"]))), 3)
    rows5 = choose([a5[i]["value"] for i in range(len(a5))], (-4, 3, -2), 200, 400)
    rows6 = choose([a6[i]["value"] for i in range(len(a6))], (3, -2), 100, 200)
    _STATES["m5_400"], _STATES["m6_200"] = _STATES["mined5"][rows5], _STATES["mined6"][rows6]
    np.savez_compressed(os.path.join(HERE, "tinue_positions.npz"), m5_400=_STATES["m5_400"], m6_200=_STATES["m6_200"])
    with ctx.Pool(workers) as pool:
        d5 = solve(pool, "m5_400", list(range(len(rows5))), 5)
        idx5 = select([d5[i]["value"] for i in range(len(rows5))])
        d4 = solve(pool, "m5_400", idx5, 4)
        s4 = solve(pool, "m6_200", list(range(len(rows6))), 4)
        idx6 = select([s4[i]["value"] for i in range(len(rows6))])
    five = [{"index": i, "counts": len(d5[i]["moves"]), "moves": d5[i]["moves"], "depth4": entry(d4[i]), "depth5": entry(d5[i])} for i in idx5]
    six = [{"index": i, "counts": len(s4[i]["moves"]), "moves": s4[i]["moves"], "depth4": entry(s4[i])} for i in idx6]
    doc = {"road_only": True, "all_moves": False,
           "generator": {"seed": SEED, "p_flat": P_FLAT, "half_komi": HALF_KOMI, "kept": "hist[-6:-1] of every game that ends in a road"},
           "five": {"set": "m5_400", "games": GAMES5, "road_games": roads5, "mined": len(a5),
                    "value_counts_depth4_mined": counts_of(a5.values()),
                    "value_counts_depth4_committed": counts_of([a5[i] for i in rows5]),
                    "value_counts_depth5_committed": counts_of(d5.values()), "cases": five},
           "six": {"set": "m6_200", "games": GAMES6, "road_games": roads6, "mined": len(a6),
                   "value_counts_depth3_mined": counts_of(a6.values()),
                   "value_counts_depth3_committed": counts_of([a6[i] for i in rows6]),
                   "value_counts_depth4_committed": counts_of(s4.values()), "cases": six}}
    with open(os.path.join(HERE, "tinue_cases.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
        f.write("\n")
    for b in ("five", "six"):
        print(b, {k: v for k, v in doc[b].items() if k != "cases"}, len(doc[b]["cases"]), "cases")
    fives = doc["five"]["value_counts_depth5_committed"].get("5", 0)
    print(f"5x5 positions of value 5: {fives}" + ("" if fives >= 2 else " — fewer than two: raise GAMES5"))


if __name__ == "__main__":
    main()
