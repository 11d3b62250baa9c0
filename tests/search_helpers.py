"""What the GPU search and self-play tests share: engines and root positions, tree and example comparisons, and the replay of
the self-play driver on `oracle.Search`.  A plain module, like torch_ref.py and posgen.py."""
import functools
import os

import numpy as np

import torch_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WHITE_ROAD, WHITE_FLAT, BLACK_ROAD, BLACK_FLAT = 1, 2, 3, 4


def _mk(n, evaluator, games, head=None, **kw):
    import tak_amd

    if head is None:
        head = tak_amd.HEAD_FC5 if n == 5 else tak_amd.HEAD_CONV
    return tak_amd.Engine(n, evaluator=evaluator, max_batch=max(games, 64), policy_head=head, **kw)


def _roots(orc, n, count, seed, max_plies):
    sts = orc.random_positions(n, count * 3, seed=seed, max_plies=max_plies, half_komi=4)
    sts = sts[orc.result(n, sts) == 0][:count]
    assert len(sts) == count
    return sts


def _assert_same_trees(e, s, games):
    for g in range(games):
        a, b = e.search_dump(g), s.dump(g)
        assert len(a) == len(b), (g, len(a), len(b))
        for f in a.dtype.names:
            assert np.array_equal(a[f], b[f]), (g, f)


def _best(root, g):
    c = root["counts"][g]
    v = root["visits"][g, :c]
    return root["moves"][g, c - 1 - int(np.argmax(v[::-1]))]


@functools.lru_cache(maxsize=None)
def _golden_net(stem):
    """(n, blocks, filters, head, tensors) of tests/golden/<stem>.npz: the fixture holds the seed, torch_ref regenerates the weights"""
    n, blocks, filters, head_i, seed = [int(v) for v in np.load(os.path.join(GOLDEN, stem + ".npz"))["meta"]]
    head = "fc5" if head_i == 0 else "conv"
    return n, blocks, filters, head, torch_ref.abi_tensors(torch_ref.make_net(n, blocks, filters, head, seed=seed))


def _engines(kind, n, max_batch):
    """the engine under test and, for a network, a second one the oracle evaluates its leaves with; oracle.Search keywords"""
    import tak_amd
    from oracle import oracle as orc

    if kind == "hash":
        head = tak_amd.HEAD_FC5 if n == 5 else tak_amd.HEAD_CONV
        e = tak_amd.Engine(n, evaluator=tak_amd.EVAL_HASH, max_batch=max_batch, policy_head=head)
        return e, None, dict(head=orc.HEAD_FC5 if n == 5 else orc.HEAD_CONV, evaluator=orc.EVAL_HASH)
    gn, blocks, filters, head, tensors = _golden_net(kind)
    assert gn == n
    h = tak_amd.HEAD_FC5 if head == "fc5" else tak_amd.HEAD_CONV
    pair = []
    for _ in range(2):
        x = tak_amd.Engine(n, res_blocks=blocks, filters=filters, policy_head=h, evaluator=tak_amd.EVAL_RESNET, max_batch=max_batch)
        x.load_state_dict(tensors)
        pair.append(x)
    e, ev = pair
    return e, ev, dict(head=orc.HEAD_FC5 if head == "fc5" else orc.HEAD_CONV, py_eval=lambda st: ev.policy_eval(st))


@functools.lru_cache(maxsize=None)
def _three_roots(n):
    """a middle-game position; a position one ply before the end of a game (terminal leaves inside every batch); the
    position with the fewest legal moves among 3000 wall-heavy playouts one ply before their board fills up (fewer children
    than a batch of 16 has rollouts: the virtual visits pile up on the same children)"""
    from oracle import oracle as orc

    mid = orc.random_positions(n, 16, seed=12, max_plies=20, half_komi=4)
    mid = mid[orc.result(n, mid) == 0][0]
    late = orc.playouts(n, 8, seed=3, style=0, half_komi=4)["prev"]
    late = late[orc.result(n, late) == 0][0]
    full = orc.playouts(n, 3000, seed=7, style=2, half_komi=4, avoid_roads=True)["prev"]
    full = full[orc.result(n, full) == 0]
    counts = orc.movegen(n, full)[1]
    few = full[int(np.argmin(counts))]
    assert 0 < counts.min() < 16
    return np.stack([mid, late, few])


class Replay:
    """One ply of self_play_parallel (oracle/tak_mcts.hpp SelfPlay::ply_step) around `oracle.Search(batch = B)`, for a run
    without recycling (total_games = games: a finished game retires its slot) and slot_base 0 — every game is generation 0 of
    its slot, so the search's own RNG keys (seed, game, 0, ply) are the driver's."""

    def __init__(self, orc, n, games, batch, rollouts, noise_plies, exploit_plies, noise_alpha=0.2, noise_ratio=0.3, komi=2, seed=0,
                 **search_kw):
        self.orc, self.n, self.G = orc, n, games
        self.rollouts, self.noise_plies, self.exploit_plies = rollouts, noise_plies, exploit_plies
        self.noise_alpha, self.noise_ratio, self.seed = noise_alpha, noise_ratio, seed
        self.s = orc.Search(n, batch=batch, seed=seed, **search_kw)
        self.start = orc.new_game(n, half_komi=2 * komi)
        self.hdr = len(self.start) - 16
        self.s.reset(np.stack([self.start] * games))
        self.alive = np.ones(games, bool)
        self.staged = [[] for _ in range(games)]
        self.examples = []  # (game_id, n_moves, result, state, moves, visits) in the order they are emitted
        self.stats = dict(games_finished=0, examples=0, white_wins=0, black_wins=0, draws=0, instant_wins=0)

    def _to_move(self, st):
        return int(st[self.hdr + 1])

    def _ply(self, st):
        return int(st[self.hdr + 2]) | (int(st[self.hdr + 3]) << 8)

    def _mask(self):
        return self.alive.astype(np.uint8)

    def _finish(self, g, result):
        st = self.stats
        st["games_finished"] += 1
        white = 1.0 if result in (WHITE_ROAD, WHITE_FLAT) else -1.0 if result in (BLACK_ROAD, BLACK_FLAT) else 0.0
        st["white_wins" if white > 0 else "black_wins" if white < 0 else "draws"] += 1
        for state, moves, visits in self.staged[g]:
            self.examples.append((g, len(moves), white if self._to_move(state) == 0 else -white, state, moves, visits))
        st["examples"] += len(self.staged[g])
        self.staged[g] = []
        self.alive[g] = False  # completed + games < total_games never holds when total_games = games

    def before_the_pick(self):
        """phases (a) – (d); returns the roots' (moves, visits, counts) the pick chooses from"""
        orc, n, G = self.orc, self.n, self.G
        sts = self.s.states()
        # (a) opening: a1, then one of the two far corners (the same counter-based draw as the driver's)
        if all(self._ply(sts[g]) == 0 for g in range(G)):
            sts, status = orc.play(n, sts, np.zeros(G, np.uint16))
            assert not status.any()
            corner = np.zeros(G, np.uint16)
            for g in range(G):
                r = orc.philox(self.seed, g, 0, 0 | (1 << 16), 0)  # rng_draw(seed, slot, generation, ply 0, RNG_OPENING, 0, 0)
                corner[g] = (n - 1) * n + (0 if int(r[0]) & 1 else n - 1)
            sts, status = orc.play(n, sts, corner)
            assert not status.any()
            self.s.reset(sts)
        # (b) instant-win scan: an example with fake visits (1000 on every winning move, 1 elsewhere), Winner{to_move, flat}
        mv, cnt = orc.movegen(n, sts)
        for g in range(G):
            if not self.alive[g]:
                continue
            c = int(cnt[g])
            nxt, status = orc.play(n, np.repeat(sts[g][None], c, 0), mv[g, :c])
            assert not status.any()
            res = orc.result(n, nxt)
            mine = (WHITE_ROAD, WHITE_FLAT) if self._to_move(sts[g]) == 0 else (BLACK_ROAD, BLACK_FLAT)
            wins = np.isin(res, mine)
            if wins.any():
                self.staged[g].append((sts[g].copy(), mv[g, :c].copy(), np.where(wins, 1000, 1).astype(np.uint32)))
                self.stats["instant_wins"] += 1
                self._finish(g, WHITE_FLAT if self._to_move(sts[g]) == 0 else BLACK_FLAT)
        # (c) one batch, then Dirichlet noise (Player::add_noise) for the games under noise_plies
        noisy = np.array([self.alive[g] and self._ply(sts[g]) < self.noise_plies for g in range(G)], np.uint8)
        if noisy.any():
            self.s.run(1, noisy)
            self.s.apply_dirichlet(self.noise_alpha, self.noise_ratio, noisy)
        # (d) `rollouts` iterations of one batch each
        if self.alive.any():
            self.s.run(self.rollouts, self._mask())
        r = self.s.root()
        return r["moves"], r["visits"], r["counts"]

    def exploit_pick(self, moves, visits, counts):
        """pick_move(true): the most visited child, the LAST one on ties"""
        out = np.zeros(self.G, np.uint16)
        for g in np.nonzero(self.alive)[0]:
            c = int(counts[g])
            out[g] = moves[g, c - 1 - int(np.argmax(visits[g, :c][::-1]))]
        return out

    def play(self, picked, moves, visits, counts):
        """phase (e) with the given moves: example, play, result, finish"""
        orc, n = self.orc, self.n
        sts = self.s.states()
        for g in np.nonzero(self.alive)[0]:
            c = int(counts[g])
            self.staged[g].append((sts[g].copy(), moves[g, :c].copy(), visits[g, :c].copy()))
        assert self.s.play(picked, self._mask()) == 0
        res = orc.result(n, self.s.states())
        for g in np.nonzero(self.alive)[0]:
            if res[g] != 0:
                self._finish(g, int(res[g]))

    def rollouts_run(self):
        return self.s.counters()[0]


def _engine_examples(drain):
    hdr, states, moves, visits = drain
    return [(int(hdr["game_id"][i]), int(hdr["n_moves"][i]), float(hdr["result"][i]), states[i], moves[i, : hdr["n_moves"][i]],
             visits[i, : hdr["n_moves"][i]]) for i in range(len(hdr))]


def _assert_same_examples(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a[:3] == b[:3], (i, a[:3], b[:3])
        assert np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5]), (i, a[0])
