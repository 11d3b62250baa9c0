"""Reference for proven values in the search tree (tg_search_set_proof): a Python MCTS on the oracle's RULES — oracle.play /
movegen / result / move_index / state_hash — with the solver backup and the proof-aware pick of include/takgpu.h on top.

The oracle's own tree code cannot take the rule, so the search is restated here: per-node numpy arrays, every f32 operation
done singly in np.float32 in the order of oracle/tak_mcts.hpp:223-272 (numpy's elementwise f32 operations round once each and
fuse nothing), logf from libm through ctypes as the oracle's, `batch` virtual rollouts per iteration ordered as
oracle.Search(batch=B) orders them.  With proof=False the dumps equal oracle.Search's bit for bit (tests/test_proof_ref.py pins
that), so proof=True differs from the oracle by the rule alone.

`Tree(..., variant=...)` plants one deliberate mistake (VARIANTS); the teeth tests check that a named check rejects each."""
import ctypes as C
import ctypes.util

import numpy as np

from oracle import oracle

NODE_RECORD = oracle.NODE_RECORD
ONGOING, WHITE_ROAD, WHITE_FLAT, BLACK_ROAD, BLACK_FLAT, DRAW, DRAW_REVERSIBLE = range(7)
PROVEN_WHITE, PROVEN_BLACK, PROVEN_DRAW = 8, 9, 10
W, B, D, UNKNOWN = 0, 1, 2, 3  # statuses: the colours are the colour codes of the packed state (white 0, black 1)
_STATUS = np.full(16, UNKNOWN, np.int64)
_STATUS[[WHITE_ROAD, WHITE_FLAT, PROVEN_WHITE]] = W
_STATUS[[BLACK_ROAD, BLACK_FLAT, PROVEN_BLACK]] = B
_STATUS[[DRAW, DRAW_REVERSIBLE, PROVEN_DRAW]] = D
VARIANTS = ("and_with_unknown", "draw_is_loss", "wrong_parity", "status_lost_in_play", "pick_first_proven")

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]
F = np.float32
ONE = F(1.0)


def status(code):
    """W / B / D / UNKNOWN of a result code (0, a TgResult or a TgProven); arrays too"""
    return _STATUS[np.asarray(code, np.int64)]


def proven_code(color):
    return PROVEN_WHITE if color == W else PROVEN_BLACK


def rule(child_codes, c, variant=None):
    """the rule of include/takgpu.h for an initialised ongoing node whose mover has colour c: the TG_PROVEN_* code, or 0"""
    st = status(child_codes)
    if (st == c).any():
        return proven_code(c)
    unknown = (st == UNKNOWN).any()
    if variant == "and_with_unknown":
        unknown = (st == UNKNOWN).all()
    if unknown:
        return 0
    if (st == D).any() and variant != "draw_is_loss":
        return PROVEN_DRAW
    return proven_code(c ^ 1)


def to_move(state):
    return int(state[len(state) - 16 + 1])


def ply_of(state):
    h = len(state) - 16
    return int(state[h + 2]) | (int(state[h + 3]) << 8)


def hash_evaluator(n):
    """TG_EVAL_HASH: state → (priors of the given policy indices, eval), through orc_hash_policy / orc_hash_eval"""
    lib = oracle.lib()

    def ev(state):
        h = oracle.state_hash(n, state)
        return (lambda idx: np.array([lib.orc_hash_policy(h, int(i)) for i in idx], F)), F(lib.orc_hash_eval(h))

    return ev


def callable_evaluator(py_eval):
    """py_eval(states[k, bytes]) → (policy[k, P], eval[k]), as oracle.Search(py_eval=...) takes it"""
    def ev(state):
        p, e = py_eval(np.ascontiguousarray(state, np.uint8)[None])
        p = np.asarray(p, F).reshape(-1)
        return (lambda idx: p[np.asarray(idx, np.int64)]), F(np.asarray(e, F).reshape(-1)[0])

    return ev


def pick(visits, codes, mover, exploit, seed=0, slot=0, generation=0, ply=0, variant=None):
    """The proof-aware pick of include/takgpu.h on a root's children (visits, result codes) → (child index, step, excluded):
    step 1 = a child decided for the mover was played, 2 = pick_move on the candidates; excluded = children step 2 left out."""
    visits = np.asarray(visits, np.uint32)
    st = status(codes)
    last_max = lambda idx: int(idx[len(idx) - 1 - int(np.argmax(visits[idx][::-1]))])  # most visited, the LAST on ties
    mine = np.nonzero(st == mover)[0]
    if len(mine):
        return (int(mine[0]) if variant == "pick_first_proven" else last_max(mine)), 1, 0
    cand = np.nonzero(st != (mover ^ 1))[0]
    if not len(cand):
        cand = np.arange(len(visits))
    excluded = len(visits) - len(cand)
    if exploit or int(visits[cand].astype(np.uint64).sum()) == 0:
        return last_max(cand), 2, excluded
    v = np.zeros_like(visits)
    v[cand] = visits[cand]
    i = oracle.pick_move(v, False, seed, slot, generation, ply)
    assert i >= 0
    return i, 2, excluded


class Tree:
    """One game's search tree.  Node i: prior, q, visits, virt, code (result nibble), the move that leads to it, and its
    children block [cbase, cbase + nchild) in possible_moves order."""

    def __init__(self, n, state, evaluator, base=500.0, init=4.0, batch=1, proof=False, variant=None):
        assert variant is None or variant in VARIANTS
        self.n, self.ev, self.batch, self.proof, self.variant = n, evaluator, max(1, batch), proof, variant
        self.base, self.init = F(base), F(init)
        cap = 1024
        self.prior, self.q = np.zeros(cap, F), np.zeros(cap, F)
        self.visits, self.virt = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        self.code, self.move = np.zeros(cap, np.uint8), np.zeros(cap, np.uint16)
        self.cbase, self.nchild = np.zeros(cap, np.int64), np.zeros(cap, np.int64)
        self.used = 1
        self.root = 0
        self.state = np.ascontiguousarray(state, np.uint8).copy()
        self.rollouts = self.evals = self.nodes_proven = self.ended_on_proven = 0
        self.proven_by = {}  # node → "or" (a child decided for the mover) / "and" (no child unknown), with its depth at the time
        self._ctab = {}

    # ---- arithmetic, tak_mcts.hpp:223-234 ----
    def _rate(self, total):
        r = self._ctab.get(total)
        if r is None:
            nf = F(total)
            r = self._ctab[total] = F(_libm.logf(float(((ONE + nf) + self.base) / self.base))) + self.init
        return r

    def _update_concrete(self, i, reward):
        cumulative = self.q[i] * F(self.visits[i])
        self.visits[i] += 1
        self.q[i] = (cumulative + F(reward)) / F(self.visits[i])

    def _grow(self, need):
        if self.used + need <= len(self.prior):
            return
        cap = max(2 * len(self.prior), self.used + need)
        for name in ("prior", "q", "visits", "virt", "code", "move", "cbase", "nchild"):
            a = getattr(self, name)
            b = np.zeros(cap, a.dtype)
            b[: len(a)] = a
            setattr(self, name, b)

    def _select(self, i):
        """select, tak_mcts.hpp:239-253: the child with the largest upper confidence bound, the LAST on ties"""
        sl = slice(self.cbase[i], self.cbase[i] + self.nchild[i])
        total = int(self.visits[i]) + int(self.virt[i])
        vc = F(total)
        v, vv = self.visits[sl], self.virt[sl]
        cn = (v + vv).astype(F)
        with np.errstate(invalid="ignore", divide="ignore"):
            qwl = np.where((v | vv) != 0, (self.q[sl] * v.astype(F) - vv.astype(F)) / cn, F(0.0)).astype(F)
        ucb = qwl + (self._rate(total) * self.prior[sl]) * (np.sqrt(vc) / (ONE + cn))
        assert ucb.dtype == F and not np.isnan(ucb).any()
        return int(sl.start) + len(ucb) - 1 - int(np.argmax(ucb[::-1]))

    # ---- virtual_rollout, tak_mcts.hpp:256-275, iteratively ----
    def _rollout(self):
        path, st, i = [self.root], self.state, self.root
        fresh = False
        while True:
            if self.visits[i] == 0 and self.virt[i] == 0:
                res = int(oracle.result(self.n, st)[0])
                self.code[i] = res
                if res == ONGOING:
                    moves, counts = oracle.movegen(self.n, st)
                    c = int(counts[0])
                    self._grow(c)
                    a = self.used
                    self.used += c
                    self.cbase[i], self.nchild[i] = a, c
                    self.move[a : a + c] = moves[0, :c]
                    self.prior[a : a + c] = ONE / F(c)
                fresh = True
                break
            res = int(self.code[i])
            if res != ONGOING:
                if res >= PROVEN_WHITE:
                    self.ended_on_proven += 1
                break
            i = self._select(i)
            st = oracle.play(self.n, st, [self.move[i]])[0][0]
            path.append(i)
        self.rollouts += 1
        root_color = to_move(self.state)
        s = int(status(res))
        for d, nd in enumerate(path):
            if res == ONGOING:
                self.virt[nd] += 1
            else:
                curr = root_color ^ (d & 1)
                self._update_concrete(nd, 0.0 if s == D else (-1.0 if s == curr else 1.0))
        if self.proof and fresh and res != ONGOING:
            self._walk(path, root_color, s)
        return (path, st) if res == ONGOING else None

    def _walk(self, path, root_color, child_status):
        """the rule upward from the parent of the terminal node just initialised; stops at the first node that stays unknown"""
        for d in range(len(path) - 2, -1, -1):
            x = path[d]
            c = root_color ^ (d & 1)
            if self.variant == "wrong_parity":
                c ^= 1
            if child_status == c:
                code, how = proven_code(c), "or"
            else:
                code = rule(self.code[self.cbase[x] : self.cbase[x] + self.nchild[x]], c, self.variant)
                how = "or" if code == proven_code(c) else "and"
            if not code:
                return
            self.code[x] = code
            self.nodes_proven += 1
            self.proven_by[x] = (how, d)
            child_status = int(status(code))

    # ---- devirtualize_path, tak_mcts.hpp:278-291 ----
    def _devirtualize(self, path, leaf_state, evaluated=None):
        priors_of, e = evaluated if evaluated is not None else self.ev(leaf_state)
        leaf = path[-1]
        a, c = int(self.cbase[leaf]), int(self.nchild[leaf])
        self.prior[a : a + c] = priors_of(oracle.move_index(self.n, self.move[a : a + c]))
        self.evals += 1
        val = F(e)
        for nd in reversed(path):
            self.virt[nd] -= 1
            val = -val
            self._update_concrete(nd, val)

    def run(self, iters):
        """`iters` iterations of `batch` virtual rollouts, one evaluation of their leaves, the de-virtualisations in order"""
        for _ in range(iters):
            leaves = [r for r in (self._rollout() for _ in range(self.batch)) if r is not None]
            for path, st in leaves:
                self._devirtualize(path, st)

    @staticmethod
    def run_lockstep(trees, iters, py_eval):
        """`iters` iterations of all trees with ONE evaluator call per iteration on the leaves of all of them, game by game in
        rollout order — how oracle.Search(py_eval=...) and the engine batch a network; py_eval(states[k]) → (policy[k, P], eval[k])"""
        for _ in range(iters):
            leaves = [(t, r) for t in trees for r in (t._rollout() for _ in range(t.batch)) if r is not None]
            if not leaves:
                continue
            pol, ev = py_eval(np.stack([st for _, (_, st) in leaves]))
            pol, ev = np.asarray(pol, F), np.asarray(ev, F)
            for k, (t, (path, st)) in enumerate(leaves):
                t._devirtualize(path, st, ((lambda idx, k=k: pol[k][np.asarray(idx, np.int64)]), ev[k]))

    # ---- Node::play with tree reuse ----
    def play(self, move):
        sl = slice(self.cbase[self.root], self.cbase[self.root] + self.nchild[self.root])
        hit = np.nonzero(self.move[sl] == move)[0]
        assert len(hit) == 1, "move is not a child of the root"
        self.root = int(sl.start) + int(hit[0])
        self.state = oracle.play(self.n, self.state, [move])[0][0]
        if self.variant == "status_lost_in_play" and self.code[self.root] >= PROVEN_WHITE:
            self.code[self.root] = ONGOING

    def root_children(self):
        """(moves, visits, codes) of the root's children"""
        sl = slice(self.cbase[self.root], self.cbase[self.root] + self.nchild[self.root])
        return self.move[sl].copy(), self.visits[sl].copy(), self.code[sl].copy()

    def pick(self, exploit, seed=0, slot=0, generation=0):
        _, visits, codes = self.root_children()
        return pick(visits, codes, to_move(self.state), exploit, seed, slot, generation, ply_of(self.state), self.variant)

    def walk(self):
        """every initialised node, depth-first in child order: (node, depth, packed state)"""
        stack = [(self.root, 0, self.state)]
        while stack:
            i, d, st = stack.pop()
            yield i, d, st
            a, c = int(self.cbase[i]), int(self.nchild[i])
            kids = [k for k in range(a, a + c) if self.visits[k] or self.virt[k]]
            if kids:
                nxt = oracle.play(self.n, np.repeat(st[None], len(kids), 0), self.move[kids])[0]
                stack.extend((k, d + 1, nxt[j]) for j, k in reversed(list(enumerate(kids))))

    def dump(self):
        """TgNodeRecord layout, as tg_search_dump / oracle.Search.dump"""
        out = []

        def rec(i, is_root):
            init = is_root or self.visits[i] != 0 or self.virt[i] != 0
            out.append((0 if is_root else self.move[i], self.nchild[i] if init else 0xFFFF, self.visits[i], self.virt[i],
                        self.code[i] if init else 0, self.prior[i : i + 1].view(np.uint32)[0], self.q[i : i + 1].view(np.uint32)[0]))
            return init

        stack = [(self.root, True)]
        while stack:
            i, is_root = stack.pop()
            if rec(i, is_root):
                a, c = int(self.cbase[i]), int(self.nchild[i])
                stack.extend((k, False) for k in range(a + c - 1, a - 1, -1))
        return np.array(out, NODE_RECORD)


# ---- the checks the tests use, on a Tree ---------------------------------------------------------------------------------
def check_closure(t):
    """The invariant: every proven node satisfies the rule, no unproven initialised ongoing node does.  → list of faults"""
    bad = []
    for i, d, st in t.walk():
        code = int(t.code[i])
        if code != ONGOING and code < PROVEN_WHITE:
            continue
        want = rule(t.code[t.cbase[i] : t.cbase[i] + t.nchild[i]], to_move(st)) if t.nchild[i] else 0
        if want != code:
            bad.append(f"closure: node {i} at depth {d} holds {code}, the rule on its children gives {want}")
    return bad


def check_sound(t):
    """Every proven node's status follows structurally from its children, the finished ones re-judged by oracle.result on
    their replayed positions (nothing here calls `rule`): a node proven for its mover has a child of that status; one proven
    against its mover has every child initialised and of the opponent's status; a proven draw has every child decided, none
    for the mover, at least one drawn.  → list of faults"""
    bad = []
    for i, d, st in t.walk():
        code = int(t.code[i])
        a, c = int(t.cbase[i]), int(t.nchild[i])
        if code < PROVEN_WHITE:
            if code != int(oracle.result(t.n, st)[0]) and (t.visits[i] or t.virt[i]):
                bad.append(f"sound: node {i} holds result {code}, the rules say {int(oracle.result(t.n, st)[0])}")
            continue
        m = to_move(st)
        kids = oracle.play(t.n, np.repeat(st[None], c, 0), t.move[a : a + c])[0]
        real = oracle.result(t.n, kids)
        cs = []
        for k in range(c):
            kc = int(t.code[a + k])
            if kc != ONGOING and kc < PROVEN_WHITE and kc != int(real[k]):
                bad.append(f"sound: child {k} of node {i} holds result {kc}, the rules say {int(real[k])}")
            cs.append(int(status(kc)))
        s = int(status(code))
        if s == m:
            ok = m in cs
        elif s == D:
            ok = UNKNOWN not in cs and m not in cs and D in cs
        else:
            ok = all(x == (m ^ 1) for x in cs)
        if not ok:
            bad.append(f"sound: node {i} at depth {d}, mover {m}, holds {code} over children of status {cs}")
    return bad


def proof_depth(t, i=None):
    """plies of the proof tree the walk built below a proven node (a finished child counts 0): a node proven through one child
    decided for its mover needs the shallowest such child, any other proven node needs every child"""
    i = t.root if i is None else i
    a, c = int(t.cbase[i]), int(t.nchild[i])
    sub = lambda k: proof_depth(t, k) if t.code[k] >= PROVEN_WHITE else 0
    if t.proven_by[i][0] == "or":
        s = int(status(t.code[i]))
        return 1 + min(sub(k) for k in range(a, a + c) if int(status(t.code[k])) == s)
    return 1 + max(sub(k) for k in range(a, a + c))


# ---- the inputs and the reference runs the CPU and the GPU tests share (each computed once per process) --------------------
# 5×5: near-end positions of tests/golden/solve_cases.json whose exact depth-5 value is a win or a loss within 3 plies, by
# their index into tactics_ref.positions("p5_160"): a win at once for either colour (0, 8), a loss in 2 (5: the only one of the
# set whose root the all-children rule decides, after ≈ 4400 rollouts under the hash evaluator; 1), wins in 3 (28, 155).
# 6×6: the file holds no 6×6 positions; the same kind of position from the same generator, oracle.playouts(6, 12, 7)["prev"].
# ROLLOUTS: the smallest round counts at which the reference alone meets the floors of tests/test_proof_ref.py.
CASES = {5: (0, 8, 5, 28, 155, 1), 6: (4, 5, 8, 9, 7, 10)}
ROLLOUTS = {5: 4500, 6: 1600}


def inputs(n):
    import json
    import os

    import tactics_ref

    if n == 5:
        doc = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solve_cases.json")))
        value = {c["index"]: c["depth5"]["value"] for c in doc["cases"]}
        assert all(1 <= abs(value[i]) <= 3 for i in CASES[5])
        return np.ascontiguousarray(tactics_ref.positions(doc["set"])[list(CASES[5])])
    pos = oracle.playouts(6, 12, 7)["prev"]
    assert not oracle.result(6, pos).any()
    return np.ascontiguousarray(pos[list(CASES[6])])


_REFERENCE = {}


def reference(n, batch):
    """The reference's run on inputs(n): ROLLOUTS[n] rollouts under proof=True, the exploit pick played on every game, as
    many rollouts again.  → dict(trees, dumps = [before the play, after], children = (moves, visits, codes) per game before
    the play, roots = root codes [before, after], root_depth = proof_depth of the proven roots before, picked, counters = [(nodes proven, ended on proven) before, after])"""
    key = (n, batch)
    if key not in _REFERENCE:
        sts = inputs(n)
        iters = ROLLOUTS[n] // batch
        trees = [Tree(n, st, hash_evaluator(n), batch=batch, proof=True) for st in sts]
        out = dict(trees=trees, dumps=[], roots=[], counters=[], iters=iters)

        def snap():
            out["dumps"].append([t.dump() for t in trees])
            out["roots"].append([int(t.code[t.root]) for t in trees])
            out["counters"].append((sum(t.nodes_proven for t in trees), sum(t.ended_on_proven for t in trees)))

        for t in trees:
            t.run(iters)
        snap()
        out["children"] = [t.root_children() for t in trees]
        out["proven_by"] = [dict(t.proven_by) for t in trees]
        out["picked"] = np.array([t.root_children()[0][t.pick(True)[0]] for t in trees], np.uint16)
        out["root_depth"] = [proof_depth(t) if t.code[t.root] >= PROVEN_WHITE else None for t in trees]
        out["faults"] = [check_closure(t) + check_sound(t) for t in trees]  # (of the trees before the play)
        for t, mv in zip(trees, out["picked"]):
            t.play(mv)
            t.run(iters)
        snap()
        _REFERENCE[key] = out
    return _REFERENCE[key]


class SelfPlay:
    """self_play_parallel (oracle/tak_mcts.hpp SelfPlay::ply_step, train/src/self_play.rs:96-262) on `Tree`s with proof=True and
    the proof-aware pick: phases (a) – (e) in the driver's order, slots recycled while completed + games < total_games.  Keeps
    what the engine's run is compared with: `picks` (slot, generation, ply, child index, step, excluded, candidates without a
    visit) in the order they are made, `examples` in the order they are emitted, `stats`."""

    def __init__(self, n, games, rollouts, noise_plies, exploit_plies, total_games, noise_alpha=0.2, noise_ratio=0.3, komi=2, seed=0,
                 batch=1, boost_plies=0, boost_factor=1):
        self.n, self.G, self.rollouts, self.batch = n, games, rollouts, batch
        self.noise_plies, self.exploit_plies, self.total_games = noise_plies, exploit_plies, total_games
        self.noise_alpha, self.noise_ratio, self.seed = noise_alpha, F(noise_ratio), seed
        self.boost_plies, self.boost_factor = boost_plies, boost_factor
        self.ev = hash_evaluator(n)
        self.start = oracle.new_game(n, half_komi=2 * komi)
        self.trees = [self._tree(self.start) for _ in range(games)]
        self.alive = [True] * games
        self.generation = [0] * games
        self.staged = [[] for _ in range(games)]
        self.examples, self.picks = [], []
        self.stats = dict(games_finished=0, examples=0, plies=0, white_wins=0, black_wins=0, draws=0, instant_wins=0)
        self.retired = dict(rollouts=0, evals=0, nodes_proven=0, ended_on_proven=0)  # of the trees that were dropped
        self.partial_lists = 0  # boosted rounds that ran over some of the alive games only

    def _tree(self, st):
        return Tree(self.n, st, self.ev, batch=self.batch, proof=True)

    def _drop(self, g, st):
        for k in self.retired:
            self.retired[k] += getattr(self.trees[g], k)
        self.trees[g] = self._tree(st)

    def counters(self):
        return {k: v + sum(getattr(t, k) for t in self.trees) for k, v in self.retired.items()}

    def _finish(self, g, result):
        st = self.stats
        st["games_finished"] += 1
        white = 1.0 if result in (WHITE_ROAD, WHITE_FLAT) else -1.0 if result in (BLACK_ROAD, BLACK_FLAT) else 0.0
        st["white_wins" if white > 0 else "black_wins" if white < 0 else "draws"] += 1
        self._drop(g, self.start)
        if not (self.total_games == 0 or st["games_finished"] + self.G < self.total_games):
            self.alive[g] = False
        gid = g | (self.generation[g] << 20)
        for state, moves, visits in self.staged[g]:
            self.examples.append((gid, len(moves), white if to_move(state) == 0 else -white, state, moves, visits))
        st["examples"] += len(self.staged[g])
        self.staged[g] = []
        self.generation[g] += 1

    def step(self):
        n, G = self.n, self.G
        live = lambda: [g for g in range(G) if self.alive[g]]
        for g in live():  # (a) the opening: a1, then one of the two far corners
            if ply_of(self.trees[g].state) == 0:
                st = oracle.play(n, self.trees[g].state, [0])[0][0]
                r = oracle.philox(self.seed, g, self.generation[g], 0 | (1 << 16), 0)
                st = oracle.play(n, st, [(n - 1) * n + (0 if int(r[0]) & 1 else n - 1)])[0][0]
                self._drop(g, st)
        for g in live():  # (b) the instant-win scan
            st = self.trees[g].state
            mv, cnt = oracle.movegen(n, st)
            c = int(cnt[0])
            res = oracle.result(n, oracle.play(n, np.repeat(st[None], c, 0), mv[0, :c])[0])
            wins = status(res) == to_move(st)
            if wins.any():
                self.staged[g].append((st.copy(), mv[0, :c].copy(), np.where(wins, 1000, 1).astype(np.uint32)))
                self.stats["instant_wins"] += 1
                self._finish(g, WHITE_FLAT if to_move(st) == 0 else BLACK_FLAT)
        for g in live():  # (c) one iteration, then Dirichlet noise on the root's priors
            t = self.trees[g]
            if ply_of(t.state) < self.noise_plies:
                t.run(1)
                a, c = int(t.cbase[t.root]), int(t.nchild[t.root])
                if c and t.visits[t.root]:
                    noise = oracle.dirichlet(c, self.noise_alpha, self.seed, g, self.generation[g], ply_of(t.state))
                    t.prior[a : a + c] = noise * self.noise_ratio + t.prior[a : a + c] * (ONE - self.noise_ratio)
        for g in live():  # (d) the rollouts
            self.trees[g].run(self.rollouts)
        if self.boost_plies > 0 and self.boost_factor > 1:  # the boosted rounds over the games that are owed them
            owed = [g for g in live() if ply_of(self.trees[g].state) < self.boost_plies]
            self.partial_lists += 0 < len(owed) < G
            for g in owed:
                self.trees[g].run((self.boost_factor - 1) * self.rollouts)
        for g in live():  # (e) pick, example, play, result
            t = self.trees[g]
            st = t.state
            moves, visits, codes = t.root_children()
            k, step, excluded = pick(visits, codes, to_move(st), ply_of(st) >= self.exploit_plies, self.seed, g, self.generation[g], ply_of(st))
            unvisited = step == 2 and int(visits[status(codes) != (to_move(st) ^ 1)].astype(np.uint64).sum()) == 0 and excluded < len(codes)
            self.picks.append((g, self.generation[g], ply_of(st), k, step, excluded, unvisited))
            self.staged[g].append((st.copy(), moves, visits))
            t.play(moves[k])
            res = int(oracle.result(n, t.state)[0])
            if res != ONGOING:
                self._finish(g, res)
        self.stats["plies"] += 1
