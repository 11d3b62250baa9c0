"""Search analysis on the host side: `NodeDebugInfo` / `MoveInfo` (reference alpha-tak/src/search/debug.rs) and the annotated PTN
text of `Analysis` (alpha-tak/src/analysis.rs).

The data comes from `tg_search_debug` (`Engine.search_debug`), which ranks the root's children and walks their continuations on the
device; this module only does arithmetic the reference does in f32 (kept in np.float32 here, in the same order) and text.  Moves print
through `tg_format_move`, so only the library has to be loaded (no GPU)."""
import math

import numpy as np

from .engine import format_move

MAX_BRANCH_LENGTH = 10            # analysis.rs:7, the depth Analysis::update asks Node::debug for
BRANCH_MIN_VISITS = 10_000        # analysis.rs:8, continuation moves a branch keeps (strictly more visits)
CANDIDATE_MOVE_RATIO = np.float32(0.9)  # analysis.rs:9

_F0 = np.float32(0.0)


def fmt_f32(x, prec, sign=False):
    """Rust's `{:.prec}` / `{:+.prec}` of an f32 (the value is exact in a double, so the decimal rounding agrees); NaN prints
    as `NaN` with no sign, as Rust does"""
    x = float(np.float32(x))
    if math.isnan(x):
        return "NaN"
    return format(x, f"{'+' if sign else ''}.{prec}f")


class MoveInfo:
    """debug.rs:77-84: one root child — move, visits, reward (expected_reward), policy (prior), continuation [(move, visits)]"""

    def __init__(self, n, mov, visits, reward, policy, continuation=()):
        self.n = int(n)
        self.mov = int(mov)
        self.visits = int(visits)
        self.reward = np.float32(reward)
        self.policy = np.float32(policy)
        self.continuation = [(int(m), int(v)) for m, v in continuation]

    def move_text(self):
        return format_move(self.n, self.mov)

    def ptn_comment(self, flip_reward):
        """debug.rs:87-90"""
        r = -self.reward if flip_reward else self.reward
        return f" {{r: {fmt_f32(r, 3, True)}, p: {fmt_f32(self.policy, 4)}, v: {self.visits}}}"

    def __str__(self):
        """one row of the table (debug.rs:93-107), newline included"""
        cont = " ".join(format_move(self.n, m) for m, _ in self.continuation)
        return (f"{self.move_text(): <8} {self.visits: >8} {fmt_f32(self.reward, 4, True): >8} {fmt_f32(self.policy, 4): >8} | "
                f"{cont}\n")


class NodeDebugInfo:
    """debug.rs:38-75: the root's children in descending order of visits"""

    def __init__(self, infos):
        self.infos = list(infos)

    def __iter__(self):
        return iter(self.infos)

    def __len__(self):
        return len(self.infos)

    def eval(self):
        """debug.rs:43-51: (float)(u32 sum of visits), then +0.0 + Σ reward · (visits / total) in list order, all f32 — no children
        gives +0.0, children without visits NaN"""
        total = np.float32(sum(i.visits for i in self.infos) & 0xFFFFFFFF)
        acc = _F0
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in self.infos:
                acc = np.float32(acc + np.float32(i.reward * np.float32(np.float32(i.visits) / total)))
        return acc

    def maybe_flip(self, flip):
        """debug.rs:53-58: rewards negated (0.0 becomes -0.0); eval follows from the flipped rewards"""
        if not flip:
            return self
        return NodeDebugInfo(MoveInfo(i.n, i.mov, i.visits, np.float32(i.reward * np.float32(-1.0)), i.policy, i.continuation)
                             for i in self.infos)

    def __format__(self, spec):
        """debug.rs:61-75: the precision is the number of rows, `{:.10}`"""
        if not self.infos:
            return "Node has no children"
        rows = self.infos if not spec else self.infos[: int(spec.lstrip("."))]
        head = f"evaluation: {fmt_f32(self.eval(), 4, True)}\nturn      visited   reward   policy | continuation\n"
        return head + "".join(str(i) for i in rows)

    def __str__(self):
        return format(self, "")

    @staticmethod
    def from_search_debug(n, r, g):
        """row g of Engine.search_debug's arrays"""
        infos = []
        c = int(r["counts"][g])
        k = r["cont_len"].shape[1]
        for j in range(c):
            cont = []
            if j < k:
                ln = int(r["cont_len"][g, j])
                cont = zip(r["cont_moves"][g, j, :ln], r["cont_visits"][g, j, :ln])
            infos.append(MoveInfo(n, r["moves"][g, j], r["visits"][g, j], r["reward"][g, j], r["policy"][g, j], cont))
        return NodeDebugInfo(infos)


_MARKS = {"blunder": "??", "mistake": "?", "strong": "!", "brilliancy": "!!"}  # analysis.rs:235-247


def _mark(diff):
    """analysis.rs:64-75 on eval_diff = -(eval + previous eval), f32 and the reference's range ends (first match wins)"""
    lo, mid_lo, mid_hi, hi = np.float32(-0.4), np.float32(-0.15), np.float32(0.1), np.float32(0.3)
    if diff <= lo:
        return "blunder"
    if lo <= diff <= mid_lo:
        return "mistake"
    if mid_hi <= diff <= hi:
        return "strong"
    if diff >= hi:
        return "brilliancy"
    return None


class Analysis:
    """analysis.rs:11-20: an annotated PTN record of a game — evaluation comments, blunder / mistake / strong / brilliancy marks and
    candidate branches"""

    def __init__(self, board_size, half_komi, start_ply):
        """analysis.rs:23-37.  Komi is written as the reference writes it: truncating i8 division and remainder, so
        half_komi = -1 prints "0.5" and -3 prints "-1.5"."""
        hk = int(half_komi)
        whole = int(hk / 2)  # toward zero
        frac = "" if hk - 2 * whole == 0 else ".5"
        self.n = int(board_size)
        self.settings = f'[Size "{self.n}"]\n[Komi "{whole}{frac}"]\n'
        self.start_ply = int(start_ply)
        self.played_moves = []
        self.move_info = []  # MoveInfo or None
        self.branches = []   # (ply, MoveInfo)
        self.evals = []      # np.float32
        self.marks = []      # (ply, kind)
        self.tactics = {}    # index into played_moves → (suffix after the move, comment): annotate_tactics, opt-in

    @classmethod
    def default(cls, board_size):
        """Analysis::default(): what Player::get_analysis leaves behind (std::mem::take) — no settings, start ply 0"""
        a = cls(board_size, 0, 0)
        a.settings = ""
        return a

    def add_setting(self, name, value):
        """analysis.rs:39-41"""
        self.settings += f'[{name} "{value}"]\n'

    def add_move_without_info(self, mov):
        self.played_moves.append(int(mov))
        self.move_info.append(None)

    def add_move(self, mov, info, ev):
        self.played_moves.append(int(mov))
        self.move_info.append(info)
        self.evals.append(np.float32(ev))

    def update(self, debug_info, played_move):
        """analysis.rs:54-92 with the NodeDebugInfo of the position before `played_move` (Node::debug(MAX_BRANCH_LENGTH))"""
        ply = self.start_ply + len(self.played_moves)
        top = debug_info.infos[0].visits if len(debug_info) else 0
        ev = debug_info.eval()
        if self.evals:
            kind = _mark(np.float32(-np.float32(ev + self.evals[-1])))  # the previous eval is from the other side
            if kind:
                self.marks.append((ply - 1, kind))
        for info in debug_info:
            if info.mov == int(played_move):
                self.add_move(played_move, info, ev)
            elif np.float32(info.visits) > np.float32(np.float32(top) * CANDIDATE_MOVE_RATIO):
                self.branches.append((ply, info))

    def annotate_tactics(self, solver, state, played_move, depth, node_budget=1 << 16, road_only=False):
        """Opt-in tactical annotation of the move just recorded (call after update / add_move): `solver` (an Engine) solves
        the position after `played_move` from `state` at `depth` plies (Engine.solve).
          the opponent is proven lost      → `"` after the move, before any ?/! mark, and the comment {forced win in k}
          the move itself is proven losing → the comment {loses in k}
          otherwise, from ply 2 on (the first two plies place the opponent's stone), `'` (Tak) when the mover would win at
          once if it were their turn again: a depth-1 solve of the same position with the header's to_move byte flipped.
        k counts the plies after the move.  With road_only = False a win is one by road OR by flats within `depth` plies, so `"` is
        wider than PTN's mark.  road_only = True gives PTN's own marks: every solve is a road-only proof (Engine.solve's road_only),
        `"` stands for a tinuë, a road that cannot be stopped, with the comments {tinue in k} and {road loss in k}, each followed by
        the proof's principal line (forced_line) as a comment of its own, and `'` for a road threat.
        node_budget: Engine.solve's (one position: see player.TACTICS_BUDGET); a proof the budget cuts off is a missing mark, never a
        wrong one."""
        k = len(self.played_moves) - 1
        if k < 0 or self.played_moves[k] != int(played_move) or self.move_info[k] is None:
            return
        road = {"road_only": True} if road_only else {}  # (the default mode's calls are what they were)
        after, _ = solver.play(np.ascontiguousarray(state, np.uint8).reshape(1, -1), np.array([played_move], np.uint16))
        value = int(solver.solve(after, int(depth), node_budget=int(node_budget), **road)["value"][0])
        line = ""
        if value != 0 and road_only:
            line = " {" + " ".join(format_move(self.n, m) for m in forced_line(solver, after, abs(value), True, node_budget)) + "}"
        if value < 0:
            self.tactics[k] = ('"', (f" {{tinue in {-value}}}" if road_only else f" {{forced win in {-value}}}") + line)
        elif value > 0:
            self.tactics[k] = ("", (f" {{road loss in {value}}}" if road_only else f" {{loses in {value}}}") + line)
        elif self.start_ply + k >= 2:
            again = np.array(after, np.uint8, copy=True)
            again[0, again.shape[1] - 16 + 1] ^= 1  # TgHeader.to_move
            if int(solver.solve(again, 1, node_budget=int(node_budget), **road)["value"][0]) > 0:
                self.tactics[k] = ("'", "")

    def without_branches(self):
        a = Analysis.default(self.n)
        a.__dict__.update({k: list(v) if isinstance(v, list) else v for k, v in self.__dict__.items()})
        a.branches = []
        return a

    def __str__(self):
        """analysis.rs:102-191: settings, one line per move number, then the branches"""
        out = [self.settings]
        n_moves = len(self.played_moves)
        evals = iter(self.evals[1:])  # the comment after a move shows the eval of the position it leads to
        marks = list(self.marks)
        mi = 0
        ply = self.start_ply

        def move_text(k, ply, flip_eval):
            nonlocal mi
            info = self.move_info[k]
            s = format_move(self.n, self.played_moves[k])
            tac = self.tactics.get(k)
            if tac:
                s += tac[0]
            if mi < len(marks) and marks[mi][0] == ply:
                s += _MARKS[marks[mi][1]]
                mi += 1
            if info is not None:
                ev = next(evals, None)
                if ev is not None:
                    ev = np.float32(ev * np.float32(-1.0)) if flip_eval else ev
                    s += f"{{evaluation: {fmt_f32(ev, 3, True)}}}"
                s += info.ptn_comment(not flip_eval)
            if tac:
                s += tac[1]
            return s

        k = 0
        if self.start_ply % 2 != 0:
            line = f"{ply // 2 + 1}. -- "
            if k < n_moves:
                line += move_text(k, ply, False)
                k += 1
            out.append(line + "\n")
            ply += 1
        while k < n_moves:
            line = f"{ply // 2 + 1}. " + move_text(k, ply, True) + " "
            k += 1
            ply += 1
            if k < n_moves:
                line += move_text(k, ply, False)
                k += 1
            out.append(line + "\n")
            ply += 1
        for bply, info in self.branches:
            out.append("\n" + _format_branch(bply, info))
        return "".join(out)


def forced_line(engine, state, depth, road_only=False, node_budget=1 << 16):
    """The principal line of a position proven at `depth` plies (Engine.solve): the moves until the game ends, [] when nothing is
    proven.  Both sides play the solver's `best`: the side with the proof its fastest win, the other side its longest defence;
    after each move the new position is solved again at the plies that remain, so the line has exactly |value| moves and its
    last move ends the game in favour of the side with the proof (with road_only by a road).  `engine` needs solve and play.
    Raises RuntimeError if a step comes back unproven with budget_hit set: the budget, not the position, cut the line."""
    road = {"road_only": True} if road_only else {}
    cur = np.ascontiguousarray(state, np.uint8).reshape(1, -1)
    line, left = [], int(depth)
    while left > 0:
        r = engine.solve(cur, left, node_budget=int(node_budget), **road)
        value = int(r["value"][0])
        if value == 0:
            if "budget_hit" in r and int(r["budget_hit"][0]):
                raise RuntimeError(f"forced_line: node_budget {node_budget} ran out {len(line)} moves into the line")
            if line:
                raise RuntimeError(f"forced_line: the proof does not continue {len(line)} moves into the line")
            break
        line.append(int(r["best"][0]))
        cur, _ = engine.play(cur, np.array([line[-1]], np.uint16))
        left = abs(value) - 1
    return line


def root_eval(engine, states, ensemble=True):
    """The network's own view of root positions, for analysis: (policy [k, P], eval [k]).  ensemble = True evaluates every root with
    the full symmetry ensemble (Engine.policy_eval(symmetries=0xFF): the mean over the 8 dihedral images mapped back to the root's
    orientation) — a quieter evaluation than the single orientation the search sees; False is the plain Network::policy_eval."""
    return engine.policy_eval(states, symmetries=0xFF if ensemble else None)


def _format_branch(ply, info):
    """analysis.rs:194-232: `{ply_move}`, the candidate with its comment, then its continuation moves with more than
    BRANCH_MIN_VISITS visits, two plies a line"""
    cont = [format_move(info.n, m) for m, v in info.continuation if v > BRANCH_MIN_VISITS]
    num = 1 + ply // 2
    out = f"{{{ply}_{info.move_text()}}}\n"
    if ply % 2 == 0:
        first = cont.pop(0) if cont else ""
        out += f"{num}. {info.move_text()} {info.ptn_comment(False)} {first}\n"
    else:
        out += f"{num}. -- {info.move_text()} {info.ptn_comment(True)}\n"
    num += 1
    for i in range(0, len(cont), 2):
        black = cont[i + 1] if i + 1 < len(cont) else ""
        out += f"{num}. {cont[i]} {black}\n"
        num += 1
    return out
