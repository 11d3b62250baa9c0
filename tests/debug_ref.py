"""Node::debug (alpha-tak/src/search/debug.rs:9-51) restated over a tree dump — the depth-first TgNodeRecord list of tg_search_dump /
oracle.Search.dump, where n_children = 0xFFFF marks an uninitialised child — returning exactly the arrays tg_search_debug returns for
one game.  Written against the records alone, so it checks the device ranking and walk without sharing code with them."""
import numpy as np

MAX_MOVES = 512
UNINIT = 0xFFFF


class _Node:
    __slots__ = ("move", "visits", "q", "prior", "init", "children")


def parse(records):
    """the record list → root _Node (children in child order)"""
    nodes = []
    for r in records:
        nd = _Node()
        nd.move = int(r["move"])
        nd.init = int(r["n_children"]) != UNINIT
        nd.visits = int(r["visits"])
        nd.q = np.array([r["q_bits"]], np.uint32).view(np.float32)[0]
        nd.prior = np.array([r["prior_bits"]], np.uint32).view(np.float32)[0]
        nd.children = []
        nodes.append((nd, int(r["n_children"]) if nd.init else 0))
    root = nodes[0][0]
    stack = [[nodes[0][0], nodes[0][1]]]  # (node, children still to attach)
    for nd, nch in nodes[1:]:
        while stack[-1][1] == 0:
            stack.pop()
        stack[-1][0].children.append(nd)
        stack[-1][1] -= 1
        stack.append([nd, nch])
    return root


def continuation(node, depth):
    """Node::continuation: while the node is initialised and has children, its most visited child (last on ties)"""
    out = []
    while len(out) < depth and node.init and node.children:
        best = max(range(len(node.children)), key=lambda i: (node.children[i].visits, i))
        node = node.children[best]
        out.append((node.move, node.visits))
    return out


def eval_f32(visits, rewards):
    """NodeDebugInfo::eval in f32, in list order"""
    total = np.float32(int(np.sum(np.asarray(visits, np.uint64))) & 0xFFFFFFFF)
    acc = np.float32(0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for v, r in zip(visits, rewards):
            acc = np.float32(acc + np.float32(np.float32(r) * np.float32(np.float32(v) / total)))
    return acc


def debug_ref(records, depth, top_k):
    root = parse(records) if not isinstance(records, _Node) else records
    kids = root.children
    order = sorted(range(len(kids)), key=lambda i: (kids[i].visits, i), reverse=True)
    out = dict(moves=np.zeros(MAX_MOVES, np.uint16), visits=np.zeros(MAX_MOVES, np.uint32), reward=np.zeros(MAX_MOVES, np.float32),
               policy=np.zeros(MAX_MOVES, np.float32), cont_moves=np.zeros((top_k, depth), np.uint16),
               cont_visits=np.zeros((top_k, depth), np.uint32), cont_len=np.zeros(top_k, np.int32))
    for r, i in enumerate(order):
        c = kids[i]
        out["moves"][r], out["visits"][r], out["reward"][r], out["policy"][r] = c.move, c.visits, c.q, c.prior
        if r < top_k:
            cont = continuation(c, depth)
            out["cont_len"][r] = len(cont)
            for l, (m, v) in enumerate(cont):
                out["cont_moves"][r, l], out["cont_visits"][r, l] = m, v
    out["counts"] = np.int32(len(kids))
    out["eval"] = eval_f32(out["visits"][: len(kids)], out["reward"][: len(kids)])
    return out


def assert_same(dev, g, ref, depth=None, top_k=None):
    """row g of Engine.search_debug's arrays == debug_ref's, floats as bits (an all-zero-visit root's NaN eval by isnan)"""
    for k in ("moves", "visits", "cont_moves", "cont_visits", "cont_len"):
        assert np.array_equal(dev[k][g], ref[k]), (g, k)
    for k in ("reward", "policy"):
        assert np.array_equal(dev[k][g].view(np.uint32), ref[k].view(np.uint32)), (g, k)
    assert int(dev["counts"][g]) == int(ref["counts"]), g
    a, b = np.float32(dev["eval"][g]), np.float32(ref["eval"])
    if np.isnan(b):
        assert np.isnan(a), g
    else:
        assert np.array([a]).view(np.uint32)[0] == np.array([b]).view(np.uint32)[0], (g, a, b)


def records(tree):
    """hand-built trees for the CPU tests: tree = (move, visits, q, prior, [children]) or (move, q, prior) for an uninitialised
    child → the depth-first record list"""
    from tak_amd.engine import NODE_RECORD

    out = []

    def walk(t):
        if len(t) == 3:
            m, q, p = t
            out.append((m, UNINIT, 0, 0, 0, _bits(p), _bits(q)))
            return
        m, v, q, p, ch = t
        out.append((m, len(ch), v, 0, 0, _bits(p), _bits(q)))
        for c in ch:
            walk(c)

    walk(tree)
    return np.array(out, NODE_RECORD)


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])
