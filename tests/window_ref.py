"""What tests/test_window_ring.py (CPU) and tests/test_gpu_window.py (GPU) share about the example window's training case: its
shapes, and a numpy statement of k_window_gather (tak_amd/csrc/window_kernels.hip) in which three mistakes can be planted.

The case (tg_window_train = tg_train, test 6 of the GPU file): a window of CAPACITY 48 receives PUSHED = 78 examples, so example k
lives at row k % 48, the 30 oldest are evicted and logical index 0 (example 30) is at row HEAD = 30.  The trained range [FIRST,
FIRST + COUNT) = [3, 40) occupies rows 33 … 47, 0 … 21: it wraps the physical end.  With CHUNK = 8 its 37 examples give 4 chunks
(both example sets are used twice; with chunks_in_step = 2 an optimiser step falls in the middle of the call) and a remainder of 5.
"""
import numpy as np

CAPACITY, PUSHED, FIRST, COUNT, CHUNK, CHUNKS_IN_STEP = 48, 78, 3, 37, 8, 2
HEAD = PUSHED % CAPACITY  # row of logical index 0: the window is full, the next example to enter evicts this row
PUSHES = (5, 20, 1, 30, 22)  # sums to PUSHED; the fourth wraps the physical end
SEEDS = (11, 13)             # of the two training calls: both train on the row behind the wrap (tests/test_window_ring.py)
FIELDS = ("states", "n_moves", "moves", "visits", "results")
assert sum(PUSHES) == PUSHED and HEAD == 30 and HEAD + FIRST < CAPACITY < HEAD + FIRST + COUNT


def canonical(ex):
    """the rows as a window keeps them: nothing past n_moves"""
    out = {k: np.array(v, copy=True) for k, v in ex.items()}
    keep = np.arange(out["moves"].shape[1])[None, :] < out["n_moves"][:, None]
    out["moves"] *= keep.astype(out["moves"].dtype)
    out["visits"] *= keep.astype(out["visits"].dtype)
    return out


def physical(ex, capacity=CAPACITY):
    """the window's arrays after the examples `ex` (oldest first) have entered an empty window: example k at row k % capacity.
    One row more than the window has, filled with a pattern no example holds: an index one past the end reads it, as a kernel
    would read its neighbour's memory."""
    ex = canonical(ex)
    total = len(ex["n_moves"])
    phys = {}
    for k in FIELDS:
        a = np.full((capacity + 1,) + ex[k].shape[1:], 0xA5 if ex[k].dtype.kind in "ui" else -7.0, ex[k].dtype)
        for j in range(max(0, total - capacity), total):
            a[j % capacity] = ex[k][j]
        phys[k] = a
    return phys


def gather(phys, head, first, order, chunk, size=CHUNK, capacity=CAPACITY, mistake=None):
    """chunk `chunk` of the call as k_window_gather fills an example set: example i of the chunk is logical first +
    order[chunk·size + i], logical j is row (head + j) % capacity; zt holds the example's result 8 times.
    mistake: "physical_order" — the permutation indexes rows from row 0 instead of logical indices from the oldest example;
             "zt_row"         — the value target comes from the chunk's i-th example in window order, not in shuffled order;
             "late_wrap"      — the wrap happens one row late (row `capacity` is read instead of row 0)."""
    o = np.asarray(order[chunk * size:(chunk + 1) * size], np.int64)
    unshuffled = np.arange(chunk * size, (chunk + 1) * size, dtype=np.int64)

    def rows(offsets):
        r = head + first + offsets
        if mistake == "physical_order":
            return (first + offsets) % capacity
        if mistake == "late_wrap":
            return np.where(r > capacity, r - capacity, r)
        return r % capacity

    src = rows(o)
    zsrc = rows(unshuffled) if mistake == "zt_row" else src
    out = {k: phys[k][src] for k in ("states", "n_moves", "moves", "visits")}
    out["zt"] = np.repeat(phys["results"][zsrc], 8)
    return out


def same(a, b):
    return all(np.array_equal(a[k].view(np.uint8) if a[k].dtype.kind == "f" else a[k], b[k].view(np.uint8) if b[k].dtype.kind == "f" else b[k])
               for k in a)
