"""ctypes binding of libtakgpu.so (C ABI: include/takgpu.h).  The structures, constants and function signatures come from the
header itself (abi.py); what is written here is the Python surface: Engine, the text formats, pit."""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi
from .abi import *  # noqa: F401,F403  every Tg* structure and TG_* constant of include/takgpu.h, and ALLREDUCE_FN

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TAKGPU_LIB") or os.path.join(_HERE, "libtakgpu.so")  # TAKGPU_LIB: probe builds (scripts/probes)
ABI_SYMBOLS = list(abi.FUNCTIONS)  # every symbol include/takgpu.h declares (tests check the library exports all of them)
HEAD_FC5, HEAD_CONV = TG_HEAD_FC5, TG_HEAD_CONV
EVAL_RESNET, EVAL_DUMMY, EVAL_HASH = TG_EVAL_RESNET, TG_EVAL_DUMMY, TG_EVAL_HASH
SYMM_OFF, SYMM_HASHED = TG_SYMM_OFF, TG_SYMM_HASHED
PROOF_OFF, PROOF_ON = TG_PROOF_OFF, TG_PROOF_ON
PROVEN_WHITE, PROVEN_BLACK, PROVEN_DRAW = TG_PROVEN_WHITE, TG_PROVEN_BLACK, TG_PROVEN_DRAW  # node-record codes beside the TgResult ones
NODE_RECORD, EXAMPLE_HEADER = np.dtype(TgNodeRecord), np.dtype(TgExampleHeader)


class TgError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"takgpu error {code}: {msg}")
        self.code = code


def example_means(sums):
    """The means tg_eval_examples' sums stand for (a dict of TgExampleMetrics' fields, possibly added up over calls or ranks):
    loss_p, loss_z, kl = loss_p - target entropy, top1, value_sign = sign_ok / decided (nan without decided positions)."""
    n = sums["positions"]
    nan = float("nan")
    return {"loss_p": sums["loss_p"] / n if n else nan, "loss_z": sums["loss_z"] / n if n else nan,
            "kl": (sums["loss_p"] - sums["target_entropy"]) / n if n else nan, "top1": sums["top1"] / n if n else nan,
            "value_sign": sums["sign_ok"] / sums["decided"] if sums["decided"] else nan}


def _symmetry_mode(mode):
    if isinstance(mode, str):
        if mode not in ("off", "hashed"):
            raise ValueError(f"symmetry must be 'off' or 'hashed', not {mode!r}")
        return SYMM_HASHED if mode == "hashed" else SYMM_OFF
    return int(mode)


STATUS_WHITE, STATUS_BLACK, STATUS_DRAW, STATUS_UNKNOWN = 0, 1, 2, 3
_STATUS_OF_CODE = np.array([3, 0, 0, 1, 1, 2, 2, 3, 0, 1, 2, 3, 3, 3, 3, 3], np.uint8)


def node_status(codes):
    """STATUS_* of result codes (TgNodeRecord.result, Engine.search_proof): white for a white win or TG_PROVEN_WHITE, black
    likewise, draw for both draws and TG_PROVEN_DRAW, unknown otherwise (include/takgpu.h)"""
    return _STATUS_OF_CODE[np.asarray(codes, np.int64) & 15]


def _proof_mode(mode):
    if isinstance(mode, str):
        if mode not in ("off", "on"):
            raise ValueError(f"proof must be 'off' or 'on', not {mode!r}")
        return PROOF_ON if mode == "on" else PROOF_OFF
    return int(mode)  # (True / False too)


def device_to_host(d_ptr, count, stream=None):
    """`count` floats of device memory as a numpy array (after synchronising `stream`); HIP runtime through the
    library's own dependency (no torch involved)."""
    lib = load_library()
    if stream is not None:
        rc = lib.hipStreamSynchronize(C.c_void_p(stream))
        assert rc == 0, f"hipStreamSynchronize: {rc}"
    out = np.empty(count, np.float32)
    rc = lib.hipMemcpy(_p(out), C.c_void_p(d_ptr), C.c_size_t(count * 4), 2)  # hipMemcpyDeviceToHost
    assert rc == 0, f"hipMemcpy D2H: {rc}"
    return out


def host_to_device(d_ptr, array):
    a = np.ascontiguousarray(array, np.float32)
    rc = load_library().hipMemcpy(C.c_void_p(d_ptr), _p(a), C.c_size_t(a.size * 4), 1)  # hipMemcpyHostToDevice
    assert rc == 0, f"hipMemcpy H2D: {rc}"


def build_library():
    """Compile the HIP sources for gfx950 into tak_amd/libtakgpu.so (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc"), "-j4"], check=True)


_lib = None


def load_library():
    """Load libtakgpu.so.  Raises (never falls back) if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} is missing: build it with tak_amd.build_library() / __graft_entry__.build()")
        _lib = abi.declare(C.CDLL(LIB_PATH))  # the header's restype and argtypes on every entry point; a missing export raises
    return _lib


def state_bytes(n):
    return 256 if n <= 5 else 384


def input_channels(n):
    return int(load_library().tg_input_channels(n))


def policy_size(n, head):
    return int(load_library().tg_policy_size(n, head))


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _check(rc, length=False):
    """anything but TG_OK → TgError with tg_last_error's message; length=True: the tg_format_* functions, which return a text
    length ≥ 0 or a negative TgStatus"""
    if rc < 0 or (rc and not length):
        raise TgError(rc, load_library().tg_last_error().decode())
    return rc


# ---- text formats (host only; no GPU needed): PTN, TPS, example lines of alpha-tak/src/example.rs:81-133 ----
def format_move(n, code):
    buf = C.create_string_buffer(32)
    _check(load_library().tg_format_move(n, int(code), buf, 32), length=True)
    return buf.value.decode()


def parse_move(n, text):
    out = C.c_uint16(0)
    _check(load_library().tg_parse_move(n, text.encode(), C.byref(out)))
    return out.value


def format_tps(n, state):
    st = np.ascontiguousarray(state, np.uint8)
    buf = C.create_string_buffer(2048)
    _check(load_library().tg_format_tps(n, _p(st), buf, 2048), length=True)
    return buf.value.decode()


def parse_tps(n, text):
    st = np.zeros(state_bytes(n), np.uint8)
    _check(load_library().tg_parse_tps(n, text.encode(), _p(st)))
    return st


def format_example(n, state, moves, visits, result):
    st = np.ascontiguousarray(state, np.uint8)
    mv = np.ascontiguousarray(moves, np.uint16)
    vs = np.ascontiguousarray(visits, np.uint32)
    buf = C.create_string_buffer(1 << 14)
    _check(load_library().tg_format_example(n, _p(st), mv.size, _p(mv), _p(vs), float(result), buf, 1 << 14), length=True)
    return buf.value.decode()


def parse_example(n, line):
    st = np.zeros(state_bytes(n), np.uint8)
    mv = np.zeros(TG_MAX_MOVES, np.uint16)
    vs = np.zeros(TG_MAX_MOVES, np.uint32)
    k = C.c_int32(0)
    res = C.c_float(0)
    _check(load_library().tg_parse_example(n, line.encode(), _p(st), TG_MAX_MOVES, _p(mv), _p(vs), C.byref(k), C.byref(res)))
    return st, mv[: k.value].copy(), vs[: k.value].copy(), res.value


def read_examples(n, paths):
    """Load `.data` example files as train/src/main.rs:69-80 does (one Example per line, alpha-tak/src/example.rs:100-133)
    → (states [k, bytes], n_moves [k], moves [k, TG_MAX_MOVES], visits [k, TG_MAX_MOVES], results [k]): the layout tg_train takes."""
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    rows = []
    for path in paths:
        with open(path) as f:
            for line in f.read().split("\n"):
                if line.strip():
                    rows.append(parse_example(n, line))
    k = len(rows)
    states = np.zeros((k, state_bytes(n)), np.uint8)
    n_moves = np.zeros(k, np.int32)
    moves = np.zeros((k, TG_MAX_MOVES), np.uint16)
    visits = np.zeros((k, TG_MAX_MOVES), np.uint32)
    results = np.zeros(k, np.float32)
    for i, (st, mv, vs, res) in enumerate(rows):
        states[i], n_moves[i], results[i] = st, len(mv), res
        moves[i, : len(mv)], visits[i, : len(mv)] = mv, vs
    return states, n_moves, moves, visits, results


def comm_unique_id():
    """ncclGetUniqueId on this rank (128 bytes); broadcast it to the other ranks with any host transport."""
    uid = np.zeros(128, np.uint8)
    _check(load_library().tg_comm_unique_id(_p(uid)))
    return uid.tobytes()


def debug_switches():
    """the TG_* A/B switches that are ON in this process's environment, as the library reads them → ["NAME=value", …];
    [] on a measured run (tg_debug_switches; needs no GPU)"""
    buf = C.create_string_buffer(4096)
    n = load_library().tg_debug_switches(buf, 4096)
    out = buf.value.decode().split()
    assert n == len(out), (n, out)
    return out


def train_order(seed, n):
    """the permutation tg_train(seed) visits n examples in (tg_train_order)"""
    order = np.zeros(n, np.int32)
    _check(load_library().tg_train_order(seed, n, _p(order)))
    return order


def pit(new, old, pairs=128, rollouts=50, batch=16, idle_rollouts=1, random_plies=2, komi=2, max_plies=0, arena_nodes=0, seed=0,
        symmetry=None):
    """`pit(new, old)` of train/src/pit.rs on two engines (one per weight set) → dict(wins, losses, draws, win_rate, …; the
    ref_* entries are the counts with the reference's early exit, pit.rs:20-23, applied);
    `rollouts` iterations of `batch` virtual rollouts per move (ROLLOUTS × BATCH_SIZE); 2·pairs·batch ≤ max_batch
    symmetry: SYMM_OFF / SYMM_HASHED (or "off" / "hashed") for both engines' searches of this match; None = each engine's own"""
    if symmetry is not None:
        new.search_set_symmetry(symmetry)
        old.search_set_symmetry(symmetry)
    cfg = TgPitConfig(pairs, rollouts, idle_rollouts, random_plies, komi, max_plies, arena_nodes, batch, seed)
    res = TgPitResult()
    _check(load_library().tg_pit(new.h, old.h, C.byref(cfg), C.byref(res)))
    return res.as_dict()


def tensor_shapes(n, res_blocks, filters, policy_head):
    """{ABI tensor name: shape} in the creation order of net5.rs:29-62 / net6.rs:29-57 (tch layouts, include/takgpu.h)."""
    F, cin, P = filters, input_channels(n), policy_size(n, policy_head)
    out = {}

    def conv(name, o, i):
        out[name + ".weight"], out[name + ".bias"] = (o, i, 3, 3), (o,)

    def bn(name):
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            out[f"{name}.{leaf}"] = (F,)

    conv("conv0", F, cin)
    bn("bn0")
    for i in range(res_blocks):
        conv(f"res{i}.conv1", F, F)
        conv(f"res{i}.conv2", F, F)
        bn(f"res{i}.bn1")
        bn(f"res{i}.bn2")
    if policy_head == HEAD_FC5:
        out["policy.weight"], out["policy.bias"] = (P, F * n * n), (P,)
    else:
        conv("policy", P // (n * n), F)
    out["value.weight"], out["value.bias"] = (1, F * n * n), (1,)
    return out


def _mask(active):
    return np.ascontiguousarray(active, np.uint8) if active is not None else None


class Engine:
    """One engine per GPU (reference: one `NET` + the statics of alpha-tak/src/lib.rs:21-23)."""

    def __init__(self, board_size=5, res_blocks=6, filters=64, policy_head=None, evaluator=EVAL_RESNET, max_batch=4096,
                 device=0):
        self.lib = load_library()
        if policy_head is None:
            policy_head = HEAD_FC5 if board_size == 5 else HEAD_CONV
        self.n = board_size
        self.head = policy_head
        self.max_batch = max_batch
        self.cfg = TgConfig(TG_ABI_VERSION, device, board_size, res_blocks, filters, policy_head, evaluator, max_batch)
        self.h = C.c_void_p(None)
        self._check(self.lib.tg_engine_create(C.byref(self.cfg), C.byref(self.h)))
        self.sb = state_bytes(board_size)
        self.cin = input_channels(board_size)
        self.psize = policy_size(board_size, policy_head)
        self.games = 0

    def device_info(self):
        """the card this engine runs on as the HIP runtime names it: {hip_device, pci_bus_id, name, arch, cu_count, …}"""
        info = TgDeviceInfo()
        self._check(self.lib.tg_device_info(self.h, C.byref(info)))
        return info.as_dict()

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.lib.tg_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    _check = staticmethod(_check)

    def _states(self, states):
        states = np.ascontiguousarray(states, np.uint8).reshape(-1, self.sb)
        return states, states.shape[0]

    def sync(self):
        self._check(self.lib.tg_sync(self.h))

    @property
    def stream(self):
        return self.lib.tg_stream(self.h)

    # ---- Game::{possible_moves, play, result}, game_repr, move_index -------------------------------
    def movegen(self, states):
        states, k = self._states(states)
        moves = np.zeros((k, TG_MAX_MOVES), np.uint16)
        counts = np.zeros(k, np.int32)
        self._check(self.lib.tg_movegen(self.h, k, _p(states), _p(moves), _p(counts)))
        return moves, counts

    def play(self, states, moves, check=False):
        states, k = self._states(states)
        states = states.copy()
        moves = np.ascontiguousarray(moves, np.uint16).reshape(k)
        status = np.zeros(k, np.uint8)
        rc = self.lib.tg_play(self.h, k, _p(states), _p(moves), _p(status))
        if rc != 0 and (check or rc != -8):
            self._check(rc)
        return states, status

    def result(self, states):
        states, k = self._states(states)
        out = np.zeros(k, np.uint8)
        self._check(self.lib.tg_result(self.h, k, _p(states), _p(out)))
        return out

    def encode(self, states):
        states, k = self._states(states)
        out = np.zeros((k, self.cin, self.n, self.n), np.float32)
        self._check(self.lib.tg_encode(self.h, k, _p(states), _p(out)))
        return out

    def move_index(self, moves):
        moves = np.ascontiguousarray(moves, np.uint16).ravel()
        out = np.zeros(moves.size, np.int32)
        self._check(self.lib.tg_move_index(self.h, moves.size, _p(moves), _p(out)))
        return out

    def augment_examples(self, states, n_moves, moves, visits):
        """Example::to_tensors: 8 symmetric states and policy targets per example."""
        states, k = self._states(states)
        n_moves = np.ascontiguousarray(n_moves, np.int32)
        moves = np.ascontiguousarray(moves, np.uint16).reshape(k, TG_MAX_MOVES)
        visits = np.ascontiguousarray(visits, np.uint32).reshape(k, TG_MAX_MOVES)
        out = np.zeros((k * 8, self.sb), np.uint8)
        pi = np.zeros((k * 8, self.psize), np.float32)
        self._check(self.lib.tg_augment_examples(self.h, k, _p(states), _p(n_moves), _p(moves), _p(visits), _p(out), _p(pi)))
        return out, pi

    # ---- training step (Network::train / train_inner, alpha-tak/src/model/network.rs:37-97) ----
    def train_create(self, learning_rate=1e-4, weight_decay=1e-4, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=0.1,
                     bn_eps=1e-5, chunk_size=500, chunks_in_step=20):
        cfg = TgTrainConfig(learning_rate, weight_decay, beta1, beta2, eps, bn_momentum, bn_eps, chunk_size, chunks_in_step, 0)
        self._check(self.lib.tg_train_create(self.h, C.byref(cfg)))
        self.chunk_size = chunk_size

    def _examples(self, states, n_moves, moves, visits, results):
        states, k = self._states(states)
        n_moves = np.ascontiguousarray(n_moves, np.int32)
        moves = np.ascontiguousarray(moves, np.uint16).reshape(k, TG_MAX_MOVES)
        visits = np.ascontiguousarray(visits, np.uint32).reshape(k, TG_MAX_MOVES)
        results = np.ascontiguousarray(results, np.float32).reshape(k)
        return states, k, n_moves, moves, visits, results

    def train_chunk(self, states, n_moves, moves, visits, results):
        """train_inner on one chunk → (loss_p, loss_z, stepped)"""
        states, k, n_moves, moves, visits, results = self._examples(states, n_moves, moves, visits, results)
        lp, lz, did = C.c_float(0), C.c_float(0), C.c_int32(0)
        self._check(self.lib.tg_train_chunk(self.h, k, _p(states), _p(n_moves), _p(moves), _p(visits), _p(results),
                                            C.byref(lp), C.byref(lz), C.byref(did)))
        return lp.value, lz.value, bool(did.value)

    def train(self, states, n_moves, moves, visits, results, seed=0):
        """Network::train over a set of examples → (mean loss_p, mean loss_z, optimiser steps)"""
        states, k, n_moves, moves, visits, results = self._examples(states, n_moves, moves, visits, results)
        lp, lz, steps = C.c_float(0), C.c_float(0), C.c_int32(0)
        self._check(self.lib.tg_train(self.h, k, _p(states), _p(n_moves), _p(moves), _p(visits), _p(results), seed,
                                      C.byref(lp), C.byref(lz), C.byref(steps)))
        return lp.value, lz.value, steps.value

    def train_step(self):
        self._check(self.lib.tg_train_step(self.h))

    def train_forward(self, states):
        """forward_training: (log_softmax policy, eval) with BatchNorm on the batch statistics"""
        states, k = self._states(states)
        logp = np.zeros((k, self.psize), np.float32)
        ev = np.zeros(k, np.float32)
        self._check(self.lib.tg_train_forward(self.h, k, _p(states), _p(logp), _p(ev)))
        return logp, ev

    def train_get_tensor(self, name, shape):
        out = np.zeros(shape, np.float32)
        self._check(self.lib.tg_train_get_tensor(self.h, name.encode(), _p(out), out.size))
        return out

    def train_get_grad(self, name, shape):
        out = np.zeros(shape, np.float32)
        self._check(self.lib.tg_train_get_grad(self.h, name.encode(), _p(out), out.size))
        return out

    def train_debug_capture(self, layer):
        """keep dy / dz / dx of conv layer `layer` in the backward pass of the next chunks (layer < 0: stop)"""
        self._check(self.lib.tg_train_debug_capture(self.h, int(layer)))

    def train_debug_read(self, what, layer, shape):
        """an intermediate tensor of the last training chunk / forward (include/takgpu.h tg_train_debug_read)"""
        out = np.zeros(shape, np.float32)
        self._check(self.lib.tg_train_debug_read(self.h, what.encode(), int(layer), _p(out), out.size))
        return out

    def train_commit(self):
        self._check(self.lib.tg_train_commit(self.h))

    def evaluate_examples(self, states, n_moves, moves, visits, results, symmetries=False, rows=False):
        """tg_eval_examples: the losses of the deployed (folded-BatchNorm, running statistics) network on examples it may never
        have been trained on.  Returns a dict: the means loss_p, loss_z, kl, top1, value_sign (example_means), "sums" (the raw
        TgExampleMetrics fields, which add over calls and ranks) and, with rows=True, "rows": positions x 4 float32
        (loss_p, loss_z, top1, v), position 8 i + s with symmetries."""
        states, k, n_moves, moves, visits, results = self._examples(states, n_moves, moves, visits, results)
        sums = TgExampleMetrics()
        out = np.zeros((k * (8 if symmetries else 1), 4), np.float32) if rows else None
        self._check(self.lib.tg_eval_examples(self.h, k, _p(states), _p(n_moves), _p(moves), _p(visits), _p(results),
                                              int(symmetries), C.byref(sums), _p(out) if rows else None))
        res = example_means(sums.as_dict())
        res["sums"] = sums.as_dict()
        if rows:
            res["rows"] = out
        return res

    def train_set_allreduce(self, fn, world):
        """Route the gradient / BatchNorm-statistics reduction through fn(d_ptr, count, stream) -> 0 | error instead of
        RCCL (tg_train_set_allreduce).  fn must leave the SUM over all `world` ranks in the device buffer.  None removes it."""
        if fn is None:
            self._allreduce_cb = None
            self._check(self.lib.tg_train_set_allreduce(self.h, None, None, 1))
            return

        def cb(ctx, d_buf, count, stream):
            try:
                return int(fn(d_buf, count, stream) or 0)
            except Exception:  # an exception must not unwind through the C caller
                import traceback

                traceback.print_exc()
                return 1

        self._allreduce_cb = ALLREDUCE_FN(cb)  # kept alive as long as the engine uses it
        self._check(self.lib.tg_train_set_allreduce(self.h, self._allreduce_cb, None, int(world)))

    def train_grad_buffer(self):
        """(device address, float count) of the flat gradient buffer"""
        ptr, cnt = C.c_void_p(0), C.c_size_t(0)
        self._check(self.lib.tg_train_grad_buffer(self.h, C.byref(ptr), C.byref(cnt)))
        return ptr.value, cnt.value

    def train_comm_stats(self):
        """(total milliseconds, count) of the gradient all-reduces issued by optimiser steps so far (HIP events on the engine stream)"""
        ms, cnt = C.c_double(0), C.c_int64(0)
        self._check(self.lib.tg_train_comm_stats(self.h, C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def train_comm_info(self):
        """what is attached to the optimiser step's reduction, as the library sees it: ncclCommCount / ncclCommUserRank of the
        communicator, ncclGetVersion, the file ncclAllReduce was bound from, whether that copy was already mapped"""
        info = TgCommInfo()
        self._check(self.lib.tg_train_comm_info(self.h, C.byref(info)))
        return info.as_dict()

    def train_comm_preflight(self):
        """one float summed over the ranks through the optimiser step's reduction, before any training work is enqueued →
        wall-clock milliseconds of the round trip (0.0 on a single-rank trainer); raises if the sum is not world_size"""
        ms = C.c_double(0)
        self._check(self.lib.tg_train_comm_preflight(self.h, C.byref(ms)))
        return ms.value

    def train_comm_init(self, rank, world, unique_id):
        uid = np.frombuffer(bytes(unique_id), np.uint8).copy()
        assert uid.size == 128
        self._check(self.lib.tg_train_comm_init(self.h, rank, world, _p(uid)))

    def perft(self, states, depth):
        states, k = self._states(states)
        out = np.zeros(k, np.uint64)
        self._check(self.lib.tg_perft(self.h, k, _p(states), depth, _p(out)))
        return out

    # ---- Network<N> -------------------------------------------------------------------------------
    def set_tensor(self, name, array):
        a = np.ascontiguousarray(array, np.float32)
        self._check(self.lib.tg_net_set_tensor(self.h, name.encode(), _p(a), a.size))

    def set_precision(self, precision):
        """"f32" (exact, default) or "bf16x3" (split-bf16 tower); takes effect at the next load_state_dict / finalize"""
        self._check(self.lib.tg_net_set_precision(self.h, {"f32": 0, "bf16x3": 1}[precision]))

    def init_random(self, seed=0, finalize=True):
        """Network::default(): tch's default initialisers drawn from Philox(seed) (tg_net_init_random)."""
        self._check(self.lib.tg_net_init_random(self.h, seed))
        if finalize:
            self._check(self.lib.tg_net_finalize(self.h))

    def get_tensor(self, name, shape):
        """the tensor as last set / initialised / committed (tg_net_get_tensor) — what Network::save writes"""
        out = np.zeros(shape, np.float32)
        self._check(self.lib.tg_net_get_tensor(self.h, name.encode(), _p(out), out.size))
        return out

    def state_dict(self):
        """{name: array} of every tensor as last set / initialised / committed (Network::save's content)"""
        return {k: self.get_tensor(k, shp) for k, shp in tensor_shapes(self.n, self.cfg.res_blocks, self.cfg.filters, self.head).items()}

    def load_state_dict(self, tensors):
        """tensors: {name: array} with the names of include/takgpu.h (tch layouts)."""
        for k, v in tensors.items():
            self.set_tensor(k, np.asarray(v, np.float32))
        self._check(self.lib.tg_net_finalize(self.h))

    def policy_eval(self, states, symmetries=None):
        """Network::policy_eval: states → (policy [k, P] softmax, eval [k] tanh).
        symmetries: a mask of dihedral images (bit s = image s of tg_augment_examples' order, 0xFF = all eight) → the mean of
        the network's output over them, mapped back to each state's own orientation (tg_policy_eval_symm); None = the plain call"""
        states, k = self._states(states)
        policy = np.zeros((k, self.psize), np.float32)
        ev = np.zeros(k, np.float32)
        if symmetries is None:
            self._check(self.lib.tg_policy_eval(self.h, k, _p(states), _p(policy), _p(ev)))
        else:
            self._check(self.lib.tg_policy_eval_symm(self.h, k, _p(states), int(symmetries), _p(policy), _p(ev)))
        return policy, ev

    def policy_eval_symm_dev(self, n, d_states, mask, d_policy, d_eval):
        self._check(self.lib.tg_policy_eval_symm_dev(self.h, n, d_states, int(mask), d_policy, d_eval))

    def symm_perm(self):
        """the device's policy permutation tables [8, P] (tg_symm_perm_read): perm[s, j] = slot of the image under s of slot j's move"""
        perm = np.zeros((8, self.psize), np.int32)
        self._check(self.lib.tg_symm_perm_read(self.h, _p(perm)))
        return perm

    def search_set_symmetry(self, mode):
        """tg_search_set_symmetry: SYMM_OFF / SYMM_HASHED (or "off" / "hashed") for the current search or self-play object"""
        self._check(self.lib.tg_search_set_symmetry(self.h, _symmetry_mode(mode)))

    def search_get_symmetry(self):
        """(mode, leaves sent to the network under a non-identity image since the engine was created); synchronises"""
        mode, count = C.c_int(0), C.c_uint64(0)
        self._check(self.lib.tg_search_get_symmetry(self.h, C.byref(mode), C.byref(count)))
        return mode.value, count.value

    def search_set_proof(self, mode):
        """tg_search_set_proof: PROOF_OFF / PROOF_ON (or "off" / "on", False / True) for the current search or self-play object"""
        self._check(self.lib.tg_search_set_proof(self.h, _proof_mode(mode)))

    def search_get_proof(self):
        """(mode, nodes proven, rollouts that ended on a proven node) since the search was created; synchronises"""
        mode, a, b = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.tg_search_get_proof(self.h, C.byref(mode), C.byref(a), C.byref(b)))
        return mode.value, a.value, b.value

    def search_proof(self):
        """tg_search_proof: dict(root_status [games], child_status [games, TG_MAX_MOVES], counts [games]) — the result code of every
        root and of its children in possible_moves order (0, a TgResult or a TG_PROVEN_* code; node_status maps them)"""
        g = self.games
        o = dict(root_status=np.zeros(g, np.uint8), child_status=np.zeros((g, TG_MAX_MOVES), np.uint8), counts=np.zeros(g, np.int32))
        self._check(self.lib.tg_search_proof(self.h, _p(o["root_status"]), _p(o["child_status"]), _p(o["counts"])))
        return o

    def forward_mcts(self, planes):
        planes = np.ascontiguousarray(planes, np.float32).reshape(-1, self.cin, self.n, self.n)
        k = planes.shape[0]
        policy = np.zeros((k, self.psize), np.float32)
        ev = np.zeros(k, np.float32)
        self._check(self.lib.tg_forward_mcts(self.h, k, _p(planes), _p(policy), _p(ev)))
        return policy, ev

    def policy_eval_dev(self, n, d_states, d_policy, d_eval):
        self._check(self.lib.tg_policy_eval_dev(self.h, n, d_states, d_policy, d_eval))

    # ---- Node / search ----------------------------------------------------------------------------
    def search_create(self, games, arena_nodes=1 << 16, base=500.0, init=4.0, seed=0, slot_base=0, batch=1, visit_limit=0, symmetry=None,
                      proof=None):
        """batch: virtual rollouts per tree and iteration (Player's batching); games * batch <= max_batch
        proof: PROOF_ON / "on" / True = proven values in the tree (search_set_proof); None = off
        symmetry: SYMM_HASHED / "hashed" = one hashed dihedral image per evaluated leaf (search_set_symmetry); None = off"""
        cfg = TgSearchConfig(games, arena_nodes, base, init, seed, slot_base, batch, visit_limit, 0)
        self._check(self.lib.tg_search_create(self.h, C.byref(cfg)))
        self.games = games
        if symmetry is not None and _symmetry_mode(symmetry) != SYMM_OFF:
            self.search_set_symmetry(symmetry)
        if proof is not None and _proof_mode(proof) != PROOF_OFF:
            self.search_set_proof(proof)

    def search_reset(self, states):
        states, k = self._states(states)
        assert k == self.games
        self._check(self.lib.tg_search_reset(self.h, _p(states)))

    def search_run(self, iters, active=None):
        self._check(self.lib.tg_search_run(self.h, iters, _p(_mask(active))))

    def search_apply_dirichlet(self, alpha, ratio, active=None):
        self._check(self.lib.tg_search_apply_dirichlet(self.h, alpha, ratio, _p(_mask(active))))

    def search_apply_noise(self, noise, ratio, active=None):
        noise = np.ascontiguousarray(noise, np.float32).reshape(self.games, TG_MAX_MOVES)
        self._check(self.lib.tg_search_apply_noise(self.h, _p(noise), ratio, _p(_mask(active))))

    def search_root(self):
        g = self.games
        moves = np.zeros((g, TG_MAX_MOVES), np.uint16)
        visits = np.zeros((g, TG_MAX_MOVES), np.uint32)
        prior = np.zeros((g, TG_MAX_MOVES), np.float32)
        q = np.zeros((g, TG_MAX_MOVES), np.float32)
        counts = np.zeros(g, np.int32)
        rv = np.zeros(g, np.uint32)
        rq = np.zeros(g, np.float32)
        self._check(self.lib.tg_search_root(self.h, _p(moves), _p(visits), _p(prior), _p(q), _p(counts), _p(rv), _p(rq)))
        return dict(moves=moves, visits=visits, prior=prior, q=q, counts=counts, root_visits=rv, root_q=rq)

    def search_play(self, moves, active=None):
        moves = np.ascontiguousarray(moves, np.uint16).reshape(self.games)
        self._check(self.lib.tg_search_play(self.h, _p(moves), _p(_mask(active))))

    def search_states(self):
        out = np.zeros((self.games, self.sb), np.uint8)
        self._check(self.lib.tg_search_states(self.h, _p(out)))
        return out

    def search_dump(self, game, capacity=1 << 20):
        rec = np.zeros(capacity, NODE_RECORD)
        nrec = C.c_size_t(0)
        self._check(self.lib.tg_search_dump(self.h, game, _p(rec), capacity, C.byref(nrec)))
        return rec[: nrec.value].copy()

    def search_debug(self, depth=10, top_k=TG_MAX_MOVES):
        """Node::debug(depth) of every root (tg_search_debug): children sorted by visits (ties: higher child index first), eval, and
        the continuations of the first top_k sorted children.  Arrays are zero past counts / cont_len."""
        g = self.games
        moves = np.zeros((g, TG_MAX_MOVES), np.uint16)
        visits = np.zeros((g, TG_MAX_MOVES), np.uint32)
        reward = np.zeros((g, TG_MAX_MOVES), np.float32)
        policy = np.zeros((g, TG_MAX_MOVES), np.float32)
        counts = np.zeros(g, np.int32)
        ev = np.zeros(g, np.float32)
        k, d = max(int(top_k), 0), max(int(depth), 0)
        cont_moves = np.zeros((g, k, d), np.uint16)
        cont_visits = np.zeros((g, k, d), np.uint32)
        cont_len = np.zeros((g, k), np.int32)
        self._check(self.lib.tg_search_debug(self.h, int(depth), int(top_k), _p(moves), _p(visits), _p(reward), _p(policy), _p(counts),
                                             _p(ev), _p(cont_moves), _p(cont_visits), _p(cont_len)))
        return dict(moves=moves, visits=visits, reward=reward, policy=policy, counts=counts, eval=ev, cont_moves=cont_moves,
                    cont_visits=cont_visits, cont_len=cont_len)

    # ---- forced wins (tg_solve / tg_search_solve) ----------------------------------------------------
    def _solve_out(self, k):
        return dict(value=np.zeros(k, np.int8), best=np.zeros(k, np.uint16), counts=np.zeros(k, np.int32),
                    moves=np.zeros((k, TG_MAX_MOVES), np.uint16), move_values=np.zeros((k, TG_MAX_MOVES), np.int8),
                    budget_hit=np.zeros(k, np.uint8), nodes=np.zeros(k, np.uint64))

    @staticmethod
    def _solve_flags(all_moves, road_only):
        return (TG_SOLVE_ALL_MOVES if all_moves else 0) | (TG_SOLVE_ROAD_ONLY if road_only else 0)

    def solve(self, states, depth, all_moves=False, node_budget=0, flags=None, road_only=False):
        """Exact forced wins within `depth` plies of every position (definitions: include/takgpu.h).  Returns a dict of arrays:
        value / best / counts / budget_hit / nodes [k], moves / move_values [k, TG_MAX_MOVES] (zero past counts).
        all_moves: deepen every position to `depth` and complete the move table instead of stopping at the deciding level;
        road_only: only roads win (TG_SOLVE_ROAD_ONLY, the tinuë), a move that ends the game any other way proves nothing;
        node_budget: positions one (position, root move, level) may create, 0 = the library's default;
        flags overrides all_moves and road_only."""
        states, k = self._states(states)
        cfg = TgSolveConfig(int(depth), self._solve_flags(all_moves, road_only) if flags is None else int(flags), int(node_budget))
        o = self._solve_out(k)
        self._check(self.lib.tg_solve(self.h, k, _p(states), C.byref(cfg), _p(o["value"]), _p(o["best"]), _p(o["counts"]), _p(o["moves"]),
                                      _p(o["move_values"]), _p(o["budget_hit"]), _p(o["nodes"])))
        return o

    def search_solve(self, depth, active=None, all_moves=False, node_budget=0, road_only=False, flags=None):
        """Engine.solve on the current roots of the live search / self-play object, in place on the device; games outside
        `active` and dead games give zero rows.  The trees are not touched."""
        cfg = TgSolveConfig(int(depth), self._solve_flags(all_moves, road_only) if flags is None else int(flags), int(node_budget))
        o = self._solve_out(self.games)
        self._check(self.lib.tg_search_solve(self.h, C.byref(cfg), _p(_mask(active)), _p(o["value"]), _p(o["best"]), _p(o["counts"]),
                                             _p(o["moves"]), _p(o["move_values"]), _p(o["budget_hit"]), _p(o["nodes"])))
        return o

    def search_counters(self):
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.tg_search_counters(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- measurement hooks ----------------------------------------------------------------------
    def search_pool(self):
        """node-pool occupancy: dict(total, in_use, peak) in nodes"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.tg_search_pool(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"total": a.value, "in_use": b.value, "peak": c.value}

    def profile_enable(self, sample_every):
        self._check(self.lib.tg_profile_enable(self.h, sample_every))

    def profile_read(self):
        p = TgProfile()
        self._check(self.lib.tg_profile_read(self.h, C.byref(p)))
        return p.as_dict()

    def board_pass_bench(self, states, moves, reps=10):
        """Fused play → result → movegen-count → encode pass on device-resident inputs (micro-benchmark)."""
        states, k = self._states(states)
        moves = np.ascontiguousarray(moves, np.uint16).reshape(k)
        ms = C.c_double(0)
        out_states = np.zeros_like(states)
        res = np.zeros(k, np.uint8)
        cnt = np.zeros(k, np.int32)
        self._check(self.lib.tg_board_pass_bench(self.h, k, _p(states), _p(moves), reps, C.byref(ms), _p(out_states), _p(res), _p(cnt)))
        return ms.value, out_states, res, cnt

    # ---- self_play_parallel ------------------------------------------------------------------------
    def selfplay_create(self, games, arena_nodes=0, base=500.0, init=4.0, seed=0, rollouts=400, noise_plies=80,
                        exploit_plies=40, noise_alpha=0.2, noise_ratio=0.3, komi=2, total_games=0, max_examples=1 << 16,
                        slot_base=0, max_game_plies=0, visit_limit=0, batch=1, boost_plies=0, boost_factor=1, symmetry=None,
                        proof=None):
        """proof: PROOF_ON / "on" / True = proven values in the tree and the proof-aware pick (search_set_proof); None = off
        batch: virtual rollouts per game and iteration (Player's batching; the reference's self_play uses 32): `rollouts`
        iterations of `batch` rollouts per move, games * batch leaves per network call, games * batch <= max_batch
        boost_plies, boost_factor: the rollout schedule (QUAD_ROLLOUT_PLIES; the reference's self_play uses 10 and 4): a move
        of a game whose ply < boost_plies gets boost_factor * rollouts iterations.  0 / 1 = off: the setter is not called"""
        scfg = TgSearchConfig(games, arena_nodes, base, init, seed, slot_base, 0, visit_limit, 0)
        cfg = TgSelfPlayConfig(rollouts, noise_plies, exploit_plies, noise_alpha, noise_ratio, komi, total_games, max_examples,
                               max_game_plies, batch)
        self._check(self.lib.tg_selfplay_create(self.h, C.byref(scfg), C.byref(cfg)))
        self.games = games
        if boost_plies != 0 and boost_factor != 1:
            self.selfplay_set_schedule(boost_plies, boost_factor)
        if symmetry is not None and _symmetry_mode(symmetry) != SYMM_OFF:  # (None / off: the setter is not called)
            self.search_set_symmetry(symmetry)
        if proof is not None and _proof_mode(proof) != PROOF_OFF:
            self.search_set_proof(proof)

    def selfplay_set_schedule(self, boost_plies, boost_factor, reserved=(0, 0)):
        """tg_selfplay_set_schedule as it is: after selfplay_create, before the first selfplay_step"""
        s = TgRolloutSchedule(boost_plies, boost_factor, (C.c_int32 * 2)(*reserved))
        self._check(self.lib.tg_selfplay_set_schedule(self.h, C.byref(s)))

    def selfplay_schedule_stats(self):
        """{boosted_moves, compact_iterations, compact_leaves} since selfplay_create (synchronises)"""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.lib.tg_selfplay_schedule_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"boosted_moves": a.value, "compact_iterations": b.value, "compact_leaves": c.value}

    def selfplay_step(self, plies=1):
        self._check(self.lib.tg_selfplay_step(self.h, plies))

    def selfplay_stats(self):
        s = TgSelfPlayStats()
        self._check(self.lib.tg_selfplay_stats(self.h, C.byref(s)))
        return s.as_dict()

    def write_examples(self, path, cap=1 << 16, window=None):
        """Drain finished examples and append them to `path` in the reference's `.data` text format.
        window=(first, n): write that logical range of the example window instead (window_read; nothing is drained or removed)."""
        if window is not None:
            hdr, states, moves, visits = self.window_read(*window)
        else:
            hdr, states, moves, visits = self.selfplay_drain(cap)
        with open(path, "a") as f:
            for i in range(len(hdr)):
                k = int(hdr["n_moves"][i])
                f.write(format_example(self.n, states[i], moves[i, :k], visits[i, :k], float(hdr["result"][i])) + "\n")
        return len(hdr)

    def selfplay_drain(self, cap=4096):
        hdr = np.zeros(cap, EXAMPLE_HEADER)
        states = np.zeros((cap, self.sb), np.uint8)
        moves = np.zeros((cap, TG_MAX_MOVES), np.uint16)
        visits = np.zeros((cap, TG_MAX_MOVES), np.uint32)
        k = C.c_int32(0)
        self._check(self.lib.tg_selfplay_drain(self.h, cap, _p(hdr), _p(states), _p(moves), _p(visits), C.byref(k)))
        k = k.value
        return hdr[:k].copy(), states[:k].copy(), moves[:k].copy(), visits[:k].copy()

    # ---- the example window of training_loop (train/src/main.rs:26,56-123) on the device -----------
    def window_create(self, capacity):
        """(re)create an empty window of `capacity` examples; 0 frees it.  It outlives selfplay_create, train_create, commits and pits"""
        self._check(self.lib.tg_window_create(self.h, int(capacity)))

    def window_info(self):
        """{capacity, count, entered, evicted}: count = min(entered, capacity), counted since window_create / window_clear"""
        info = TgWindowInfo()
        self._check(self.lib.tg_window_info(self.h, C.byref(info)))
        return info.as_dict()

    def window_clear(self):
        self._check(self.lib.tg_window_clear(self.h))

    def window_absorb(self):
        """every finished example of the self-play ring -> the window, on the device, in drain's order (shares drain's cursor)
        -> how many entered"""
        k = C.c_int32(0)
        self._check(self.lib.tg_window_absorb(self.h, C.byref(k)))
        return k.value

    def window_push(self, states, n_moves, moves, visits, results, game_ids=None):
        """the same rows from the host (read_examples' layout); every example is validated first, a bad one raises and
        leaves the window untouched"""
        states, k, n_moves, moves, visits, results = self._examples(states, n_moves, moves, visits, results)
        ids = np.ascontiguousarray(game_ids, np.int32).reshape(k) if game_ids is not None else None
        self._check(self.lib.tg_window_push(self.h, k, _p(states), _p(n_moves), _p(moves), _p(visits), _p(results), _p(ids)))

    def window_read(self, first, n):
        """logical [first, first + n) of the window (0 = oldest) in selfplay_drain's layout -> (headers, states, moves, visits)"""
        rows = max(int(n), 0)
        hdr = np.zeros(rows, EXAMPLE_HEADER)
        states = np.zeros((rows, self.sb), np.uint8)
        moves = np.zeros((rows, TG_MAX_MOVES), np.uint16)
        visits = np.zeros((rows, TG_MAX_MOVES), np.uint32)
        self._check(self.lib.tg_window_read(self.h, int(first), int(n), _p(hdr), _p(states), _p(moves), _p(visits)))
        return hdr, states, moves, visits

    def window_train(self, first, count, seed=0):
        """Network::train on logical [first, first + count) of the window: bit for bit train() on those examples, oldest first
        -> (mean loss_p, mean loss_z, optimiser steps)"""
        lp, lz, steps = C.c_float(0), C.c_float(0), C.c_int32(0)
        self._check(self.lib.tg_window_train(self.h, int(first), int(count), seed, C.byref(lp), C.byref(lz), C.byref(steps)))
        return lp.value, lz.value, steps.value

    def reanalyse(self, first, count, rollouts, noise_alpha=0.0, noise_ratio=0.0):
        """tg_reanalyse: search the positions of logical window rows [first, first + count) again on the live search object
        (search_create: its games, batch, seed, symmetry and proof modes; its trees are destroyed) and write the new root visit
        counts into the rows in place, on the device -> {rows, updated, mismatched, unvisited, expansions, evals}"""
        cfg = TgReanalyseConfig(int(rollouts), float(noise_alpha), float(noise_ratio), 0)
        stats = TgReanalyseStats()
        self._check(self.lib.tg_reanalyse(self.h, int(first), int(count), C.byref(cfg), C.byref(stats)))
        return stats.as_dict()
