"""The ctypes binding is built from include/takgpu.h at import (tak_amd/abi.py): every signature, structure and constant is
checked here against the header as the C compiler reads it, and bare Python values are converted by their declared C types.
Needs no GPU."""
import ctypes as C
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

from abi_helpers import LIB_RS, ROOT, defined_symbols, parsed_header

# written out here, not taken from the module under test
SCALARS = {"int": C.c_int, "int8_t": C.c_int8, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "TgMove": C.c_uint16, "int32_t": C.c_int32,
           "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float,
           "double": C.c_double, "char": C.c_char}
RETURNS = {"int": C.c_int, "void": None, "const char*": C.c_char_p, "void*": C.c_void_p, "size_t": C.c_size_t}
TG_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def lib():
    import tak_amd

    if not os.path.exists(tak_amd.LIB_PATH):
        tak_amd.build_library()
    return tak_amd.load_library()


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """one C program over the header: `sizeof` of every structure, `offsetof` of every field, the value of every define and
    enum item, as the compiler sees them → {"TgConfig": 32, "TgConfig.device": 4, "TG_MAX_MOVES": 512, …}"""
    h = parsed_header()
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "takgpu.h"', "int main(void) {"]
    for name, fields in h["structs"]:
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f, _, _ in fields]
    for name in [n for n, _ in h["defines"]] + [k for _, items in h["enums"] for k, _ in items]:
        lines.append(f'    printf("{name} %lld\\n", (long long){name});')
    lines += ["    return 0;", "}"]
    d = tmp_path_factory.mktemp("abi_layout")
    (d / "layout.c").write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(d / "layout.c"), "-o", str(d / "layout")],
                   check=True)
    out = subprocess.run([str(d / "layout")], capture_output=True, text=True, check=True).stdout
    return {k: int(v) for k, v in (ln.split() for ln in out.splitlines())}


def test_every_function_has_the_headers_signature(lib):
    from tak_amd import abi
    from tak_amd.engine import ABI_SYMBOLS

    h = parsed_header()
    fnptrs = {n for n, _, _ in h["fnptrs"]}
    assert len(h["functions"]) == 90
    for name, ret, args in h["functions"]:
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(args), name
        assert fn.restype is RETURNS[ret], (name, ret, fn.restype)
        for (ctype, arg), got in zip(args, fn.argtypes):
            bare = ctype.replace("const ", "")
            if bare == "char*":
                assert got is C.c_char_p, (name, arg)
            elif "*" in bare or bare in fnptrs:
                assert got is C.c_void_p, (name, arg)
            else:
                assert got is SCALARS[bare], (name, arg, ctype, got)
    declared = {name for name, _, _ in h["functions"]}
    assert declared == set(ABI_SYMBOLS) == set(abi.FUNCTIONS) and len(ABI_SYMBOLS) == len(declared)
    assert declared == defined_symbols()
    assert abi.ALLREDUCE_FN._restype_ is C.c_int and abi.ALLREDUCE_FN._argtypes_ == (C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


def test_every_structure_has_the_compilers_layout(compiled):
    from tak_amd import abi, engine

    h = parsed_header()
    assert len(h["structs"]) == 21
    for name, fields in h["structs"]:
        S = getattr(engine, name)
        assert S is getattr(abi, name) and issubclass(S, abi.TgStruct) and issubclass(S, C.Structure)
        assert [f for f, _ in S._fields_] == [f for f, _, _ in fields], name  # header order
        assert C.sizeof(S) == compiled[name], name
        for (f, ctype, arr), (_, got) in zip(fields, S._fields_):
            assert getattr(S, f).offset == compiled[f"{name}.{f}"], (name, f)
            want = SCALARS[ctype] if ctype in SCALARS else getattr(abi, ctype)
            assert got is (want * arr if arr else want), (name, f)


def test_the_two_record_dtypes_are_the_ones_spelled_out_before():
    from tak_amd import engine

    node = np.dtype([("move", "<u2"), ("n_children", "<u2"), ("visits", "<u4"), ("virtual_visits", "<u4"), ("result", "<u4"),
                     ("prior_bits", "<u4"), ("q_bits", "<u4")])
    header = np.dtype([("game_id", "<i4"), ("n_moves", "<i4"), ("result", "<f4"), ("reserved", "<i4")])
    for got, want, size in ((engine.NODE_RECORD, node, 24), (engine.EXAMPLE_HEADER, header, 16)):
        assert got == want and got.itemsize == want.itemsize == size and got.names == want.names
        assert [got.fields[f] for f in got.names] == [want.fields[f] for f in want.names]  # (dtype, offset) of every field
    assert engine.NODE_RECORD == np.dtype(engine.TgNodeRecord) and engine.EXAMPLE_HEADER == np.dtype(engine.TgExampleHeader)


def test_every_constant_has_the_compilers_value(compiled):
    import tak_amd
    from tak_amd import abi, engine

    h = parsed_header()
    names = [n for n, _ in h["defines"]] + [k for _, items in h["enums"] for k, _ in items]
    assert len(names) == len(set(names)) > 50
    for name in names:
        assert getattr(abi, name) == getattr(engine, name) == compiled[name], name
        assert type(getattr(abi, name)) is int, name
    assert "TG_SOLVE_ALL_MOVES" in names and abi.TG_SOLVE_ALL_MOVES == 1  # `1u`: a define with an unsigned suffix
    assert "pub const TG_SOLVE_ALL_MOVES: i32 = 1;" in open(LIB_RS).read()
    assert (abi.TG_ABI_VERSION, abi.TG_MAX_MOVES, abi.TG_LIMIT_VISITS, abi.TG_ERR_LIMIT) == (5, 512, 1 << 22, -9)
    # the short names the package has always exported
    assert (tak_amd.HEAD_FC5, tak_amd.HEAD_CONV, tak_amd.EVAL_RESNET, tak_amd.EVAL_DUMMY, tak_amd.EVAL_HASH) == (0, 1, 0, 1, 2)
    assert (tak_amd.SYMM_OFF, tak_amd.SYMM_HASHED, tak_amd.PROOF_OFF, tak_amd.PROOF_ON) == (0, 1, 0, 1)
    assert (tak_amd.PROVEN_WHITE, tak_amd.PROVEN_BLACK, tak_amd.PROVEN_DRAW, tak_amd.TG_MAX_MOVES) == (8, 9, 10, 512)


def test_bare_python_values_are_converted_by_their_declared_types(lib):
    import rng_ref
    import tak_amd

    # a 64-bit seed: without argtypes ctypes passes the low 32 bits of a bare int
    seed = (1 << 63) + 5
    assert rng_ref.shuffle(seed, 8) != rng_ref.shuffle(seed & 0xFFFFFFFF, 8)
    order = np.zeros(8, np.int32)
    assert lib.tg_train_order(seed, 8, order.ctypes.data) == 0
    assert order.tolist() == rng_ref.shuffle(seed, 8)
    # a bare float (an ArgumentError without argtypes), a bare size_t, bytes and a string buffer for char*
    state = tak_amd.parse_tps(5, "x5/x5/x5/x5/x5 1 1")
    moves = np.array([tak_amd.parse_move(5, "a1"), tak_amd.parse_move(5, "b2")], np.uint16)
    visits = np.array([3, 7], np.uint32)
    buf = C.create_string_buffer(1 << 14)
    length = lib.tg_format_example(5, state.ctypes.data, 2, moves.ctypes.data, visits.ctypes.data, -1.0, buf, 1 << 14)
    assert length == len(buf.value) > 0
    st, mv, vs = np.zeros(256, np.uint8), np.zeros(512, np.uint16), np.zeros(512, np.uint32)
    k, res = C.c_int32(0), C.c_float(0)
    assert lib.tg_parse_example(5, buf.value, st.ctypes.data, 512, mv.ctypes.data, vs.ctypes.data, C.byref(k), C.byref(res)) == 0
    assert k.value == 2 and res.value == -1.0 and np.array_equal(st, state)
    assert np.array_equal(mv[:2], moves) and np.array_equal(vs[:2], visits) and not mv[2:].any() and not vs[2:].any()
    # arity is checked
    with pytest.raises(TypeError):
        lib.tg_train_order(seed, 8)
    with pytest.raises(TypeError):
        lib.tg_sync()
    # None goes through every pointer kind: engine, function pointer, context, structures
    assert lib.tg_train_set_allreduce(None, None, None, 1) == TG_ERR_INVALID_ARG
    assert lib.tg_reanalyse(None, 0, 0, None, None) == TG_ERR_INVALID_ARG
    assert isinstance(lib.tg_last_error(), bytes) and lib.tg_state_bytes(6) == 384


def test_as_dict_returns_what_the_hand_written_methods_returned():
    from tak_amd import engine

    pit = engine.TgPitResult(wins=3, losses=2, draws=1, unfinished=0, plies=77, reserved=9, win_rate=0.6, ref_wins=3, ref_losses=2,
                             ref_draws=1, ref_pairs=3, ref_win_rate=0.6)
    assert pit.as_dict() == {"wins": 3, "losses": 2, "draws": 1, "unfinished": 0, "plies": 77, "win_rate": 0.6, "ref_wins": 3,
                             "ref_losses": 2, "ref_draws": 1, "ref_pairs": 3, "ref_win_rate": 0.6}
    comm = engine.TgCommInfo(attached=1, world_size=8, rank=2, nccl_count=8, nccl_rank=2, nccl_version=22105, lib_was_mapped=1,
                             reserved=5, lib_path=b"/opt/lib/librccl.so.1\xff")
    assert comm.as_dict() == {"attached": 1, "world_size": 8, "rank": 2, "nccl_count": 8, "nccl_rank": 2, "nccl_version": 22105,
                              "lib_was_mapped": 1, "lib_path": "/opt/lib/librccl.so.1�"}
    dev = engine.TgDeviceInfo(hip_device=1, cu_count=256, clock_khz=2400000, reserved=4, total_mem=288 << 30, pci_bus_id=b"0000:05:00.0",
                              name=b"AMD Instinct MI355X", arch=b"gfx950:sramecc+:xnack-")
    assert dev.as_dict() == {"hip_device": 1, "pci_bus_id": "0000:05:00.0", "name": "AMD Instinct MI355X", "arch": "gfx950:sramecc+:xnack-",
                             "cu_count": 256, "clock_khz": 2400000, "total_mem": 288 << 30}
    for d in (pit.as_dict(), comm.as_dict(), dev.as_dict()):
        assert "reserved" not in d
        assert {k: type(v) for k, v in d.items()} == {
            k: str if k in ("lib_path", "pci_bus_id", "name", "arch") else float if k.endswith("win_rate") else int for k in d}


def test_a_missing_header_fails_the_import_and_names_the_path(tmp_path):
    """the binding has no copy of the header to fall back on: tak_amd/abi.py beside no include/takgpu.h does not import"""
    (tmp_path / "pkg").mkdir()
    shutil.copy(os.path.join(ROOT, "tak_amd", "abi.py"), tmp_path / "pkg" / "abi.py")
    spec = importlib.util.spec_from_file_location("abi_without_header", tmp_path / "pkg" / "abi.py")
    with pytest.raises(FileNotFoundError) as ei:
        spec.loader.exec_module(importlib.util.module_from_spec(spec))
    assert os.path.join(str(tmp_path), "include", "takgpu.h") in str(ei.value)
