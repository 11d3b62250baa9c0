"""TgSelfPlayConfig.batch took the place of the struct's `reserved` word: same size, same offsets, and the Python binding agrees
with the header.  Needs no GPU (the C compiler checks the layout, ctypes the binding)."""
import ctypes as C
import os
import re
import subprocess

from abi_helpers import parsed_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "takgpu.h")

CTYPES = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "float": C.c_float, "uint64_t": C.c_uint64}


def _header_fields(struct):
    structs = dict(parsed_header()["structs"])
    return [(name, ctype) for name, ctype, array in structs[struct]]


def test_batch_is_where_reserved_was_and_the_size_is_unchanged(tmp_path):
    fields = _header_fields("TgSelfPlayConfig")
    assert [f for f, _ in fields] == ["rollouts", "noise_plies", "exploit_plies", "noise_alpha", "noise_ratio", "komi", "total_games",
                                      "max_examples", "max_game_plies", "batch"]
    assert fields[-1] == ("batch", "int32_t")
    # ten 4-byte words as before the field had a name: the compiler's own view of the header
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include "takgpu.h"\n'
                   "_Static_assert(sizeof(TgSelfPlayConfig) == 40, \"size\");\n"
                   "_Static_assert(offsetof(TgSelfPlayConfig, batch) == 36, \"offset\");\n"
                   "_Static_assert(offsetof(TgSelfPlayConfig, max_game_plies) == 32, \"offset\");\n"
                   "_Static_assert(TG_ABI_VERSION == 5, \"abi\");\n")
    r = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_ctypes_structure_agrees_with_the_header():
    from tak_amd import engine

    fields = _header_fields("TgSelfPlayConfig")
    assert [(f, CTYPES[t]) for f, t in fields] == list(engine.TgSelfPlayConfig._fields_)
    assert C.sizeof(engine.TgSelfPlayConfig) == 40 and engine.TgSelfPlayConfig.batch.offset == 36
    assert engine.TG_ABI_VERSION == 5
    # the keyword reaches the field: Engine.selfplay_create(..., batch=1)
    import inspect

    sig = inspect.signature(engine.Engine.selfplay_create)
    assert sig.parameters["batch"].default == 1


def test_the_search_config_documents_that_selfplay_ignores_its_batch():
    text = open(HEADER).read()
    body = re.search(r"typedef struct TgSearchConfig \{(.*?)\} TgSearchConfig;", text, flags=re.S).group(1)
    comment = re.search(r"uint32_t batch;\s*/\*(.*?)\*/", body, flags=re.S).group(1)
    assert "tg_selfplay_create" in comment and "TgSelfPlayConfig.batch" in comment
