"""include/takgpu.h, read once: the header's parser (scripts/gen_rust_sys.py writes the Rust binding from the same one) and, built
from it at import, the ctypes side of the C ABI — every structure, constant and function signature under its header name.
Nothing here is written by hand per declaration: an edit of the header is an edit of this module's contents."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "takgpu.h")


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def split_decl(decl):
    """'const float* d_buf' → ('const float*', 'd_buf', None); 'uint64_t stack[25]' → ('uint64_t', 'stack', 25)"""
    m = re.match(r"^(.*?)(\w+)\s*(?:\[(\d+)\])?$", decl.strip())
    assert m, decl
    return m.group(1).strip(), m.group(2), int(m.group(3)) if m.group(3) else None


def parse_header(path=HEADER):
    """→ dict(defines=[(name, value)], enums=[(name, [(item, value)])], structs=[(name, [(field, ctype, array)])],
    aliases=[(name, ctype)], opaque=[name], fnptrs=[(name, ret, [(ctype, argname)])], functions=[(name, ret, [(ctype, argname)])])"""
    text = strip_comments(open(path).read())
    text = re.sub(r"\bTG_API\s+", "", text)  # the export attribute of the 60-odd entry points: not part of a signature
    out = dict(defines=[], enums=[], structs=[], aliases=[], opaque=[], fnptrs=[], functions=[])
    for m in re.finditer(r"^#define\s+(TG_[A-Z0-9_]+)\s+(.+)$", text, flags=re.M):
        name, val = m.group(1), m.group(2).strip()
        if "(" in name or name.startswith("TG_META"):
            continue
        mm = re.fullmatch(r"\(?\s*(-?\d+)[uU]?\s*(?:<<\s*(\d+))?\s*\)?", val)
        if mm:
            out["defines"].append((name, int(mm.group(1)) << int(mm.group(2) or 0)))
    for m in re.finditer(r"typedef\s+enum\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        items, nxt = [], 0
        for part in m.group(2).split(","):
            part = part.strip()
            if not part:
                continue
            if "=" in part:
                k, v = [x.strip() for x in part.split("=")]
                nxt = int(v, 0)
            else:
                k = part
            items.append((k, nxt))
            nxt += 1
        out["enums"].append((m.group(1), items))
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            stmt = " ".join(stmt.split())
            if not stmt:
                continue
            first, *rest = [p.strip() for p in stmt.split(",")]
            ctype, fname, arr = split_decl(first)
            fields.append((fname, ctype, arr))
            for r in rest:  # `uint8_t a, b, c;`
                _, fname2, arr2 = split_decl(ctype + " " + r)
                fields.append((fname2, ctype, arr2))
        out["structs"].append((m.group(1), fields))
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s+\1\s*;", text):
        out["opaque"].append(m.group(1))
    for m in re.finditer(r"typedef\s+(\w+)\s+(\w+)\s*;", text):
        if m.group(1) not in ("struct", "enum"):
            out["aliases"].append((m.group(2), m.group(1)))
    for m in re.finditer(r"typedef\s+([\w\s\*]+?)\(\s*\*\s*(\w+)\s*\)\s*\((.*?)\)\s*;", text, flags=re.S):
        args = [split_decl(a)[:2] for a in " ".join(m.group(3).split()).split(",")]
        out["fnptrs"].append((m.group(2), m.group(1).strip(), args))
    body = re.sub(r"typedef\s+(enum|struct)\s+\w+\s*\{.*?\}\s*\w+\s*;", "", text, flags=re.S)
    body = re.sub(r"typedef[^;]*;", "", body)
    for m in re.finditer(r"^\s*([\w\s\*]+?)\b(tg_\w+)\s*\(([^;{}]*?)\)\s*;", body, flags=re.M | re.S):
        ret, name, args = m.group(1).strip(), m.group(2), " ".join(m.group(3).split())
        alist = [] if args in ("", "void") else [split_decl(a)[:2] for a in args.split(",")]
        out["functions"].append((name, ret, alist))
    return out


# ---- the ctypes side, built from the header at import ------------------------------------------------------------------------
if not os.path.exists(HEADER):
    raise FileNotFoundError(f"{HEADER} is missing: tak_amd builds its ctypes binding from this header and has no copy of it")
_h = parse_header()

SCALARS = {
    "int": C.c_int, "short": C.c_short, "char": C.c_char, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
    "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "uint16_t": C.c_uint16, "int32_t": C.c_int32,
    "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
}
for _name, _ctype in _h["aliases"]:  # typedef uint16_t TgMove
    SCALARS[_name] = SCALARS[_ctype]
for _name, _ in _h["enums"]:  # a C enum is passed and returned as int
    SCALARS[_name] = C.c_int


class TgStruct(C.Structure):
    """base of every `typedef struct` of the header"""

    def as_dict(self):
        """{field: Python number | str (char[N], decoded) | list (other arrays) | dict (a nested structure)} without `reserved`"""
        out = {}
        for name, _ in self._fields_:
            if name == "reserved":
                continue
            v = getattr(self, name)
            if isinstance(v, bytes):
                v = v.decode(errors="replace")
            elif isinstance(v, C.Array):
                v = list(v)
            elif isinstance(v, TgStruct):
                v = v.as_dict()
            out[name] = v
        return out


STRUCTS = {}
for _name, _fields in _h["structs"]:
    _types = [STRUCTS.get(t) or SCALARS[t] for _, t, _ in _fields]
    STRUCTS[_name] = type(_name, (TgStruct,), {"_fields_": [(f, t * arr if arr else t) for (f, _, arr), t in zip(_fields, _types)]})

CONSTANTS = dict(_h["defines"])
for _, _items in _h["enums"]:
    CONSTANTS.update(_items)


def ctype_of(ctype, value=False):
    """the ctypes type of a C parameter or return type.  One rule for pointers: `char*` is c_char_p (bytes and string buffers);
    every other data pointer, structure pointers included, and every function pointer is c_void_p — numpy arrays, byref(...),
    None, raw device addresses and CFUNCTYPE objects all arrive through them.  value=True: a return type, where void is None"""
    words = [w for w in ctype.replace("*", " * ").split() if w != "const"]
    if words == ["void"] and value:
        return None
    if "*" in words:
        return C.c_char_p if words == ["char", "*"] else C.c_void_p
    (name,) = words
    return C.c_void_p if name in FNPTRS else SCALARS[name]


FNPTRS = {}
for _name, _ret, _args in _h["fnptrs"]:
    FNPTRS[_name] = C.CFUNCTYPE(ctype_of(_ret, value=True), *[ctype_of(t) for t, _ in _args])
ALLREDUCE_FN = FNPTRS["TgAllReduceFn"]

# {entry point: (restype, argtypes)} in header order
FUNCTIONS = {name: (ctype_of(ret, value=True), [ctype_of(t) for t, _ in args]) for name, ret, args in _h["functions"]}


def declare(lib):
    """give every entry point of the header its restype and argtypes on a loaded library; one the library does not export raises"""
    for name, (restype, argtypes) in FUNCTIONS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


globals().update(STRUCTS)
globals().update(CONSTANTS)
__all__ = [*STRUCTS, *CONSTANTS, "TgStruct", "ALLREDUCE_FN"]
