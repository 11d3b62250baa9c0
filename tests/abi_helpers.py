"""What the per-feature tests/test_*_abi.py files share: a script of scripts/ as a module, the parsed header, the library's
dynamic symbols, and a structure's fields as the generated Rust binding spells them.  Needs no GPU."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "takgpu.h")
LIB_RS = os.path.join(ROOT, "rust", "takgpu-sys", "src", "lib.rs")


def script(name):
    """scripts/<name>.py as a module"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        return __import__(name)
    finally:
        sys.path.pop(0)


def parsed_header():
    return script("gen_rust_sys").parse_header(HEADER)


def defined_symbols():
    """`nm -D --defined-only` of libtakgpu.so (built first if it is missing)"""
    import tak_amd

    if not os.path.exists(tak_amd.LIB_PATH):
        tak_amd.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", tak_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def rust_fields(name):
    """the field lines of `pub struct <name>` in rust/takgpu-sys/src/lib.rs, without their trailing commas"""
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct " + name + r" \{(.*?)\}", open(LIB_RS).read(), flags=re.S).group(1)
    return [ln.strip().rstrip(",") for ln in body.strip().splitlines()]
