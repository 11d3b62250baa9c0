#!/usr/bin/env python3
"""Did a change move any kernel?  Compare the device code of two source trees, kernel by kernel.

    python scripts/kernel_isa_diff.py A B [--only net_kernels.hip ...] [--jobs 8] [--show 20]

A and B are directories that hold tak_amd/csrc/, or git revisions of this repository (exported with `git archive` into a
temporary directory; `.` and paths are taken as directories first).  Every tak_amd/csrc/*.hip of each tree is compiled
device-only with that tree's Makefile FLAGS (+ --cuda-device-only --no-gpu-bundle-output -c: an AMDGPU ELF that llvm-objdump
reads), disassembled and split per symbol with addresses and encodings dropped; the kernel descriptors (VGPR / AGPR / SGPR
counts, LDS and private-segment size, ...) come from `llvm-readelf --notes`.  Per symbol one line: same / differs / only in A /
only in B; then a summary line.  Exit status 0 only if every symbol of every file is `same`.  Needs hipcc and no GPU.
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
LLVM = os.path.join(ROCM, "llvm", "bin")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# what a kernel costs to launch and to keep resident: compared beside the instruction text
DESCRIPTOR_KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size",
                   ".kernarg_segment_size", ".max_flat_workgroup_size", ".wavefront_size", ".uses_dynamic_stack")


def resolve_tree(spec, tmp):
    """A directory as it is; anything else as a git revision of this repository, exported."""
    if os.path.isdir(os.path.join(spec, "tak_amd", "csrc")):
        return os.path.abspath(spec)
    dst = tempfile.mkdtemp(prefix="tree_", dir=tmp)
    archive = subprocess.Popen(["git", "-C", REPO, "archive", spec], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    untar = subprocess.run(["tar", "-x", "-C", dst], stdin=archive.stdout, stderr=subprocess.DEVNULL)
    if archive.wait() != 0 or untar.returncode != 0:
        sys.exit(f"{spec}: neither a source tree nor a git revision")
    return dst


def makefile_flags(csrc):
    text = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:?=\s*(.*)$", text, re.M).group(1)
    arch = re.search(r"^ARCH\s*\??=\s*(\S+)", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def compile_device(csrc, name, outdir, flags):
    obj = os.path.join(outdir, name + ".o")
    r = subprocess.run([HIPCC, *flags, "--cuda-device-only", "--no-gpu-bundle-output", "-c", name, "-o", obj], cwd=csrc,
                       stderr=subprocess.PIPE, text=True)
    if r.returncode != 0:
        sys.exit(f"{csrc}/{name} does not compile:\n{r.stderr}")
    return obj


def disassembly(obj):
    """symbol → its instructions as text: no addresses, no encodings."""
    out = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", obj], check=True,
                         stdout=subprocess.PIPE, text=True).stdout
    syms, cur = {}, None
    for line in out.splitlines():
        m = re.match(r"^(?:[0-9a-f]+ )?<(.+)>:\s*$", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
            continue
        line = line.split("//")[0].strip()  # the trailing comment holds address and encoding
        if cur is not None and line:
            cur.append(line)
    return syms


def descriptors(obj):
    """kernel symbol → the descriptor values of the code object's metadata note."""
    out = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", obj], check=True, stdout=subprocess.PIPE, text=True).stdout
    kernels, cur, indent, inside = [], None, None, False
    for line in out.splitlines():
        if line.strip() == "amdhsa.kernels:":
            inside, indent = True, None
            continue
        if not inside:
            continue
        m = re.match(r"^(\s*)(- )?(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            if line and not line.startswith(" "):
                inside = False
            continue
        lead = len(m.group(1))
        if m.group(2) and (indent is None or lead == indent):  # the next entry of the list of kernels
            indent = lead
            cur = {}
            kernels.append(cur)
        if cur is not None and lead + (2 if m.group(2) else 0) == indent + 2 and (m.group(3) in DESCRIPTOR_KEYS or m.group(3) == ".name"):
            cur[m.group(3)] = m.group(4).strip()
    return {k.pop(".name"): k for k in kernels if ".name" in k}


def build_tree(tree, outdir, only, jobs):
    csrc = os.path.join(tree, "tak_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and (not only or f in only))
    flags = makefile_flags(csrc)
    os.makedirs(outdir, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        objs = list(pool.map(lambda n: compile_device(csrc, n, outdir, flags), names))
    return {n: (disassembly(o), descriptors(o)) for n, o in zip(names, objs)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--only", nargs="*", default=[], help="file names under tak_amd/csrc to compare (default: every *.hip)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--show", type=int, default=0, help="lines of unified diff to print for a symbol that differs")
    ap.add_argument("--quiet", action="store_true", help="print only the symbols that are not `same`, and the summary")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="kernel_isa_diff_") as tmp:
        A = build_tree(resolve_tree(args.a, tmp), os.path.join(tmp, "obj_a"), args.only, args.jobs)
        B = build_tree(resolve_tree(args.b, tmp), os.path.join(tmp, "obj_b"), args.only, args.jobs)
    count = {"same": 0, "differs": 0, "only in A": 0, "only in B": 0}
    kernels = 0
    for name in sorted(set(A) | set(B)):
        (ta, da), (tb, db) = A.get(name, ({}, {})), B.get(name, ({}, {}))
        for sym in sorted(set(ta) | set(tb)):
            if sym not in tb:
                verdict = "only in A"
            elif sym not in ta:
                verdict = "only in B"
            else:
                what = []
                if ta[sym] != tb[sym]:
                    what.append(f"text ({len(ta[sym])} → {len(tb[sym])} instructions)")
                what += [f"{k} {da[sym].get(k)} → {db[sym].get(k)}" for k in DESCRIPTOR_KEYS
                         if sym in da and sym in db and da[sym].get(k) != db[sym].get(k)]
                if (sym in da) != (sym in db):
                    what.append("kernel descriptor on one side only")
                verdict = "differs" if what else "same"
            count[verdict] += 1
            kernels += sym in da or sym in db
            if verdict != "same" or not args.quiet:
                print(f"{verdict:9s} {name} {sym}" + (": " + "; ".join(what) if verdict == "differs" else ""))
            if verdict == "differs" and args.show:
                for line in list(difflib.unified_diff(ta[sym], tb[sym], "A", "B", lineterm="", n=2))[: args.show]:
                    print("    " + line)
    total = sum(count.values())
    print(f"{len(set(A) | set(B))} files, {total} symbols ({kernels} kernels): {count['same']} same, {count['differs']} differ, "
          f"{count['only in A']} only in A, {count['only in B']} only in B")
    return 0 if count["same"] == total and total > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
