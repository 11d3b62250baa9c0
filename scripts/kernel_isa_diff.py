#!/usr/bin/env python3
"""Did a change move any kernel?  Compare the device code of two source trees, kernel by kernel.

    python scripts/kernel_isa_diff.py A B [--only tower_kernels.hip ...] [--jobs 8] [--show 20] [--pairs FILE] [--mask-pcrel]

A and B are directories that hold tak_amd/csrc/, or git revisions of this repository (exported with `git archive` into a
temporary directory; `.` and paths are taken as directories first).  Every tak_amd/csrc/*.hip of each tree is compiled
device-only with that tree's Makefile FLAGS (+ --cuda-device-only --no-gpu-bundle-output -c: an AMDGPU ELF that llvm-objdump
reads), disassembled and split per symbol with addresses and encodings dropped; the kernel descriptors (VGPR / AGPR / SGPR
counts, LDS and private-segment size, ...) come from `llvm-readelf --notes`.  A symbol is compared wherever it lives: the two
trees are paired by symbol name over all their compiled files, not per file name, so a kernel that moved to another translation
unit is `same` if its text and descriptor are; the line names the file on both sides.  A symbol that one tree emits from two
files is `twice`, a failure of its own.  A kernel that was renamed is paired through --pairs (a file of lines `OLD NEW`, mangled
names): its line shows `OLD → NEW`.  What llvm-objdump prints behind a symbol's last instruction — the zero fill up to the next
symbol's alignment (`...`), the s_nop / s_code_end padding behind the last symbol of .text — is dropped: it belongs to the symbol's
place in its file, not to the kernel, and differs as soon as a kernel has another neighbour.  --only is applied per tree to the
files that exist there.  --mask-pcrel replaces the literal of the `s_add_u32` that follows an `s_getpc_b64` (the pc-relative distance to a
constant table in .rodata) by `<pcrel>`: it changes whenever a file gains or loses code between the table and the kernel, which is the
kernel's place in its file again, and with the mask such a kernel is `same`.  Per symbol one line: same / differs / only in A / only in B / twice; then a summary line.  Exit status 0
only if every symbol is `same`.  Needs hipcc and no GPU.
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


def disassembly(obj, mask_pcrel=False):
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
            if mask_pcrel and cur and cur[-1].startswith("s_getpc_b64"):
                line = re.sub(r"^(s_add_u32 s\d+, s\d+, )0x[0-9a-f]+$", r"\1<pcrel>", line)
            cur.append(line)
    # what the assembler puts behind a symbol's last instruction belongs to its place in the file, not to it: the zero fill up to
    # the next symbol's alignment (`...`) and the s_nop / s_code_end padding behind the last symbol of the section
    for text in syms.values():
        while text and text[-1] in ("...", "s_nop 0", "s_code_end"):
            text.pop()
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


def build_tree(tree, outdir, only, jobs, mask_pcrel=False):
    csrc = os.path.join(tree, "tak_amd", "csrc")
    names = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and (not only or f in only))
    flags = makefile_flags(csrc)
    os.makedirs(outdir, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        objs = list(pool.map(lambda n: compile_device(csrc, n, outdir, flags), names))
    syms, twice = {}, {}  # symbol → (file, instructions, descriptor or None); symbol → every file that emits it
    for n, o in zip(names, objs):
        desc = descriptors(o)
        for sym, text in disassembly(o, mask_pcrel).items():
            if sym in syms:
                twice.setdefault(sym, [syms[sym][0]]).append(n)
            else:
                syms[sym] = (n, text, desc.get(sym))
    return names, syms, twice


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--only", nargs="*", default=[], help="file names under tak_amd/csrc to compare, where a tree has them (default: every *.hip)")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--show", type=int, default=0, help="lines of unified diff to print for a symbol that differs")
    ap.add_argument("--quiet", action="store_true", help="print only the symbols that are not `same`, and the summary")
    ap.add_argument("--pairs", help="a file of lines `OLD NEW` (mangled names; `#` starts a comment): symbol OLD of A is compared with "
                                    "symbol NEW of B, for kernels that were renamed")
    ap.add_argument("--mask-pcrel", action="store_true", help="compare pc-relative literals (s_getpc_b64 + s_add_u32) as equal")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="kernel_isa_diff_") as tmp:
        files_a, A, twice_a = build_tree(resolve_tree(args.a, tmp), os.path.join(tmp, "obj_a"), args.only, args.jobs, args.mask_pcrel)
        files_b, B, twice_b = build_tree(resolve_tree(args.b, tmp), os.path.join(tmp, "obj_b"), args.only, args.jobs, args.mask_pcrel)
    was = {}  # NEW → OLD for the pairs that were applied: from here on A holds OLD's code under NEW's name
    for line in open(args.pairs) if args.pairs else ():
        pair = line.split("#")[0].split()
        if len(pair) == 2 and pair[0] in A and pair[1] not in A:
            was[pair[1]] = pair[0]
            A[pair[1]] = A.pop(pair[0])
            if pair[0] in twice_a:
                twice_a[pair[1]] = twice_a.pop(pair[0])
    count = {"same": 0, "differs": 0, "only in A": 0, "only in B": 0, "twice": 0}
    kernels = 0
    for sym in sorted(set(A) | set(B)):
        what = []
        if sym in twice_a or sym in twice_b:
            verdict = "twice"
            what = [f"{side} emits it from {' and '.join(t[sym])}" for side, t in (("A", twice_a), ("B", twice_b)) if sym in t]
        elif sym not in B:
            verdict = "only in A"
        elif sym not in A:
            verdict = "only in B"
        else:
            (_, ta, da), (_, tb, db) = A[sym], B[sym]
            if ta != tb:
                what.append(f"text ({len(ta)} → {len(tb)} instructions)")
            if da is not None and db is not None:
                what += [f"{k} {da.get(k)} → {db.get(k)}" for k in DESCRIPTOR_KEYS if da.get(k) != db.get(k)]
            elif (da is None) != (db is None):
                what.append("kernel descriptor on one side only")
            verdict = "differs" if what else "same"
        count[verdict] += 1
        fa, fb = (A[sym][0] if sym in A else None), (B[sym][0] if sym in B else None)
        kernels += (sym in A and A[sym][2] is not None) or (sym in B and B[sym][2] is not None)
        if verdict != "same" or not args.quiet:
            where = fa if fa == fb else f"{fa} → {fb}" if fa and fb else fa or fb
            name = f"{was[sym]} → {sym}" if sym in was else sym
            print(f"{verdict:9s} {where} {name}" + (": " + "; ".join(what) if what else ""))
        if verdict == "differs" and args.show:
            for line in list(difflib.unified_diff(A[sym][1], B[sym][1], "A", "B", lineterm="", n=2))[: args.show]:
                print("    " + line)
    total = sum(count.values())
    print(f"{len(files_a)} → {len(files_b)} files, {total} symbols ({kernels} kernels): {count['same']} same, {count['differs']} differ, "
          f"{count['only in A']} only in A, {count['only in B']} only in B, {count['twice']} twice")
    return 0 if count["same"] == total and total > 0 else 1


if __name__ == "__main__":
    sys.exit(main())
