#!/usr/bin/env python3
"""Did a change move an instruction?  Compare the gfx950 code of two builds, function by function.

  python tools/diff_codegen.py OLD NEW [--rewrite 'REGEX=>REPLACEMENT' ...] [--max-diffs N]

OLD and NEW are two libraries or object files.  Their gfx950 code objects are taken out with tools/extract_co.py; for every function
symbol the tool compares the bytes of its body, its kernel descriptor (without the code-entry offset, which is the function's address)
and its entry in the code-object metadata: VGPRs, AGPRs, SGPRs, LDS, scratch, spill counts, kernarg size and the other scalar fields.
Functions are matched by their demangled names (`c++filt`).  A refactor that renames template arguments passes one `--rewrite` per
renamed argument: a regular expression and its replacement (Python `re.sub` syntax), applied to the demangled names of both sides, e.g.

  --rewrite '(stream_frame_major_lds<.*, \\d+), 1, ((?:true|false), (?:true|false)), false>=>\\1, \\2>'

An instantiation that several translation units hold is matched occurrence by occurrence, in the order of the code objects (the link
order).  The tool prints the counts of identical, differing, only-old and only-new functions, the names of the last two groups, and for
each differing function what differs plus a unified diff of its `llvm-objdump -d` text with the addresses, encodings and resolved branch
targets taken out (the branch operands that remain are relative), with a hint where every differing line differs in one literal only.
It only compares: it knows nothing about particular instructions.
Exit status 1 if anything differs or is on one side only.
"""
from __future__ import annotations

import argparse
import collections
import difflib
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LLVM = "/opt/rocm/lib/llvm/bin"
KD_ENTRY_OFFSET = slice(16, 24)  # kernel_code_entry_byte_offset of the 64-byte kernel descriptor: where the code sits, not what it is

Function = collections.namedtuple("Function", "raw co body kd meta")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def functions_of(path, tmp):
    """[Function] of every function symbol in the gfx950 code objects of `path`, in code-object order."""
    run(sys.executable, os.path.join(HERE, "extract_co.py"), path, tmp)
    out = []
    for co in sorted(glob.glob(os.path.join(tmp, "co*.o")), key=lambda p: int(re.search(r"co(\d+)\.o$", p).group(1))):
        data = open(co, "rb").read()
        sections = {}  # index -> (address, file offset)
        for m in re.finditer(r"^\s*\[\s*(\d+)\]\s+\S*\s+(?:PROGBITS|NOBITS)\s+([0-9a-f]+)\s+([0-9a-f]+)\s", run(LLVM + "/llvm-readelf", "-SW", co), re.M):
            sections[int(m.group(1))] = (int(m.group(2), 16), int(m.group(3), 16))
        funcs, objects = [], {}
        symtab = run(LLVM + "/llvm-readelf", "-sW", "--symbols", co).split("Symbol table '.symtab'")[-1]
        for line in symtab.splitlines():
            f = line.split()
            if len(f) != 8 or not f[6].isdigit() or f[3] not in ("FUNC", "OBJECT"):
                continue
            addr, sec = sections[int(f[6])]
            start = int(f[1], 16) - addr + sec
            blob = data[start:start + int(f[2])]
            if f[3] == "FUNC":
                funcs.append((f[7], blob))
            else:
                objects[f[7]] = blob
        meta = {}
        for blk in re.split(r"\n(?=\s*- \.agpr_count:)", run(LLVM + "/llvm-readelf", "--notes", co))[1:]:
            # the kernel's own scalar fields sit at the entry's indentation ("  - .agpr_count:" / "    .vgpr_count:"), its arguments deeper
            fields = dict(re.findall(r"^(?:  - |    )(\.\w+):[ \t]+(\S.*?)\s*$", blk, re.M))
            args = re.search(r"^    \.args:\n((?:      .*\n)*)", blk, re.M)
            sym = fields.pop(".symbol", None)
            fields.pop(".name", None)
            fields[".args"] = re.sub(r"\s+", " ", args.group(1)) if args else ""
            if sym:
                meta[sym] = fields
        for raw, body in funcs:
            kd = objects.get(raw + ".kd")
            if kd is not None:
                kd = kd[:KD_ENTRY_OFFSET.start] + kd[KD_ENTRY_OFFSET.stop:]
            out.append(Function(raw, co, body, kd, meta.get(raw + ".kd")))
    return out


def demangled(names):
    return subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()


def by_name(funcs, rewrites):
    table = collections.defaultdict(list)
    for f, name in zip(funcs, demangled([f.raw for f in funcs])):
        for pattern, repl in rewrites:
            name = pattern.sub(repl, name)
        table[name].append(f)
    return {(name, k): f for name, fs in table.items() for k, f in enumerate(fs)}


def listing(f):
    """The disassembly of one function without addresses, encodings and resolved targets."""
    text = run(LLVM + "/llvm-objdump", "-d", "--disassemble-symbols=" + f.raw, f.co)
    lines = [re.sub(r"\s*//.*$", "", line).rstrip() for line in text.splitlines()]
    return [re.sub(r"\s+", " ", line.strip()) for line in lines if line.startswith(("\t", " ")) and line.strip()]


def only_a_literal_differs(x, y):
    """Two lines of disassembly that are equal but for one operand, a number on both sides."""
    fx, fy = x.replace(",", " ").split(), y.replace(",", " ").split()
    odd = [(p, q) for p, q in zip(fx, fy) if p != q]
    return len(fx) == len(fy) and len(odd) == 1 and all(re.fullmatch(r"-?(0x[0-9a-f]+|\d+)", t) for t in odd[0])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rewrite", action="append", default=[], metavar="REGEX=>REPL", help="rename in the demangled names of both sides before matching")
    ap.add_argument("--max-diffs", type=int, default=1000, help="print the disassembly diff of at most this many differing functions")
    args = ap.parse_args(argv)
    rewrites = []
    for r in args.rewrite:
        pattern, sep, repl = r.partition("=>")
        if not sep:
            ap.error("--rewrite takes REGEX=>REPLACEMENT")
        rewrites.append((re.compile(pattern), repl))
    tmp = tempfile.mkdtemp(prefix="idsp_codegen_")
    try:
        old = by_name(functions_of(args.old, os.path.join(tmp, "old")), rewrites)
        new = by_name(functions_of(args.new, os.path.join(tmp, "new")), rewrites)
        same, differing = 0, []
        for key in sorted(old.keys() & new.keys()):
            a, b = old[key], new[key]
            what = [w for w, x, y in (("body", a.body, b.body), ("kernel descriptor", a.kd, b.kd), ("metadata", a.meta, b.meta)) if x != y]
            if what:
                differing.append((key, what))
            else:
                same += 1
        only_old, only_new = sorted(old.keys() - new.keys()), sorted(new.keys() - old.keys())
        print(f"{same} identical, {len(differing)} differing, {len(only_old)} only in OLD, {len(only_new)} only in NEW "
              f"({len(old)} functions in OLD, {len(new)} in NEW)")
        for title, keys in (("only in OLD", only_old), ("only in NEW", only_new)):
            for name, k in keys:
                print(f"  {title}: {name}" + (f"  [occurrence {k + 1}]" if k else ""))
        for n, ((name, k), what) in enumerate(differing):
            a, b = old[(name, k)], new[(name, k)]
            print(f"\ndiffers in {', '.join(what)}: {name}" + (f"  [occurrence {k + 1}]" if k else ""))
            if "metadata" in what and a.meta and b.meta:
                for field in sorted(a.meta.keys() | b.meta.keys()):
                    if a.meta.get(field) != b.meta.get(field):
                        print(f"  {field}: {a.meta.get(field)} -> {b.meta.get(field)}")
            if "body" in what and n < args.max_diffs:
                la, lb = listing(a), listing(b)
                print(f"  {len(a.body)} -> {len(b.body)} bytes, {len(la)} -> {len(lb)} lines of disassembly")
                sys.stdout.writelines(line + "\n" for line in difflib.unified_diff(la, lb, "OLD", "NEW", lineterm="", n=3))
                if len(la) == len(lb) and all(only_a_literal_differs(x, y) for x, y in zip(la, lb) if x != y):
                    print("  (every differing line differs in one literal operand only: if it is a PC-relative offset, a section moved, not the code)")
        return 1 if differing or only_old or only_new else 0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
