#!/usr/bin/env python3
"""Per-kernel comparison of the device code of two source trees (CPU only; needs hipcc, no GPU).

    python tools/kernel_isa_diff.py OLD_TREE NEW_TREE [--source acrobot_kernels.hip] [--out DIR] [--allow-new]
                                    [--rename OLD=NEW ...]

Each tree's translation unit is compiled device-only to assembly with _build.py's flags (and a fixed build id), and
the two outputs are compared per kernel symbol rather than as whole files, because moving code between files
changes the order of the functions.  For every kernel three things must be the same text:

  * the instruction body, from the symbol's binding directives and label to its end label (comments dropped);
  * its .amdhsa_kernel descriptor block;
  * its entry in the amdhsa.kernels metadata (argument offsets and sizes, register counts, LDS, scratch).

Local labels are renumbered first (.LBB<f>_<n> carries the function's ordinal <f>), the compilation-unit id symbol
is ignored, the kernel symbol sets must be equal, and so must the device-side objects (globals, read-only data)
as a set.  Every device function of these translation units is inlined into its kernels, so "identical" here means
that only host code differs between the trees.  OLD_TREE / NEW_TREE may also be an assembly file (*.s) already made.

A kernel whose name changed is paired by --rename OLD=NEW (repeatable).  Each side is the kernel's mangled symbol or
any part of it that no other kernel's symbol contains, e.g. --rename k_mpc_box_qp_fb=k_mpc_box_qpILb1E for a twin
kernel that became the template instantiation k_mpc_box_qp<true, ...>.  The pair is compared like any other kernel,
with the symbol's own name masked in body, descriptor and metadata; a side that selects no kernel, or more than one,
is an error (exit 2).

Prints one result line, e.g. "acrobot_kernels.hip: 106/106 identical", and exits 1 on any difference.
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys
import tempfile

ARCH = os.environ.get("GYM_OFFLOAD_ARCH", "gfx950")
PKG = "gymnast_optimalcontrol_amd"
LOCAL_LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return "hipcc"


def compile_asm(tree: str, source: str, out: str) -> str:
    csrc = os.path.join(tree, PKG, "csrc")
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", '-DGYM_BUILD_ID="isa-diff"',
           "-I", os.path.join(tree, "include"), "-I", csrc, "--cuda-device-only", "-S",
           os.path.join(csrc, source), "-o", out]
    subprocess.run(cmd, check=True)
    return out


def renumber(line: str) -> str:
    """Local labels without the function's ordinal: .LBB12_7 -> .LBB_7, .Lfunc_end12 -> .Lfunc_end.  Comments go
    too (they repeat the ordinal: "in Loop: Header=BB12_4"), except on string data, where ';' may be content."""
    if not line.lstrip().startswith((".asci", ".string")):
        line = line.split(";")[0].rstrip()
    return LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def parse(path: str) -> dict:
    """{'body': {sym: text}, 'desc': {sym: text}, 'meta': {sym: text}, 'objects': {name: text}}"""
    with open(path) as f:
        lines = f.read().split("\n")
    try:
        m0, m1 = lines.index("\t.amdgpu_metadata"), lines.index("\t.end_amdgpu_metadata")
    except ValueError:
        sys.exit(f"{path}: no .amdgpu_metadata block")
    code, meta_lines = lines[:m0], lines[m0 + 1:m1]

    desc, body, objects = {}, {}, {}
    i = 0
    while i < len(code):
        ln = code[i]
        if ln.startswith("\t.amdhsa_kernel "):
            sym = ln.split()[1]
            j = code.index("\t.end_amdhsa_kernel", i)
            desc[sym] = "\n".join(code[i:j + 1])
            i = j
        elif ln.startswith("\t.type\t") and ",@object" in ln:
            name = ln.split("\t")[2].split(",")[0]
            j = i
            while not code[j].startswith(f"\t.size\t{name},"):
                j += 1
            if not name.startswith("__hip_cuid_"):
                objects[renumber(name)] = "\n".join(renumber(c) for c in code[i:j + 1])
            i = j
        i += 1
    labels = {c.split(":")[0]: n for n, c in enumerate(code) if c[:1] not in ("\t", " ", ";", "") and ":" in c}
    for sym in desc:
        start = j = labels[sym]
        while code[start - 1].startswith("\t.") and not code[start - 1].startswith(("\t.section", "\t.text")):
            start -= 1                       # the symbol's binding directives (.globl, .protected, alignment)
        while not re.match(r"\.Lfunc_end\d+:", code[j]):
            j += 1
        text = [renumber(c) for c in code[start:j + 1]]
        d0 = text.index(renumber(f"\t.amdhsa_kernel {sym}"))      # the descriptor sits inside: compared on its own
        d1 = text.index("\t.end_amdhsa_kernel")
        body[sym] = "\n".join(text[:d0] + text[d1 + 1:])

    meta = {}
    k0 = meta_lines.index("amdhsa.kernels:")
    entry: list[str] = []

    def flush():
        if entry:
            name = next(e.split()[1] for e in entry if e.strip().startswith(".name:"))
            meta[name] = "\n".join(entry)

    for ln in meta_lines[k0 + 1:]:
        if ln.startswith("amdhsa."):
            break
        if ln.startswith("  - "):
            flush()
            entry = []
        entry.append(ln)
    flush()
    return {"body": body, "desc": desc, "meta": meta, "objects": objects}


def pick(symbols, part: str) -> list:
    """The kernel symbols that are, or contain, `part`: a rename needs exactly one."""
    return [part] if part in symbols else sorted(s for s in symbols if part in s)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--source", default="acrobot_kernels.hip", help="translation unit under csrc/")
    ap.add_argument("--out", default=None, help="directory that keeps the two assembly files")
    ap.add_argument("--allow-new", action="store_true",
                    help="kernels only in NEW are listed but are no difference: every kernel of OLD must be identical")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW",
                    help="kernel OLD of the old side is kernel NEW of the new side (symbols, or unique parts of them)")
    args = ap.parse_args(argv)
    out = args.out or tempfile.mkdtemp(prefix="isa_diff_")
    os.makedirs(out, exist_ok=True)
    stem = os.path.splitext(args.source)[0]
    sides = []
    for tag, tree in (("old", args.old), ("new", args.new)):
        asm = tree if tree.endswith(".s") else compile_asm(tree, args.source, os.path.join(out, f"{stem}.{tag}.s"))
        sides.append(parse(asm))
    old, new = sides
    pairs = []
    for pair in args.rename:
        o, sep, n = pair.partition("=")
        if not (o and sep and n):
            ap.error(f"--rename: {pair!r} is not OLD=NEW")
        for part, side, tag in ((o, old, "OLD"), (n, new, "NEW")):
            hits = pick(side["desc"], part)
            if len(hits) != 1:
                ap.error(f"--rename: {part!r} selects {len(hits)} kernels of {tag}" + "".join(f"\n  {h}" for h in hits))
            pairs.append(hits[0])
    for o, n in zip(pairs[::2], pairs[1::2]):    # NEW's kernel takes OLD's symbol, both with their own name masked
        if o != n and o in new["desc"]:
            ap.error(f"--rename: NEW has a kernel {o} of its own")
        for p in ("body", "desc", "meta"):
            old[p][o] = old[p][o].replace(o, "<kernel>")
            new[p][o] = new[p].pop(n).replace(n, "<kernel>")
    bad = 0
    only_old, only_new = sorted(set(old["desc"]) - set(new["desc"])), sorted(set(new["desc"]) - set(old["desc"]))
    for s in only_old:
        print(f"missing in NEW: {s}")
    for s in only_new:
        print(f"only in NEW:    {s}")
    common = sorted(set(old["desc"]) & set(new["desc"]))
    same = 0
    for s in common:
        parts = [p for p in ("body", "desc", "meta") if old[p].get(s) != new[p].get(s)]
        if parts:
            print(f"differs ({', '.join(parts)}): {s}")
        else:
            same += 1
    # an additive change (--allow-new): NEW may hold more kernels and their objects; only OLD's are compared
    names = set(old["objects"]) if args.allow_new else set(old["objects"]) | set(new["objects"])
    for n in sorted(names):
        if old["objects"].get(n) != new["objects"].get(n):
            bad += 1
            print(f"device object differs: {n}")
    total = len(set(old["desc"]) | set(new["desc"]))
    added = ""
    if args.allow_new:
        total -= len(only_new)
        added = f", {len(only_new)} new" if only_new else ""
    ok = same == total and not bad
    print(f"{args.source}: {same}/{total} identical{added}" + ("" if ok else "  -- DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
