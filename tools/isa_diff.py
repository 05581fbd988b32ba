#!/usr/bin/env python3
"""Kernel by kernel comparison of two device assemblies of quantization_amd/csrc/mcq_api.hip (no GPU):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -S --cuda-device-only -w mcq_api.hip -o <tree>.s
    python tools/isa_diff.py parent.s result.s [--drop-arg ", unsigned char"] [--out profiles/<name>.txt]

Per `.amdhsa_kernel` symbol: the instruction text (comments dropped; `.LBB<n>_`, `.Lfunc_begin<n>`, `.Lfunc_end<n>`, `.Ltmp<n>`
renumbered by first appearance; the kernel's own name replaced) and the descriptor block.  Symbols are matched by their
demangled names; --drop-arg removes a trailing template argument from the names of the second file, so that a template that
gained a defaulted parameter (k_search_wide<8, 0, false> -> k_search_wide<8, 0, false, unsigned char>) is held against the
instantiation it was.  Prints the counts, every kernel of the first file that is missing or differs, and for the kernels only
the second file has their number, VGPR range, largest LDS and scratch use.  Exit status 1 if a kernel of the first file moved."""
import argparse
import re
import subprocess
import sys

LABELS = re.compile(r"\.LBB\d+_\d+|\.Lfunc_begin\d+|\.Lfunc_end\d+|\.Ltmp\d+")


def kernels(path):
    """{symbol: (body lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    known = set(names)
    desc_at = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m}
    start = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"(\S+):", l)] if m and m.group(1) in known}
    out = {}
    for name in names:
        i = start[name] + 1
        body = []
        while not lines[i].startswith(".Lfunc_end"):
            text = lines[i].split(";")[0].strip()
            if text and not text.startswith((".p2align", ".loc", ".file", ".cfi")):
                body.append(text)
            i += 1
        d = desc_at[name]
        desc = []
        while ".end_amdhsa_kernel" not in lines[d]:
            d += 1
            desc.append(lines[d].strip())
        seen = {}
        body = [LABELS.sub(lambda m: seen.setdefault(m.group(0), f"L{len(seen)}"), l).replace(name, "SELF") for l in body]
        out[name] = (body, desc)
    return out


def demangled(names):
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, got.stdout.split("\n")))


def field(desc, key):
    return next(int(l.split()[-1]) for l in desc if l.startswith(key + " "))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("first")
    ap.add_argument("second")
    ap.add_argument("--drop-arg", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    A, B = kernels(a.first), kernels(a.second)
    da, db = demangled(list(A)), demangled(list(B))
    by_name = {}
    for sym, name in db.items():
        by_name[name] = sym
    if a.drop_arg:                                   # the names the second file's kernels had before the argument existed
        for sym, name in db.items():
            old = re.sub(re.escape(a.drop_arg) + r">\(", ">(", name, count=1)
            if old != name:
                assert old not in by_name, old
                by_name[old] = sym
    report, moved, matched = [], 0, set()
    for sym, name in da.items():
        other = by_name.get(name)
        if other is None:
            report.append(f"MISSING  {name}")
            moved += 1
            continue
        matched.add(other)
        if A[sym][0] != B[other][0] or A[sym][1] != B[other][1]:
            what = "body" if A[sym][0] != B[other][0] else "descriptor"
            report.append(f"DIFFERS ({what})  {name}")
            moved += 1
    new = [s for s in B if s not in matched]
    head = [f"{a.first}: {len(A)} kernels; {a.second}: {len(B)} kernels",
            f"kernels of the first file with identical instruction text and descriptor in the second: {len(A) - moved} of {len(A)}",
            f"kernels only the second file has: {len(new)}"]
    if new:
        v = [field(B[s][1], ".amdhsa_next_free_vgpr") for s in new]
        acc = [field(B[s][1], ".amdhsa_accum_offset") for s in new]
        scratch = [field(B[s][1], ".amdhsa_private_segment_fixed_size") for s in new]
        lds = [field(B[s][1], ".amdhsa_group_segment_fixed_size") for s in new]
        head.append(f"  next_free_vgpr {min(v)} .. {max(v)} (accum_offset {min(acc)} .. {max(acc)}), static LDS at most {max(lds)} B, "
                    f"scratch at most {max(scratch)} B ({sum(1 for x in scratch if x)} kernels with scratch)")
        fam = {}
        for s in new:
            fam.setdefault(re.sub(r"<.*", "", db[s].replace("void ", "")), []).append(field(B[s][1], ".amdhsa_next_free_vgpr"))
        head += [f"  {k}: {len(x)} kernels, VGPRs {min(x)} .. {max(x)}" for k, x in sorted(fam.items())]
    text = "\n".join(head + report) + "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
