#!/usr/bin/env python3
"""Registers, LDS and scratch of every kernel of the library, from the code-object metadata of a device assembly (no GPU):

    python tools/kernel_resources.py [--asm <file>.s] [--match k_tf_] [--strided] [--out profiles/<name>.txt]

Without --asm, compiles quantization_amd/csrc/mcq_api.hip for gfx950 with the library's flags (device side only, about two
minutes) into a temporary file.  Per kernel, by demangled name: VGPRs (.vgpr_count), SGPRs, SGPR spills, VGPR spills, static LDS
and scratch bytes, and the waves per SIMD the VGPRs allow -- 512 registers per lane and SIMD, allocated in granules of 8, at most
8 waves.  --match keeps the kernels whose name contains the text; --strided keeps the STRIDED = true instantiations of the pass
kernels (k_tf_stage0, k_tf_pair0s, k_tf_pair1, k_tf_table1, k_tf_level1, k_tf_comb) and exits with status 1 if one of those with
one-byte entries and 8 or 16 codebooks -- the shapes the encode's capped passes run -- has more than 64 VGPRs, an SGPR spill or
scratch."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "quantization_amd", "csrc", "mcq_api.hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only", "-w"]
KEYS = ("vgpr_count", "sgpr_count", "sgpr_spill_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")


def compile_asm():
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc] + FLAGS + [SRC, "-o", out], cwd=os.path.dirname(SRC))
    return out


def kernels(path):
    """[{name: mangled, vgpr_count: ..}] from the amdhsa.kernels metadata at the end of the assembly"""
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    out = []
    for block in re.split(r"\n  - \.", meta)[1:]:
        block = "    ." + block
        got = {}
        for key in KEYS + ("name",):
            m = re.search(r"^    \.%s:\s+(\S+)\s*$" % key, block, re.M)
            if m:
                got[key] = m.group(1)
        if "name" in got:
            out.append({k: (got[k] if k == "name" else int(got.get(k, 0))) for k in KEYS + ("name",)})
    return out


def demangled(names):
    got = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return [re.sub(r"^void ", "", re.sub(r"\(.*", "", l)) for l in got.stdout.split("\n")]


def waves(vgprs):
    return min(8, 512 // max(8, (vgprs + 7) & ~7))


STRIDED = {      # kernel -> position of the STRIDED argument from the end of the template argument list
    "mcq::k_tf_stage0": 1, "mcq::k_tf_pair0s": 1, "mcq::k_tf_pair1": 1, "mcq::k_tf_table1": 1, "mcq::k_tf_level1": 1, "mcq::k_tf_comb": 1}


def is_strided(name):
    m = re.match(r"([\w:]+)<(.*)>$", name)
    return bool(m) and m.group(1) in STRIDED and m.group(2).split(", ")[-1] == "true"


def is_checked(name):
    """a strided instantiation the capped passes of 8 or 16 codebooks of one-byte entries launch"""
    m = re.match(r"([\w:]+)<(.*)>$", name)
    args = m.group(2).split(", ")
    if "unsigned short" in args:
        return False
    if m.group(1) == "mcq::k_tf_stage0":
        return int(args[0]) <= 256 and args[1] in ("8", "16")
    if m.group(1) == "mcq::k_tf_comb":       # the last combine of 8 codebooks (16 end in k_tf_comb3; the longer lists are 32 / 64 codebooks')
        return tuple(args[:2]) in (("16", "32"), ("8", "16"))
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default=None)
    ap.add_argument("--match", default=None)
    ap.add_argument("--strided", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ks = kernels(a.asm or compile_asm())
    names = demangled([k["name"] for k in ks])
    rows, bad = [], []
    for k, name in sorted(zip(ks, names), key=lambda t: t[1]):
        if a.match and a.match not in name:
            continue
        if a.strided and not is_strided(name):
            continue
        rows.append(f"{k['vgpr_count']:5d} {k['sgpr_count']:5d} {k['sgpr_spill_count']:6d} {k['vgpr_spill_count']:6d} "
                    f"{k['group_segment_fixed_size']:7d} {k['private_segment_fixed_size']:7d} {waves(k['vgpr_count']):5d}  {name}")
        if a.strided and is_checked(name) and (k["vgpr_count"] > 64 or k["sgpr_spill_count"] or k["private_segment_fixed_size"]):
            bad.append(name)
    text = " VGPR  SGPR s-spil v-spil     LDS scratch waves  kernel\n" + "\n".join(rows) + "\n"
    text += f"{len(rows)} kernels"
    if a.strided:
        text += "; strided instantiations of one-byte entries, 8 / 16 codebooks, past 64 VGPRs or with SGPR spills or scratch: " + \
                (", ".join(bad) if bad else "none")
    text += "\n"
    sys.stdout.write(text)
    if a.out:
        open(a.out, "w").write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
