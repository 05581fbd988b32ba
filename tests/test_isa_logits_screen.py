"""Invariants of the screening instantiation of the product kernel, k_fgemm<FG_SCREEN> (mcq_fix_kernels.h), on the gfx950
ISA the compiler emits (no GPU needed: hipcc cross-compiles).  It walks the tiles like k_fgemm<0> / <1> with limbs 0-2 only:
THREE LDS-DMA pieces per wave and ring stage, so the sync of a step waits until the pieces of the two later stages are the
only ones outstanding, `s_waitcnt vmcnt(6)`, and the prologue, with four stages requested, until those of three are,
`vmcnt(9)`.  test_isa_invariants.py keeps pinning k_fgemm<0> / <1> (four pieces, vmcnt(8), 40 MFMAs)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PIECES = 3           # limb planes requested per wave and stage


@pytest.fixture(scope="module")
def isa(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "mcq.s"
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-S", "--cuda-device-only",
                           "-w", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "quantization_amd", "csrc", "mcq_api.hip"),
                           "-o", str(out)])
    return open(out).read().split("\n")


def kernel_body(isa, pref):
    start = next(i for i, l in enumerate(isa) if l.startswith(pref) and ":" in l)
    end = next(i for i in range(start, len(isa)) if "s_endpgm" in isa[i])
    body = [l.split(";")[0].strip() for l in isa[start:end]]
    return [l for l in body if l]


def test_screen_kernel_steps_request_three_pieces_and_wait_for_all_but_six(isa):
    body = kernel_body(isa, "_ZN3mcq7k_fgemmILi2EEE")
    assert not any(l.startswith("scratch_") for l in body)
    # m0 is written by the DMA asm only
    assert not any(re.search(r"s_set_gpr_idx|v_movrel|ds_gws|s_movrel", l) for l in body)
    m0_writes = [l for l in body if re.search(r"\bm0\b", l) and not l.startswith("s_mov_b32 m0,")]
    assert not m0_writes, m0_writes[:3]
    n_m0 = sum(1 for l in body if l.startswith("s_mov_b32 m0,"))
    n_dma = sum(1 for l in body if l.startswith("global_load_lds_dword"))
    assert n_m0 == n_dma and n_dma >= 4 * PIECES + 2 * PIECES      # four stages of the prologue, the two unrolled steps (+ info)
    # the counted waits that belong to PIECES pieces: three later stages after the prologue, two in the loop; nothing else counted
    counted = sorted(set(int(m.group(1)) for l in body for m in [re.search(r"vmcnt\((\d+)\)", l)] if m and m.group(1) != "0"))
    assert counted == [2 * PIECES, 3 * PIECES], counted
    syncs = [i for i, l in enumerate(body) if l == "s_barrier" and any(f"vmcnt({2 * PIECES})" in x for x in body[max(0, i - 4):i])]
    assert len(syncs) == 2, len(syncs)
    seg = body[syncs[0]:syncs[1]]
    assert sum(1 for l in seg if l.startswith("global_load_lds_dwordx4")) == PIECES
    assert sum(1 for l in seg if l.startswith("v_mfma_i32_32x32x32_i8")) >= 10      # 12 per step (a few may be hoisted above the barrier)
    assert not any(re.search(r"^(global_load_dword|global_store|global_atomic|buffer_|scratch_|flat_)", l) and "lds" not in l
                   for l in seg)
    # six limb pairs x two MFMA tiles x the two unrolled steps
    assert sum(1 for l in body if l.startswith("v_mfma_i32_32x32x32_i8")) == 24


def test_recheck_kernel_uses_integer_dot_products_and_no_scratch(isa):
    body = kernel_body(isa, "_ZN3mcq17k_fscreen_recheck")
    assert not any(l.startswith("scratch_") for l in body)
    # ten limb pairs x the four words of a 16-column chunk (v_dot4_i32_i8 or its accumulating form v_dot4c_i32_i8)
    assert sum(1 for l in body if re.match(r"v_dot4c?_i32_i8", l)) >= 40
    assert not any(l.startswith("v_mfma") for l in body)


@pytest.mark.parametrize("mode", [0, 1])
def test_ten_product_kernels_keep_their_shape(isa, mode):
    body = kernel_body(isa, f"_ZN3mcq7k_fgemmILi{mode}EEE")
    assert sum(1 for l in body if l.startswith("v_mfma_i32_32x32x32_i8")) == 40
    counted = sorted(set(int(m.group(1)) for l in body for m in [re.search(r"vmcnt\((\d+)\)", l)] if m and m.group(1) != "0"))
    assert counted == [8, 12], counted
