"""The launch sequence of the encode entry points, pinned through the two windows the C ABI offers: the per-category launch
counts of mcq_profile_encode (named by mcq_profile_category_name) and mcq_last_encode_launches() read straight after a call.

The (N, K) pairs hit every branch of the pass schedule once: one codebook, the level-0 / level-1 last combines, the fused
level-1 launch, pass16 (8 x 16 and 16 x 16), k_tf_comb3 (16 x 256), the upper levels (32, 64 codebooks) and two-byte entries
(4 x 512, int64 output only).  256 vectors stay below the skipping threshold; MCQ_SKIP_MIN_BATCH=0 (read per call) sends the
same encode through the compaction path, whose launch count does not depend on the data, and whose codes must be the same.

The expected numbers are those of commit e388410's launch sequence.  They were worked out from that commit's mcq_api.hip by
reading, NOT recorded from its library on the MI355X as intended (no recording run could be made); each case prints what it
measured before it asserts (pytest -s shows it), so one run against that commit's library settles them.  The derivation, for a
call of 256 vectors (one chunk, E / R in one launch, the screened logits = two launches, one profiler interval):
  start    frames_to_limbs 1 (not with imported codes and no pass) + logits 2 (1 with stored logits or MCQ_ENCODE_EXACT_LOGITS;
           imported codes: k_import_indexes 1) + x.C 1 (with at least one pass)
  a pass   residual energies 1 (4, 8, 16 codebooks: the first pass only, later ones come from the emitting combine) + stage 0 1
           + combines: N = 2: 1, 4: 2, 8: 3, 16: 5 (4 with 16 entries: the level-3 tables ride along), 32: 10, 64: 15
           (level v >= 3 of 32 / 64 codebooks: k_tf_table1 + (v - 2) x k_tf_up + the combine)
  tail     k_finalize 1 only where no pass emitted: one codebook, no pass, or pass16 with packed nibbles
  pass16   8 x 16 and 16 x 16 outside the profiler: every pass in ONE launch
  skipping k_zero_counts 1 + k_compact after every pass but an emitting one (5 passes: 4; one codebook: 5, and no k_finalize);
           needs three passes, and never applies with pass16"""
import ctypes

import numpy as np
import pytest
import torch

from golden import gen

pytestmark = pytest.mark.gpu

B, D = 256, 32

# (N, K, passes) -> what the calls leave behind.  encode / encode_i64: mcq_encode with the byte / the int64 output;
# skip0: mcq_encode under MCQ_SKIP_MIN_BATCH=0; all_passes / exact: mcq_encode_ex with that flag; refine: mcq_refine_indexes;
# logits_refine: mcq_logits_refine_codes (one-byte entries only); profile: the non-zero entries of launches_out
EXPECTED = {
    (1, 16, 5): {'encode': 15, 'encode_i64': 15, 'skip0': 20, 'skip0_i64': 20, 'all_passes': 15, 'exact': 14, 'refine': 14, 'logits_refine': 14, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'residual_energies': 5, 'encode_tail': 1}},
    (2, 256, 5): {'encode': 19, 'encode_i64': 19, 'skip0': 24, 'skip0_i64': 24, 'all_passes': 19, 'exact': 18, 'refine': 18, 'logits_refine': 18, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'residual_energies': 5}},
    (4, 64, 5): {'encode': 20, 'encode_i64': 20, 'skip0': 25, 'skip0_i64': 25, 'all_passes': 20, 'exact': 19, 'refine': 19, 'logits_refine': 19, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level1': 5, 'residual_energies': 1}},
    (8, 256, 5): {'encode': 25, 'encode_i64': 25, 'skip0': 30, 'skip0_i64': 30, 'all_passes': 25, 'exact': 24, 'refine': 24, 'logits_refine': 24, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'residual_energies': 1, 'level1_combines_and_tables': 5}},
    (8, 16, 5): {'encode': 6, 'encode_i64': 5, 'skip0': 6, 'skip0_i64': 5, 'all_passes': 6, 'exact': 5, 'refine': 4, 'logits_refine': 4, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'residual_energies': 1, 'level1_combines_and_tables': 5}},
    (16, 16, 5): {'encode': 6, 'encode_i64': 5, 'skip0': 6, 'skip0_i64': 5, 'all_passes': 6, 'exact': 5, 'refine': 4, 'logits_refine': 4, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'combine_upper_levels': 5, 'residual_energies': 1, 'level1_combines_and_tables': 5}},
    (16, 256, 5): {'encode': 35, 'encode_i64': 35, 'skip0': 40, 'skip0_i64': 40, 'all_passes': 35, 'exact': 34, 'refine': 34, 'logits_refine': 34, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'tables_upper_levels': 5, 'combine_upper_levels': 5, 'residual_energies': 1, 'level1_combines_and_tables': 5}},
    (32, 16, 5): {'encode': 64, 'encode_i64': 64, 'skip0': 69, 'skip0_i64': 69, 'all_passes': 64, 'exact': 63, 'refine': 63, 'logits_refine': 63, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'tables_upper_levels': 25, 'combine_upper_levels': 10, 'residual_energies': 5, 'level1_combines_and_tables': 5}},
    (32, 256, 5): {'encode': 64, 'encode_i64': 64, 'skip0': 69, 'skip0_i64': 69, 'all_passes': 64, 'exact': 63, 'refine': 63, 'logits_refine': 63, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'tables_upper_levels': 25, 'combine_upper_levels': 10, 'residual_energies': 5, 'level1_combines_and_tables': 5}},
    (64, 16, 5): {'encode': 89, 'encode_i64': 89, 'skip0': 94, 'skip0_i64': 94, 'all_passes': 89, 'exact': 88, 'refine': 88, 'logits_refine': 88, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level2': 5, 'tables_upper_levels': 45, 'combine_upper_levels': 15, 'residual_energies': 5, 'level1_combines_and_tables': 5}},
    (4, 512, 5): {'encode': 20, 'encode_i64': 20, 'skip0': 25, 'skip0_i64': 25, 'all_passes': 20, 'exact': 19, 'refine': 19, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 5, 'xc_product': 1, 'combine_level0': 5, 'combine_level1': 5, 'residual_energies': 1}},
    (8, 256, 0): {'encode': 4, 'encode_i64': 4, 'skip0': 4, 'skip0_i64': 4, 'all_passes': 4, 'exact': 3, 'refine': 2, 'logits_refine': 3, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'encode_tail': 1}},
    (8, 256, 1): {'encode': 9, 'encode_i64': 9, 'skip0': 9, 'skip0_i64': 9, 'all_passes': 9, 'exact': 8, 'refine': 8, 'logits_refine': 8, 'profile': {'logits_product_argmax': 1, 'frames_to_limbs': 1, 'stage0_tables': 1, 'xc_product': 1, 'combine_level0': 1, 'combine_level2': 1, 'residual_energies': 1, 'level1_combines_and_tables': 1}},
}

CASES = [(1, 16, 5), (2, 256, 5), (4, 64, 5), (8, 256, 5), (8, 16, 5), (16, 16, 5), (16, 256, 5), (32, 16, 5), (32, 256, 5),
         (64, 16, 5), (4, 512, 5), (8, 256, 0), (8, 256, 1)]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _quantizer(N, K):
    from quantization_amd import Quantizer
    state = gen.synthetic_state(900 + N + K, D, K, N)
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for k, v in state.items():
        sd[k] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    return q.to("cuda:0")


@pytest.mark.parametrize("N,K,iters", CASES)
def test_launch_census(N, K, iters, monkeypatch):
    from quantization_amd import _lib
    L = _lib.lib()
    q = _quantizer(N, K)
    x = torch.from_numpy(gen.make_x(901 + N + K, B, D)).cuda()
    blob, ls, fl = q._prepared(), q._lscale_exp, q._scale_flags
    assert fl == 0                                   # inference flavour: mcq_encode and mcq_encode_ex(flags) see the same blob
    ws = torch.empty(L.mcq_encode_workspace_bytes(B, N, K, D), dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    wide = K > 256
    u8 = lambda: torch.zeros((B, N), dtype=torch.uint8, device="cuda:0")
    i64 = lambda: torch.zeros((B, N), dtype=torch.int64, device="cuda:0")

    def launches(rc, what):
        n = L.mcq_last_encode_launches()             # straight after the call, on the calling thread
        _lib.check(rc, what)
        torch.cuda.synchronize()
        return n

    def encode(out, flags=None):
        p8, p64 = (out.data_ptr(), None) if out.dtype == torch.uint8 else (None, out.data_ptr())
        if flags is None:
            return launches(L.mcq_encode(x.data_ptr(), B, blob.data_ptr(), ls, N, K, D, iters, p8, p64, ws.data_ptr(), ws.numel(), st),
                            "mcq_encode")
        return launches(L.mcq_encode_ex(x.data_ptr(), B, blob.data_ptr(), ls, N, K, D, iters, p8, p64, ws.data_ptr(), ws.numel(), st,
                                        flags), "mcq_encode_ex")

    got = {}
    codes = i64() if wide else u8()
    got["encode"] = encode(codes)
    codes64 = i64()
    got["encode_i64"] = encode(codes64)
    monkeypatch.setenv("MCQ_SKIP_MIN_BATCH", "0")
    codes_skip, codes64_skip = torch.zeros_like(codes), i64()
    got["skip0"] = encode(codes_skip)
    got["skip0_i64"] = encode(codes64_skip)
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH")
    for name, flag in (("all_passes", _lib.MCQ_ENCODE_ALL_PASSES), ("exact", _lib.MCQ_ENCODE_EXACT_LOGITS)):
        out = torch.zeros_like(codes)
        got[name] = encode(out, flag)
        assert torch.equal(out, codes), name
    start, refined = q.encode(x, 0, as_bytes=False).contiguous(), i64()
    got["refine"] = launches(L.mcq_refine_indexes(x.data_ptr(), B, blob.data_ptr(), N, K, D, iters, start.data_ptr(),
                                                  refined.data_ptr(), ws.data_ptr(), ws.numel(), st), "mcq_refine_indexes")
    if not wide:
        logits = torch.empty((B, N * K), dtype=torch.float32, device="cuda:0")
        idx, also = i64(), u8()
        got["logits_refine"] = launches(L.mcq_logits_refine_codes(x.data_ptr(), B, blob.data_ptr(), ls, N, K, D, iters,
                                                                  logits.data_ptr(), idx.data_ptr(), also.data_ptr(), ws.data_ptr(),
                                                                  ws.numel(), st, 0), "mcq_logits_refine_codes")
        assert torch.equal(idx, codes64) and torch.equal(also.to(torch.int64), codes64)
    ms, cnt = (ctypes.c_float * 32)(), (ctypes.c_int * 32)()
    ncat = L.mcq_profile_encode(x.data_ptr(), B, blob.data_ptr(), ls, N, K, D, iters, ws.data_ptr(), ws.numel(), st, ms, cnt, 32)
    assert ncat > 0, ncat
    torch.cuda.synchronize()
    got["profile"] = {L.mcq_profile_category_name(c).decode(): cnt[c] for c in range(ncat) if cnt[c]}
    print(f"CENSUS ({N}, {K}, {iters}): {got!r},")

    # results as well as counts: the compaction path and the other output form give the same codes
    assert torch.equal(codes_skip, codes) and torch.equal(codes64_skip, codes64)
    assert torch.equal(refined, codes64)             # the passes from the imported initial codes end where the encode ends
    if not wide and not (K == 16 and N >= 2):        # (16-entry codebooks leave as packed nibbles)
        assert torch.equal(codes.to(torch.int64), codes64)
    assert got == EXPECTED[(N, K, iters)]


def test_cross_check_by_reading():
    """8 x 256, 5 passes, below the skipping threshold, default flags: 1 limb conversion, 2 for the screened logits, 1 x.C
    product, 1 E / R launch for the first pass (one launch up to 8,192 vectors) and 4 per pass (stage 0, level 0, the fused
    level 1, the level-2 combine that also forms E / R of the next pass)"""
    assert EXPECTED[(8, 256, 5)]["encode"] == 1 + 2 + 1 + 1 + 4 * 5
