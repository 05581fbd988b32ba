"""Host-side checks of tests/skip_grid.py (no GPU): the constants it reads from the driver's source are where the GPU cases of
tests/test_gpu_skip_strided.py expect them, every case binds the cap of each kernel it names, and the mirror of the chunk
arithmetic agrees with the library's mcq_encode_workspace_bytes."""
import pytest

import skip_grid as sg


def test_constants_read_from_the_driver():
    c = sg.constants()
    assert c == dict(cap_stage0=32768, cap_wave=65536, skip_min_batch=8192, default_chunk_max=65536)


@pytest.mark.parametrize("case", sg.ALL, ids=lambda c: c.name)
def test_every_case_binds_the_caps_it_names(case):
    from quantization_amd import _lib
    c = sg.constants()
    per, _ = sg.ws_layout(_lib.lib(), case.N, case.K, case.D)
    chunk = case.chunk(per)
    smb = c["skip_min_batch"] if case.skip_min_batch is None else case.skip_min_batch
    skipping = [Bc for _, Bc in sg.chunks(case.B, chunk) if sg.skips(Bc, case.N, case.K, case.passes, smb)]
    capped = sg.capped_kernels(case.N, case.K)
    assert set(case.multi) <= set(case.binds)
    for k in case.binds:
        assert k in capped, (case.name, k, capped)
        assert case.passes >= 4 and any(sg.binds(k, Bc, case.N, case.K, c) for Bc in skipping), (case.name, k)
        if k in case.multi:     # reachable at all: the loop goes round twice when every vector of a chunk is active
            assert any(sg.strides(k, Bc, Bc, case.N, case.K, c) >= 2 for Bc in skipping), (case.name, k)
    if not case.binds:
        assert case.note or not skipping or case.passes < 4


def test_threshold_and_chunk_edges():
    """the threshold cases straddle skip_min_batch; the mixed-chunk cases put chunks on both sides of it"""
    c = sg.constants()
    smb = c["skip_min_batch"]
    by = {k.name: k for k in sg.ALL}
    assert [by[f"n16_k256_b{b}"].B - smb for b in (8191, 8192, 8193)] == [-1, 0, 1]
    assert not sg.binds("stage0", smb, 16, 256, c) and sg.binds("stage0", smb + 1, 16, 256, c)
    below = [Bc for _, Bc in sg.chunks(by["n32_mixed_8064"].B, sg.chunk_of(by["n32_mixed_8064"].B, 8064))]
    assert below and max(below) < smb
    at = [Bc for _, Bc in sg.chunks(by["n32_mixed_8192"].B, sg.chunk_of(by["n32_mixed_8192"].B, 8192))]
    assert at[:2] == [smb, smb] and 0 < at[-1] < smb
    from quantization_amd import _lib
    t = by["n32_k256_default_tail"]
    per, _ = sg.ws_layout(_lib.lib(), t.N, t.K, t.D)
    tail = [Bc for _, Bc in sg.chunks(t.B, t.chunk(per))]
    assert len(tail) == 2 and tail[0] >= smb and tail[-1] < smb
    big = [k for k in sg.BIG if k.ws is not None and k.ws > c["default_chunk_max"]]
    assert {(k.N, k.K) for k in big} >= {(1, 256), (2, 256), (32, 16)}


@pytest.mark.parametrize("N,K,D", [(1, 256, 40), (8, 256, 512), (16, 512, 64), (32, 256, 128), (64, 16, 64), (64, 256, 256)])
def test_chunk_mirror_matches_the_library(N, K, D):
    from quantization_amd import _lib
    L = _lib.lib()
    per, slack = sg.ws_layout(L, N, K, D)
    dc = sg.default_chunk(per, sg.constants()["default_chunk_max"])
    assert L.mcq_encode_workspace_bytes(10 ** 7, N, K, D) == slack + per * dc
    assert L.mcq_encode_workspace_bytes(dc - 1, N, K, D) == slack + per * (dc - 1)
    assert sg.ws_bytes(L, N, K, D, 3 * dc) == slack + 3 * per * dc
