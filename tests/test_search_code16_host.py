"""Host-side checks of the search over stores of two-byte codes (no GPU; include/mcq_code16.h rules 32-35): the seven entries
of the companion header are declared as _lib.CODE16_SIGNATURES binds them, exported, bound and disjoint from the other tables;
include/mcq.h keeps its 64 declarations and the ABI version stays 7; the one-byte entries go on answering MCQ_EUNSUPPORTED at
K = 512 and 1,024; every argument check of the new entries answers in search_check's order before anything touches the device
(fake pointers, no launch): the domain with 32 x 1,024 and 64 x 512 outside it, the cap of k, sizes, the metric, pointers, the
min(2 N, 16) alignment, a workspace one byte short; the size queries equal the mirrors of wide_plan and range_lists_plan and,
at K <= 256, the one-byte queries; Quantizer.pack_codes round trips and refuses digits outside [0, K); the argument errors of
the Python interface precede any device work; and the claims of the GPU case table hold, so that a kernel reading one byte per
digit could not pass it."""
import ctypes

import numpy as np
import pytest

import search_code16_grid as cg
import search_range_lists_grid as rl
import search_selection_grid as sel
import search_wide_grid as wg

NEW = ("mcq_search_tables_u16", "mcq_code_norms_u16", "mcq_search_topk_u16_workspace_bytes", "mcq_search_topk_u16",
       "mcq_search_range_u16_workspace_bytes", "mcq_search_range_u16_count", "mcq_search_range_u16_fill")
CODE16_HDR = sel.API.replace("quantization_amd/csrc/mcq_api.hip", "include/mcq_code16.h")
OUTSIDE = ((32, 1024), (64, 512), (64, 1024), (8, 2048), (8, 8), (128, 16))       # MCQ_EUNSUPPORTED (rule 33)
INVALID = ((3, 1024), (8, 300), (0, 512))                                        # MCQ_EINVAL


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(CODE16_HDR)
    assert tuple(hdr) == NEW == m.CODE16_SYMBOLS == tuple(m.CODE16_SIGNATURES)
    assert ab.mismatches(hdr, m.CODE16_SIGNATURES) == []
    for other in (m.SYMBOLS, m.RESIDUAL_SYMBOLS, m.PROBE_SYMBOLS, m.WIDE_SYMBOLS, m.RERANK_SYMBOLS):
        assert not set(NEW) & set(other)
    assert not set(NEW) & set(ab.header_signatures()) and len(ab.header_signatures()) == 64 == len(m.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == list(m.CODE16_SIGNATURES[name][1])
    text = open(CODE16_HDR).read()
    for rule in (" 32. ", " 33. ", " 34. ", " 35. "):
        assert rule in text
    assert '#include "mcq_rerank.h"' in text and L.mcq_abi_version() == 7
    doctored = dict(m.CODE16_SIGNATURES)                      # the comparison can fail: a long turned into an int
    r, args = doctored["mcq_search_topk_u16"]
    doctored["mcq_search_topk_u16"] = (r, args[:1] + (ctypes.c_int,) + args[2:])
    assert len(ab.mismatches(hdr, doctored)) == 1


def test_one_byte_entries_still_refuse_wide_codebooks():
    m = _lib()
    L = m.lib()
    U = m.MCQ_EUNSUPPORTED
    for N, K in ((8, 512), (8, 1024), (1, 1024), (32, 512)):
        assert L.mcq_search_tables(None, 0, 4, None, N, K, 64, None, None) == U
        assert L.mcq_code_norms(None, 4, None, N, K, 64, None, None) == U
        assert L.mcq_code_rnorms(None, 4, None, N, K, 64, None, None) == U
        assert L.mcq_search_scan(None, 4, None, None, 100, N, K, 10, None, None, None, 0, None) == U
        assert L.mcq_search_scan_lists(None, 4, None, None, 100, N, K, 10, 0, None, None, 3, None, 2, None, None, None, 0, None) == U
        assert L.mcq_search_range_count(None, 4, None, None, 100, N, K, 0, None, None, None, 0, None) == U
        assert L.mcq_search_wide(None, 4, None, None, 100, N, K, 300, 0, None, None, None, None, 0, None) == U
        assert L.mcq_search_wide_workspace_bytes(4, 100, N, K, 300) == 256


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    at = lambda o: ctypes.c_void_p((1 << 20) + o)
    big = (1 << 31) - 1

    def topk(tables=fake, Q=4, codes=fake, w=fake, B=1000, N=8, K=1024, k=10, metric=0, mask=None, off=None, Ls=0, probes=None,
             P=0, bias=None, outs=fake, ws=fake, ws_bytes=1 << 30):
        return L.mcq_search_topk_u16(tables, Q, codes, w, B, N, K, k, metric, mask, off, Ls, probes, P, bias, outs, outs, ws,
                                     ws_bytes, None)

    def count(tables=fake, Q=4, codes=fake, w=fake, B=1000, N=8, K=1024, k=None, metric=0, mask=None, off=None, Ls=0,
              probes=None, P=0, bias=None, outs=fake, thr=fake, ws=fake, ws_bytes=1 << 30):
        return L.mcq_search_range_u16_count(tables, Q, codes, w, B, N, K, metric, mask, off, Ls, probes, P, bias, thr, outs, ws,
                                            ws_bytes, None)

    def fill(tables=fake, Q=4, codes=fake, w=fake, B=1000, N=8, K=1024, k=None, metric=0, mask=None, off=None, Ls=0,
             probes=None, P=0, bias=None, outs=fake, thr=fake, ws=fake, ws_bytes=1 << 30, out=fake, capacity=100):
        return L.mcq_search_range_u16_fill(tables, Q, codes, w, B, N, K, metric, mask, off, Ls, probes, P, bias, thr, outs, out, out,
                                           capacity, ws, ws_bytes, None)

    nothing = dict(tables=None, codes=None, w=None, outs=None, ws=None, ws_bytes=0)
    lists = dict(off=fake, Ls=7, probes=fake, P=3)
    for f in (topk, count, fill):
        has_k = f is topk
        for li in (dict(), lists):
            # the domain first, before any pointer is looked at
            for N, K in OUTSIDE:
                assert f(N=N, K=K, Q=-1, metric=9, **nothing, **li) == U, (N, K)
            for N, K in INVALID:
                assert f(N=N, K=K, **li) == I, (N, K)
            for N, K in cg.SHAPES + cg.CROSS + ((16, 1024), (64, 256), (1, 16)):
                assert f(N=N, K=K, Q=-1, **li) == I, (N, K)                 # inside: the next check answers
            if has_k:
                for k in (1025, 1 << 20):
                    assert f(k=k, Q=-1, metric=9, **nothing, **li) == U      # the cap of k before the sizes
                for k in (0, -3):
                    assert f(k=k, **li) == I
                for k in (1, 64, 65, 1024):
                    assert f(k=k, Q=-1, **li) == I
            for neg in ("Q", "B"):
                assert f(**{neg: -1}, metric=9, **nothing, **li) == I
            assert f(Q=big + 1, **li) == I
            for metric in (-1, 3):
                assert f(metric=metric, B=big + 1, **li) == I               # the metric before the size of the store
            assert f(B=big + 1, **nothing, **li) == U
            assert f(outs=None, **li) == I
            # pointers, then w, then the alignments, then (range) thr, then the workspace
            for name in ("tables", "codes", "ws"):
                assert f(**{name: None}, **li) == I
            assert f(w=None, **li) == I and f(w=None, metric=2, **li) == I
            for mis in (2, 4, 8):
                assert f(codes=at(mis), **li) == I                          # 8 codebooks: 16 bytes
            assert f(mask=at(4), **li) == I
        assert f(off=fake, Ls=-1, probes=fake, P=3, **nothing) == I and f(off=fake, Ls=7, probes=fake, P=-1, **nothing) == I
        assert f(off=fake, Ls=7, probes=fake, P=4097, **nothing) == U
        assert f(off=None, Ls=7, probes=fake, P=3) == I
        assert f(off=at(4), Ls=7, probes=fake, P=3) == I and f(off=fake, Ls=7, probes=at(2), P=3) == I
        assert f(bias=at(2), **lists) == I
        # probes == NULL is the whole store: list_offsets, L, P and probe_bias are not looked at
        assert f(off=at(3), Ls=-5, probes=None, P=-1, bias=at(1), ws_bytes=0) == W
    # the alignment of rule 34: min(2 N, 16) bytes, and no more
    for N, K in ((1, 1024), (2, 1024), (4, 512), (8, 1024), (16, 1024), (32, 512), (64, 256)):
        need = min(2 * N, 16)
        for f in (topk, count, fill):
            for o in (1, 2, 4, 8, 16):
                assert f(N=N, K=K, codes=at(o), ws_bytes=0) == (W if o % need == 0 else I), (N, K, o)
    # the workspace, checked last: one byte short
    for N, K in cg.SHAPES:
        for P, li in ((1, dict()), (3, lists)):
            for metric in (0, 1, 2):
                for k in (1, 64, 65, 1024):
                    need = L.mcq_search_topk_u16_workspace_bytes(4, P, N, K, k)
                    assert need > 256 and topk(N=N, K=K, k=k, metric=metric, ws_bytes=need - 1, w=None if metric == 1 else fake, **li) == W
                need = L.mcq_search_range_u16_workspace_bytes(4, P, N, K)
                assert need > 256
                assert count(N=N, K=K, metric=metric, ws_bytes=need - 1, **li) == W
                assert fill(N=N, K=K, metric=metric, ws_bytes=need - 1, **li) == W
                assert count(N=N, K=K, metric=metric, thr=None, ws_bytes=need, **li) == I     # thr before the workspace
    # calls that do nothing: no queries (top-k), no room (fill); the limits still come first
    assert topk(Q=0, outs=None, tables=at(3), codes=at(3), ws=None, ws_bytes=0) == 0
    assert topk(Q=0, k=1025, **{k_: v for k_, v in nothing.items() if k_ != "outs"}) == U
    need = L.mcq_search_range_u16_workspace_bytes(4, 1, 8, 1024)
    assert fill(capacity=0, out=None, ws_bytes=need) == 0 and fill(capacity=-1, ws_bytes=need) == I
    assert fill(capacity=5, out=None, ws_bytes=need) == I
    # tables and norms
    for N, K in OUTSIDE:
        assert L.mcq_search_tables_u16(None, 0, -1, None, N, K, 64, None, None) == U
        assert L.mcq_code_norms_u16(None, -1, None, N, K, 64, 0, None, 0, None, None, None) == U
    assert L.mcq_search_tables_u16(None, 0, 4, None, 8, 1024, 16385, None, None) == U
    for N, K in INVALID:
        assert L.mcq_search_tables_u16(fake, 0, 4, fake, N, K, 64, fake, None) == I
        assert L.mcq_code_norms_u16(fake, 4, fake, N, K, 64, 0, None, 0, None, fake, None) == I
    assert L.mcq_search_tables_u16(fake, 0, -1, fake, 8, 1024, 64, fake, None) == I
    assert L.mcq_search_tables_u16(None, 0, 0, None, 8, 1024, 64, None, None) == 0
    for missing in range(3):
        ptrs = [fake, fake, fake]
        ptrs[missing] = None
        assert L.mcq_search_tables_u16(ptrs[0], 0, 4, ptrs[1], 8, 1024, 64, ptrs[2], None) == I
        assert L.mcq_code_norms_u16(ptrs[0], 4, ptrs[1], 8, 1024, 64, 1, None, 0, None, ptrs[2], None) == I
    for rnorm in (0, 1):
        assert L.mcq_code_norms_u16(fake, -1, fake, 8, 1024, 64, rnorm, None, 0, None, fake, None) == I
        assert L.mcq_code_norms_u16(fake, big + 1, fake, 8, 1024, 64, rnorm, None, 0, None, fake, None) == U
        assert L.mcq_code_norms_u16(None, 0, None, 8, 1024, 64, rnorm, None, 0, None, None, None) == 0
        assert L.mcq_code_norms_u16(fake, 4, fake, 8, 1024, 64, rnorm, fake, -1, fake, fake, None) == I
        assert L.mcq_code_norms_u16(fake, 4, fake, 8, 1024, 64, rnorm, fake, 3, None, fake, None) == I      # base without assign
        assert L.mcq_code_norms_u16(fake, 4, fake, 8, 1024, 64, rnorm, None, 3, fake, fake, None) == I
        assert L.mcq_code_norms_u16(fake, 4, fake, 8, 1024, 64, rnorm, at(2), 3, fake, fake, None) == I
        assert L.mcq_code_norms_u16(at(1), 4, fake, 8, 1024, 64, rnorm, None, 0, None, fake, None) == I     # two-byte elements


def test_size_queries_equal_the_mirrors():
    m = _lib()
    L = m.lib()
    c, rc = wg.constants(), rl.constants()
    for N, K in cg.SHAPES + cg.CROSS:
        for Q in (1, 5, 17, 64, 1024, 5000):
            for P in (1, 7, 4096):
                for k in (1, 10, 64, 65, 512, 513, 1024):
                    plan = wg.wide_plan(Q, P, N, K, k, c)
                    assert L.mcq_search_topk_u16_workspace_bytes(Q, P, N, K, k) == plan.ws_bytes, (Q, P, N, K, k)
                    assert plan.lds <= 160 * 1024
                    if K <= 256:
                        assert L.mcq_search_wide_lists_workspace_bytes(Q, P, N, K, k) == plan.ws_bytes
                plan = rl.range_lists_plan(Q, P, N, K, rc)
                assert L.mcq_search_range_u16_workspace_bytes(Q, P, N, K) == plan.ws_bytes and plan.lds <= 160 * 1024
                if K <= 256:
                    assert L.mcq_search_range_lists_workspace_bytes(Q, P, N, K) == plan.ws_bytes
    assert wg.wide_plan(1, 4096, 16, 1024, 1024, c).lds == wg.wide_plan(1, 4096, 64, 256, 1024, c).lds      # the largest request is the old one
    for bad in ((0, 1, 8, 1024, 10), (-1, 1, 8, 1024, 10), (4, 0, 8, 1024, 10), (4, 4097, 8, 1024, 10), (4, 1, 8, 1024, 0),
                (4, 1, 8, 1024, 1025), (4, 1, 32, 1024, 10), (4, 1, 64, 512, 10), (4, 1, 3, 1024, 10), (1 << 31, 1, 8, 1024, 10)):
        assert L.mcq_search_topk_u16_workspace_bytes(*bad) == 256, bad
        assert L.mcq_search_range_u16_workspace_bytes(*bad[:4]) == 256 or bad[4] in (0, 1025)


def test_pack_codes():
    import torch
    _lib()
    from quantization_amd import Quantizer
    for K, dtype in ((1024, torch.int16), (512, torch.int16), (256, torch.uint8), (16, torch.uint8)):
        q = Quantizer(24, K, 4)
        d = torch.from_numpy(np.random.RandomState(K).randint(0, K, size=(3, 5, 4)))
        d[0, 0, 0], d[0, 0, 1] = K - 1, 0
        packed = q.pack_codes(d)
        assert packed.dtype == dtype and tuple(packed.shape) == (3, 5, 4) and packed.is_contiguous()
        assert torch.equal(packed.to(torch.int64), d)
        assert torch.equal(q.pack_codes(d.to(torch.int32)), packed) and torch.equal(q.pack_codes(packed), packed)
        assert q.pack_codes(d[:0]).shape == (0, 5, 4)
        for bad in (K, -1):
            wrong = d.clone()
            wrong[2, 4, 3] = bad
            with pytest.raises(ValueError, match="digits outside"):
                q.pack_codes(wrong)
        for wrong in (d.float(), d[..., :3], d > 0, [[1, 2, 3, 4]]):
            with pytest.raises(ValueError, match="pack_codes"):
                q.pack_codes(wrong)
    assert packed.element_size() == 1 and Quantizer(24, 1024, 4).pack_codes(d % 1024).element_size() == 2


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    from quantization_amd import Quantizer, search
    q = Quantizer(24, 1024, 4)
    B = 130
    codes, x = torch.zeros(B, 4, dtype=torch.int16), torch.zeros(3, 24)
    off = torch.tensor([0, 50, 130], dtype=torch.int64)
    probes = torch.zeros(3, 2, dtype=torch.int32)
    calls = (lambda **kw: q.search(x, codes, **kw), lambda **kw: q.search_wide(x, codes, 300, **kw),
             lambda **kw: q.search_lists(x, codes, off, probes, **kw), lambda **kw: q.search_lists_wide(x, codes, off, probes, 300, **kw),
             lambda **kw: q.range_search(x, codes, 1.0, **kw), lambda **kw: q.range_search_lists(x, codes, off, probes, 1.0, **kw))
    for call in calls:
        with pytest.raises(m.McqError, match="HIP device"):       # CPU tensors: no fallback
            call()
        with pytest.raises(ValueError):
            call(metric="dot")
        with pytest.raises(ValueError, match="mask"):
            call(mask=torch.zeros(B - 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="probe_bias"):
        q.search_lists(x, codes, off, probes, probe_bias=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="probes"):
        q.range_search_lists(x, codes, off, probes[:2], 1.0)
    # one-byte codes are refused with the way out, whatever the device; so are other dtypes and other widths
    for wrong in (codes.to(torch.uint8), codes.to(torch.int32), codes.float()):
        for call in (lambda c: q.search(x, c), lambda c: q.range_search(x, c, 1.0), lambda c: q.code_norms(c), lambda c: q.code_rnorms(c),
                     lambda c: q.search_lists_wide(x, c, off, probes, 300)):
            with pytest.raises(m.McqError, match="pack_codes"):
                call(wrong)
    with pytest.raises(m.McqError, match="4 codebooks"):
        q.code_norms(codes[:, :3])
    with pytest.raises(m.McqError, match="HIP device"):
        q.code_norms(codes.to(torch.int64))                          # int64 digits pass the dtype check: narrowed per call
    # N * K past 16,384: McqError naming the limit, from every call
    wide = Quantizer(24, 1024, 32)
    for call in (lambda: wide.search(x, torch.zeros(B, 32, dtype=torch.int16)), lambda: wide.search_tables(x),
                 lambda: wide.code_norms(torch.zeros(B, 32, dtype=torch.int16)),
                 lambda: wide.range_search(x, torch.zeros(B, 32, dtype=torch.int16), 1.0)):
        with pytest.raises(m.McqError, match="16,384"):
            call()
    assert search.CODE16_MAX_ROWS == cg.MAX_ROWS == 16384


def test_case_table_claims():
    shapes = {(x.N, x.K) for x in cg.CASES}
    assert shapes == set(cg.SHAPES) and {x.ch for x in cg.CASES} == {1, 2, 4, 8}
    assert {x.N // x.ch for x in cg.CASES} >= {1, 2, 4}                             # one, two and four chunks per row
    assert {x.B for x in cg.CASES} == {0, 1, 63, 64, 65, 4099} and {x.Q for x in cg.CASES} == {1, 5, 17}
    assert {x.D for x in cg.CASES} == {24, 40} and {x.k for x in cg.CASES} == {1, 10, 64, 65, 300, 1024}
    assert all(x.N * x.K <= cg.MAX_ROWS and x.B <= 20_000 for x in cg.CASES)
    assert set(cg.METRICS) == {"l2", "ip", "cosine"} and None in cg.MASKS and len(cg.MASKS) > 1
    import search_metric_grid as mg
    every = [x for x in cg.CASES + [cg.MASK_CASE] + [x for x, _ in cg.HIGH_BITS]]
    for x in every:
        if x.K <= 256 or x.B < 2:
            continue
        d = cg.digits(x.N, x.K, x.B)
        assert d.min() >= 0 and d.max() < x.K and cg.store(d).dtype == np.int16
        assert all(cg.claims(d, x.K).values()), (x.name, cg.claims(d, x.K))
        # a kernel that kept the low byte of every digit would return something else
        rs = np.random.RandomState(x.N + x.K)
        T = rs.randn(min(x.Q, 3), x.N, x.K).astype(np.float32)
        w = rs.rand(x.B).astype(np.float32)
        for metric in cg.METRICS:
            s = mg.restate_metric_scores(T, w, d, metric)
            low = mg.restate_metric_scores(T, w, d & 255, metric)
            a, b = wg.restate_topk_valid(s, x.k), wg.restate_topk_valid(low, x.k)
            assert not (np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))), (x.name, metric)
            if metric == "ip":                                                      # the twins of digits()
                assert (s[:, 0] != s[:, 1]).all() and (low[:, 0] == low[:, 1]).all()
    for x, bits in cg.HIGH_BITS:
        d = cg.digits(x.N, x.K, x.B)
        hb = cg.with_high_bits(d, bits)
        assert hb.dtype == np.int16 and (hb < 0).all() and np.array_equal(hb.astype(np.int64) & (x.K - 1), d)
        assert bits & (x.K - 1) == 0 and (bits | (x.K - 1)) == 0xFFFF
