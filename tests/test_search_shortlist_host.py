"""Host-side checks of the search over a shortlist (no GPU; include/mcq_shortlist.h rules 36-39): the three entries of the
companion header are declared as _lib.SHORTLIST_SIGNATURES binds them, exported, bound and disjoint from the six other tables;
include/mcq.h keeps its 64 declarations and the ABI version stays 7; every argument check of both entries answers in the
documented order before anything touches the device (fake pointers, no launch); the size query and the mirror of short_plan
(tests/search_shortlist_grid.py) agree over the domain and outside it; the numpy restatement equals a plain double loop bit for
bit, and with a deduplicated shortlist equals search_mask_grid.restate_topk_masked with the shortlist's bits; the claims of the
GPU case table hold; and the argument errors of the Python interface precede any device work."""
import ctypes

import numpy as np
import pytest

import search_mask_grid as kg
import search_metric_grid as mg
import search_selection_grid as sel
import search_shortlist_grid as hg

NEW = ("mcq_search_shortlist_workspace_bytes", "mcq_search_shortlist", "mcq_search_shortlist_u16")
SHORT_HDR = sel.API.replace("quantization_amd/csrc/mcq_api.hip", "include/mcq_shortlist.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(SHORT_HDR)
    assert tuple(hdr) == NEW == m.SHORTLIST_SYMBOLS == tuple(m.SHORTLIST_SIGNATURES)
    assert ab.mismatches(hdr, m.SHORTLIST_SIGNATURES) == []
    others = (m.SYMBOLS, m.RESIDUAL_SYMBOLS, m.PROBE_SYMBOLS, m.WIDE_SYMBOLS, m.RERANK_SYMBOLS, m.CODE16_SYMBOLS)
    for other in others:
        assert not set(NEW) & set(other)
    assert not set(NEW) & set(ab.header_signatures()) and len(ab.header_signatures()) == 64 == len(m.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == list(m.SHORTLIST_SIGNATURES[name][1])
    text = open(SHORT_HDR).read()
    for rule in (" 36. ", " 37. ", " 38. ", " 39. "):
        assert rule in text
    assert '#include "mcq_code16.h"' in text and L.mcq_abi_version() == 7
    doctored = dict(m.SHORTLIST_SIGNATURES)                   # the comparison can fail: a long turned into an int
    r, args = doctored["mcq_search_shortlist"]
    assert args[10] is ctypes.c_long
    doctored["mcq_search_shortlist"] = (r, args[:10] + (ctypes.c_int,) + args[11:])
    assert len(ab.mismatches(hdr, doctored)) == 1
    c = hg.constants()
    assert hg.NS == tuple(hg.wg.wide_pick_lists()) and c["kShortStep"] == 64


@pytest.mark.parametrize("two", (False, True), ids=("u8", "u16"))
def test_argument_validation_without_launch(two):
    m = _lib()
    L = m.lib()
    entry = L.mcq_search_shortlist_u16 if two else L.mcq_search_shortlist
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 3)
    at = lambda o: ctypes.c_void_p((1 << 20) + o)
    big = (1 << 31) - 1

    def f(tables=fake, Q=4, codes=fake, w=fake, B=1000, N=8, K=256, k=10, metric=0, short=fake, S=100, row_of=None, Bs=0,
          bias=None, outs=fake, ws=fake, ws_bytes=1 << 30):
        return entry(tables, Q, codes, w, B, N, K, k, metric, short, S, row_of, Bs, bias, outs, outs, ws, ws_bytes, None)

    need = lambda k=10, N=8, K=256: L.mcq_search_shortlist_workspace_bytes(4, 100, N, K, k)
    nothing = dict(tables=None, codes=None, w=None, short=None, outs=None, ws=None, ws_bytes=0)
    for row_of, Bs in ((None, -5), (fake, 1000)):
        ro = dict(row_of=row_of, Bs=Bs)
        # the shape and k first, before any pointer is looked at
        for N, K in ((128, 16), (8, 2048), (8, 8), (64, 512), (32, 1024)):
            assert f(N=N, K=K, k=0, Q=-1, metric=9, **nothing, **ro) == U
        for N, K in ((3, 256), (8, 100), (0, 256), (-2, 256)):
            assert f(N=N, K=K, k=0, Q=-1, metric=9, **nothing, **ro) == I
        assert f(N=8, K=1024, **ro, ws_bytes=need(10, 8, 1024) - 1) == (W if two else U)       # rule 33 against rule 5
        assert f(N=16, K=512, **ro, ws_bytes=need(10, 16, 512) - 1) == (W if two else U)
        for k in (1025, 1 << 20):
            assert f(k=k, Q=-1, metric=9, **nothing, **ro) == U
        for k in (0, -3):
            assert f(k=k, metric=9, Q=big, **ro) == I
        for neg in ("Q", "S", "B"):
            assert f(**{neg: -1}, metric=9, **nothing, **ro) == I
        for metric in (-1, 3):
            assert f(metric=metric, Q=big, **ro) == I         # the metric before the large sizes
        for name in ("Q", "S", "B"):
            assert f(**{name: big}, **nothing, **ro) == U
            assert f(**{name: 1 << 40}, **nothing, **ro) == U
        assert f(outs=None, **ro) == I                        # missing outputs
        # no queries: 0, and no input is looked at; the limits still come first
        assert f(Q=0, tables=odd, codes=odd, w=odd, short=odd, bias=odd, outs=None, ws=None, ws_bytes=0, **ro) == 0
        assert f(Q=0, k=1025, **nothing, **ro) == U
        # the pointers, then the alignments, then the workspace
        for name in ("tables", "codes", "short", "ws"):
            assert f(**{name: None}, ws_bytes=need(), **ro) == I
        assert f(w=None, **ro) == I and f(w=None, metric=2, **ro) == I
        assert f(w=None, metric=1, ws_bytes=need() - 1, **ro) == W                      # the inner product never reads w
        assert f(codes=at(8 if two else 4), **ro) == I        # 8 digits: 8 bytes, or 16
        assert f(codes=at(8 if two else 4), N=4 if two else 4, **ro, ws_bytes=need(10, 4) - 1) == W
        assert f(codes=at(16), N=64, **ro, ws_bytes=need(10, 64) - 1) == W
        assert f(codes=at(8), N=64, **ro) == I
        assert f(short=at(4), **ro) == I and f(bias=at(2), **ro) == I
        assert f(bias=at(4), ws_bytes=need() - 1, **ro) == W
        for k in (1, 10, 64, 65, 1024):
            for N, K in hg.ONE_BYTE + (hg.TWO_BYTE if two else ()):
                for metric in (0, 1, 2):
                    assert f(N=N, K=K, k=k, metric=metric, ws_bytes=need(k, N, K) - 1, **ro) == W
                assert need(k, N, K) > 256
    assert f(row_of=fake, Bs=-1, **nothing) == I
    assert f(row_of=fake, Bs=big, **nothing) == U
    assert f(row_of=at(4), Bs=1000) == I and f(row_of=at(4), Bs=1000, ws_bytes=0) == I      # alignment before the workspace
    assert f(row_of=None, Bs=big, ws_bytes=need() - 1) == W   # Bs is not looked at without row_of
    # a call whose rows cannot hold a candidate needs its outputs and looks at nothing else (with them the fill is a launch)
    for kw in (dict(S=0), dict(B=0), dict(row_of=fake, Bs=0)):
        assert f(tables=odd, codes=odd, w=None, short=odd, bias=odd, outs=None, ws=None, ws_bytes=0, **kw) == I


def test_size_query_equals_the_mirror():
    m = _lib()
    L = m.lib()
    c = hg.constants()
    shapes = [(x.Q, x.S, x.N, x.K, x.k) for x in hg.CASES if x.S > 0] + \
             [(1, 1, 1, 16, 1), (1, 1000, 8, 256, 10), (64, 1000, 8, 256, 10), (64, 1000, 64, 256, 100), (1024, 1000, 8, 256, 100),
              (64, 100, 8, 256, 10), (1, 64, 64, 256, 1024), (1, 65, 16, 1024, 1024), (5000, 1 << 20, 2, 256, 513),
              (3, (1 << 31) - 2, 8, 256, 512)]
    for Q, S, N, K, k in shapes:
        plan = hg.short_plan(Q, S, N, K, k, c)
        assert L.mcq_search_shortlist_workspace_bytes(Q, S, N, K, k) == plan.ws_bytes, (Q, S, N, K, k)
        assert 1 <= plan.parts <= max(1, min(plan.steps, c["kWideMergeEntries"] // hg.wg.wide_half(k, c)))
        assert plan.lds <= 160 * 1024
        assert all(hi > lo for lo, hi in hg.part_steps(plan.steps, plan.parts))                # no part without a step
    assert hg.short_plan(1, 1000, 64, 256, 1024, c).lds == 64 * 1024 + 16 * 1024 + 64           # the largest LDS request
    assert hg.short_plan(64, 1000, 8, 256, 10, c).parts == 16 == hg.short_plan(1, 1000, 8, 256, 10, c).parts   # ceil(1000 / 64) steps
    assert hg.short_plan(1024, 1000, 8, 256, 10, c).parts == 1 and hg.short_plan(1, 100000, 8, 256, 1024, c).parts == 64
    assert L.mcq_search_shortlist_workspace_bytes(4, 100, 1, 16, 10) == L.mcq_search_shortlist_workspace_bytes(4, 100, 64, 256, 10)
    for bad in ((0, 100, 8, 256, 10), (4, 0, 8, 256, 10), (-1, 100, 8, 256, 10), (4, -1, 8, 256, 10), (4, 100, 3, 256, 10),
                (4, 100, 8, 2048, 10), (4, 100, 64, 512, 10), (4, 100, 8, 256, 0), (4, 100, 8, 256, 1025),
                ((1 << 31) - 1, 100, 8, 256, 10), (4, (1 << 31) - 1, 8, 256, 10)):
        assert L.mcq_search_shortlist_workspace_bytes(*bad) == 256, bad


def _plain(T, w, codes, short, k, metric, row_of, bias):
    """rules 36-38 as a double loop over queries and slots, one numpy float32 operation at a time"""
    f = np.float32
    Q, S = short.shape
    B, N = codes.shape
    K = T.shape[2]
    Bs = B if row_of is None else len(row_of)
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(Q):
            found = []
            for j in range(S):
                p = int(short[q, j])
                if not 0 <= p < Bs:
                    continue
                r = p if row_of is None else int(row_of[p])
                if not 0 <= r < B:
                    continue
                acc = f(-0.0)
                for n in range(N):
                    acc = f(acc + T[q, n, int(codes[r, n]) & (K - 1)])
                acc = f(acc + (f(-0.0) if bias is None else bias[q, j]))
                s = f(acc + w[r]) if metric == "l2" else (f(acc * w[r]) if metric == "cosine" else acc)
                if not np.isnan(s):
                    found.append((s, p))
            found.sort(key=lambda e: (e[0], e[1]))            # (-0.0 == +0.0 as python floats: position decides)
            for e, (s, p) in enumerate(found[:k]):
                out_s[q, e], out_i[q, e] = s, p
    return out_s, out_i


def test_restatement_against_a_plain_double_loop():
    rs = np.random.RandomState(4)
    for (N, K), two in (((8, 256), False), ((4, 16), False), ((2, 1024), True)):
        Q, B, S = 3, 40, 50
        T = rs.standard_normal((Q, N, K)).astype(np.float32)
        codes = rs.randint(0, K, size=(B, N)).astype(np.uint16 if two else np.uint8)
        w = (rs.rand(B) * 4).astype(np.float32)
        w[5] = np.nan
        w[6] = np.inf
        short = rs.randint(-3, B + 3, size=(Q, S)).astype(np.int64)      # duplicates, and entries on both sides of [0, B)
        short[0, :4] = (B, 2 ** 40, -7, np.iinfo(np.int64).min)
        row_of = rs.randint(-2, B + 2, size=B + 7).astype(np.int64)
        bias = rs.standard_normal((Q, S)).astype(np.float32)
        bias[0, 7] = -0.0
        for metric in hg.METRICS:
            for ro in (None, row_of):
                for bi in (None, bias):
                    for k in (1, 10, 64):
                        got = hg.restate(T, w, codes, short, k, metric, ro, bi)[:2]
                        want = _plain(T, w, codes, short, k, metric, ro, bi)
                        assert np.array_equal(got[1], want[1]), (N, K, metric, k)
                        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (N, K, metric, k)
    neg = np.full((Q, S), -0.0, dtype=np.float32)             # a bias of -0.0 is no bias
    a, b = hg.restate(T, w, codes, short, 10, "l2", None, neg)[:2], hg.restate(T, w, codes, short, 10, "l2")[:2]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def test_deduplicated_shortlist_equals_the_masked_restatement():
    rs = np.random.RandomState(5)
    N, K, Q, B, S = 8, 256, 4, 300, 90
    T = rs.standard_normal((Q, N, K)).astype(np.float32)
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    w = (rs.rand(B) * 4).astype(np.float32)
    for metric in hg.METRICS:
        s = mg.restate_metric_scores(T, None if metric == "ip" else w, codes, metric)
        for q in range(Q):
            short = rs.permutation(B + 20)[:S].astype(np.int64) - 10      # distinct; some outside [0, B)
            keep = np.zeros(B, dtype=bool)
            keep[short[(short >= 0) & (short < B)]] = True
            for k in (1, 10, 100):
                got = hg.restate(T[q:q + 1], w, codes, short[None, :], k, metric)[:2]
                want = kg.restate_topk_masked(s[q:q + 1], keep, k)
                assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def test_claims_of_the_gpu_cases():
    c = hg.constants()
    seen = set()
    for x in hg.CASES:
        T, w, codes, short, row_of, bias = hg.make(x)
        assert T.shape == (x.Q, x.N, x.K) and codes.shape == (x.B, x.N) and short.shape == (x.Q, x.S) and x.B <= 4099
        assert codes.dtype == (np.uint16 if x.two else np.uint8) and (bias is None or bias.shape == short.shape)
        got = hg.reach(x, short, row_of, c)
        assert got == {f: getattr(x, f) for f in got}, (x.name, got)
        seen |= {f for f, v in got.items() if v}
        Bs = x.B if row_of is None else len(row_of)
        if x.short == "pad":
            assert (short[x.Q // 2] == -1).all() and (short[0, -1] == -1) and short[0, x.S // 2] == -1 and short[0, 0] >= 0
        if x.short == "junk":
            assert {Bs, 2 ** 40, -7, np.iinfo(np.int64).min} <= set(short.ravel().tolist())
        if x.short == "dups":
            assert all(len(set(r.tolist())) < x.S for r in short)
        if x.row_of == "perm_bad":
            pos, _ = hg.rg.candidates(short, x.B, row_of)
            assert Bs != x.B and ((row_of < 0) | (row_of >= x.B)).any() and ((pos < 0) & (short >= 0) & (short < Bs)).any()
        if x.bias == "random":
            assert (bias < 0).any() and (bias == 0).any() and np.signbit(bias[0, 0]) and bias[0, 0] == 0
    assert seen == {"parts", "one_part", "rounds", "short_row", "empty_row", "all_enter", "ragged"}
    assert {(x.N, x.K) for x in hg.CASES} >= set(hg.ONE_BYTE) | set(hg.TWO_BYTE)
    assert {x.S for x in hg.CASES} >= {0, 1, 63, 64, 65, 255, 256, 257, 1000}
    assert {x.k for x in hg.CASES} >= {1, 10, 64, 65, 300, 1024} and {x.Q for x in hg.CASES} >= {1, 5, 70}
    assert any(x.k < x.S for x in hg.CASES) and any(x.k > x.S for x in hg.CASES) and any(x.k == x.S for x in hg.CASES)
    assert any(x.one_part and x.Q > 500 and x.S > 64 for x in hg.CASES)
    assert {x.metric for x in hg.CASES} == set(hg.METRICS)
    assert {x.row_of for x in hg.CASES} == {None, "perm", "perm_bad", "arange"} and {x.bias for x in hg.CASES} == {None, "random", "negzero"}
    for metric in hg.METRICS:
        assert any(x.metric == metric and x.two for x in hg.CASES)


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    from quantization_amd import Quantizer
    quant = Quantizer(24, 256, 4)
    wide = Quantizer(24, 1024, 4)
    q, codes = torch.zeros(3, 24), torch.zeros(50, 4, dtype=torch.uint8)
    short = torch.zeros(3, 7, dtype=torch.int64)
    order = torch.arange(50)
    for k in (1, 10, 1024):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            quant.search_shortlist(q, codes, short, k)
        with pytest.raises(m.McqError):
            quant.search_shortlist(q.half(), codes, short.int(), k, metric="cosine", row_of=order, bias=torch.zeros(3, 7))
    with pytest.raises(ValueError, match="metric"):
        quant.search_shortlist(q, codes, short, 10, metric="dot")
    for k in (0, 1025, -1, 2.0, True):
        with pytest.raises(ValueError, match="k ="):
            quant.search_shortlist(q, codes, short, k)
    with pytest.raises(ValueError, match="queries"):
        quant.search_shortlist(torch.zeros(3, 23), codes, short, 10)
    with pytest.raises(ValueError, match="shortlist"):
        quant.search_shortlist(q, codes, short[:2], 10)
    with pytest.raises(ValueError, match="shortlist"):
        quant.search_shortlist(q, codes, short.float(), 10)
    with pytest.raises(ValueError, match="shortlist"):
        quant.search_shortlist(q.reshape(3, 1, 24), codes, short, 10)
    with pytest.raises(ValueError, match="row_of"):
        quant.search_shortlist(q, codes, short, 10, row_of=order.int())
    with pytest.raises(ValueError, match="row_of"):
        quant.search_shortlist(q, codes, short, 10, row_of=order.reshape(5, 10))
    with pytest.raises(ValueError, match="bias"):
        quant.search_shortlist(q, codes, short, 10, bias=torch.zeros(3, 8))
    with pytest.raises(ValueError, match="bias"):
        quant.search_shortlist(q, codes, short, 10, bias=torch.zeros(3, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="pack_codes"):
        wide.search_shortlist(q, codes, short, 10)
