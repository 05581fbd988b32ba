"""Host-side checks of the exact re-ranking of a shortlist (no GPU; include/mcq_rerank.h rules 28-31): the two entries of the
companion header are declared as _lib.RERANK_SIGNATURES binds them, exported, bound and disjoint from the other tables;
include/mcq.h keeps its 64 declarations and the ABI version stays 7; every argument check of mcq_rerank answers in the
documented order before anything touches the device (fake pointers, no launch), on both sides of k = 1,024 and D = 16,384; the
size query and the mirror of rerank_plan (tests/rerank_grid.py) agree; the numpy restatement of rule 29 equals a plain
per-element loop bit for bit and lies within the derived bound of the float64 value; the claims of the GPU case table hold; and
the argument errors of the Python interface precede any device work."""
import ctypes

import numpy as np
import pytest

import rerank_grid as rg
import search_selection_grid as sel

NEW = ("mcq_rerank_workspace_bytes", "mcq_rerank")
RERANK_HDR = sel.API.replace("quantization_amd/csrc/mcq_api.hip", "include/mcq_rerank.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(RERANK_HDR)
    assert tuple(hdr) == NEW == m.RERANK_SYMBOLS == tuple(m.RERANK_SIGNATURES)
    assert ab.mismatches(hdr, m.RERANK_SIGNATURES) == []
    for other in (m.SYMBOLS, m.RESIDUAL_SYMBOLS, m.PROBE_SYMBOLS, m.WIDE_SYMBOLS):
        assert not set(NEW) & set(other)
    assert not set(NEW) & set(ab.header_signatures()) and len(ab.header_signatures()) == 64 == len(m.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == list(m.RERANK_SIGNATURES[name][1])
    text = open(RERANK_HDR).read()
    for rule in (" 28. ", " 29. ", " 30. ", " 31. "):
        assert rule in text
    assert '#include "mcq_wide.h"' in text and L.mcq_abi_version() == 7
    doctored = dict(m.RERANK_SIGNATURES)                      # the comparison can fail: a long turned into an int
    r, args = doctored["mcq_rerank"]
    doctored["mcq_rerank"] = (r, args[:2] + (ctypes.c_int,) + args[3:])
    assert len(ab.mismatches(hdr, doctored)) == 1
    import sys
    import quantization_amd
    mod = sys.modules["quantization_amd.rerank"]             # (the package attribute of that name is the function)
    assert quantization_amd.rerank is mod.rerank and "rerank" in quantization_amd.__all__
    assert mod.MAX_DIM == rg.constants()["kRerankMaxD"]


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 3)
    at = lambda o: ctypes.c_void_p((1 << 20) + o)
    big = (1 << 31) - 1

    def f(q=fake, qh=0, Q=4, x=fake, xh=0, B=1000, D=64, short=fake, S=100, row_of=None, Bs=0, k=10, metric=0, outs=fake,
          ws=fake, ws_bytes=1 << 30):
        return L.mcq_rerank(q, qh, Q, x, xh, B, D, short, S, row_of, Bs, k, metric, outs, outs, ws, ws_bytes, None)

    need = lambda k=10, D=64: L.mcq_rerank_workspace_bytes(4, 100, D, k)
    nothing = dict(q=None, x=None, short=None, outs=None, ws=None, ws_bytes=0)
    for row_of, Bs in ((None, -5), (fake, 1000)):
        ro = dict(row_of=row_of, Bs=Bs)
        # the domain first, before any pointer is looked at: both sides of D = 16,384 and of k = 1,024
        for D, k in ((16385, 10), (1 << 20, 10), (64, 1025), (64, 1 << 20), (16385, 0), (0, 1025)):
            assert f(D=D, k=k, Q=-1, metric=9, **nothing, **ro) == U
        for D, k in ((0, 10), (-4, 10), (64, 0), (64, -3)):
            assert f(D=D, k=k, metric=9, **ro) == I
        for neg in ("Q", "S", "B"):
            assert f(**{neg: -1}, metric=9, **nothing, **ro) == I
        for metric in (-1, 3):
            assert f(metric=metric, Q=big, **ro) == I         # the metric before the large sizes
        for name in ("Q", "S", "B"):
            assert f(**{name: big}, **nothing, **ro) == U
            assert f(**{name: 1 << 40}, **nothing, **ro) == U
        assert f(outs=None, **ro) == I                        # missing outputs
        # no queries: 0, and no input is looked at; the limits still come first
        assert f(Q=0, q=odd, x=odd, short=odd, outs=None, ws=None, ws_bytes=0, **ro) == 0
        assert f(Q=0, k=1025, **nothing, **ro) == U
        # the pointers, then the alignments, then the workspace
        for name in ("q", "x", "short", "ws"):
            assert f(**{name: None}, ws_bytes=need(), **ro) == I
        assert f(q=at(2), **ro) == I and f(x=at(2), **ro) == I and f(q=at(1), qh=1, **ro) == I and f(x=at(3), xh=1, **ro) == I
        assert f(short=at(4), **ro) == I
        for k in (1, 10, 1024):
            for D in (1, 64, 16384):
                for metric in (0, 1, 2):
                    for qh, xh in ((0, 0), (1, 0), (0, 1), (1, 1)):
                        # element alignment is all queries and vectors need
                        assert f(q=at(2 if qh else 4), qh=qh, x=at(2 if xh else 4), xh=xh, k=k, D=D, metric=metric,
                                 ws_bytes=need(k, D) - 1, **ro) == W
                assert need(k, D) > 256
    assert f(row_of=fake, Bs=-1, **nothing) == I
    assert f(row_of=fake, Bs=big, **nothing) == U
    assert f(row_of=at(4), Bs=1000) == I and f(row_of=at(4), Bs=1000, ws_bytes=0) == I      # alignment before the workspace
    assert f(row_of=None, Bs=big, ws_bytes=need() - 1) == W   # Bs is not looked at without row_of
    # a call whose rows cannot hold a candidate needs its outputs and looks at nothing else (with them the fill is a launch)
    for kw in (dict(S=0), dict(B=0), dict(row_of=fake, Bs=0)):
        assert f(q=odd, x=odd, short=odd, outs=None, ws=None, ws_bytes=0, **kw) == I


def test_size_query_equals_the_mirror():
    m = _lib()
    L = m.lib()
    c = rg.constants()
    shapes = [(x.Q, x.S, x.D, x.k) for x in rg.CASES if x.S > 0] + \
             [(1, 1, 1, 1), (1, 1000, 512, 10), (64, 1000, 512, 10), (64, 1000, 512, 100), (1024, 1000, 512, 100), (64, 100, 512, 10),
              (1, 16, 16384, 1024), (1, 17, 16384, 1024), (5000, 1 << 20, 7, 513), (3, (1 << 31) - 2, 64, 512)]
    for Q, S, D, k in shapes:
        plan = rg.rerank_plan(Q, S, D, k, c)
        assert L.mcq_rerank_workspace_bytes(Q, S, D, k) == plan.ws_bytes, (Q, S, D, k)
        assert 1 <= plan.parts <= max(1, min(plan.steps, c["kWideMergeEntries"] // rg.wg.wide_half(k, c)))
        assert plan.lds <= 160 * 1024
        assert all(hi > lo for lo, hi in rg.part_steps(plan.steps, plan.parts))              # no part without a step
    assert rg.rerank_plan(1, 1000, 16384, 1024, c).lds == 64 * 1024 + 16 * 1024 + 64          # the largest LDS request
    assert rg.rerank_plan(64, 1000, 512, 10, c).parts == 16 and rg.rerank_plan(1024, 1000, 512, 10, c).parts == 1
    assert rg.rerank_plan(1, 1000, 512, 10, c).parts == 63 and rg.rerank_plan(1, 3000, 512, 1024, c).parts == 64
    assert L.mcq_rerank_workspace_bytes(4, 100, 1, 10) == L.mcq_rerank_workspace_bytes(4, 100, 16384, 10)    # D moves the LDS alone
    for bad in ((0, 100, 64, 10), (4, 0, 64, 10), (-1, 100, 64, 10), (4, -1, 64, 10), (4, 100, 0, 10), (4, 100, 16385, 10),
                (4, 100, 64, 0), (4, 100, 64, 1025), ((1 << 31) - 1, 100, 64, 10), (4, (1 << 31) - 1, 64, 10)):
        assert L.mcq_rerank_workspace_bytes(*bad) == 256, bad


def _plain_score(q, x, metric):
    """rule 29 element by element: 64 python accumulators, the butterfly on a list"""
    f = np.float32
    D = len(q)
    acc, accx = [f(0)] * 64, [f(0)] * 64
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for e in range(D):
            lane = (e // 4) % 64
            qe, xe = f(q[e]), f(x[e])
            if metric == "l2":
                d = f(qe - xe)
                acc[lane] = f(acc[lane] + f(d * d))
            else:
                acc[lane] = f(acc[lane] + f(qe * xe))
                accx[lane] = f(accx[lane] + f(xe * xe))
        for m in (32, 16, 8, 4, 2, 1):
            acc = [f(acc[l] + acc[l ^ m]) for l in range(64)]
            accx = [f(accx[l] + accx[l ^ m]) for l in range(64)]
        if metric == "l2":
            return acc[0]
        if metric == "ip":
            return f(-acc[0])
        r = f(0) if accx[0] == 0 else f(f(1) / f(np.sqrt(accx[0])))
        return f(-f(acc[0] * r))


DS = (1, 3, 4, 5, 255, 256, 257, 260, 1000)


def _rows(D, half, rs):
    """a query and rows with +-0.0, denormals, 3e38 and inf among ordinary values"""
    dt = np.float16 if half else np.float32
    q = rs.standard_normal(D).astype(dt)
    X = rs.standard_normal((6, D)).astype(dt)
    X[1, rs.rand(D) < 0.5] = -0.0
    X[1, rs.rand(D) < 0.3] = 0.0
    X[2] = (rs.standard_normal(D) * (6e-8 if half else 1e-42)).astype(dt)          # denormals of the format
    X[3, rs.randint(D)] = dt(6e4) if half else dt(3e38)
    X[4, rs.randint(D)] = np.inf
    X[5] = 0                                                                      # a zero row
    return q, X


def test_score_restatement_against_a_plain_loop():
    rs = np.random.RandomState(11)
    for D in DS:
        for qhalf, xhalf in ((False, False), (True, True), (True, False)):
            q, _ = _rows(D, qhalf, rs)
            _, X = _rows(D, xhalf, rs)
            for qq in (q, np.zeros_like(q)):                  # and a zero query
                for metric in rg.METRICS:
                    got = rg.restate_scores(qq, X, metric)
                    want = np.array([_plain_score(qq, x, metric) for x in X], dtype=np.float32)
                    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (D, metric, qhalf, xhalf)
    # the score does not depend on the other rows, and dtype pairings with the same widened values give the same bits
    q, X = _rows(260, True, rs)
    for metric in rg.METRICS:
        a = rg.restate_scores(q, X, metric)
        b = rg.restate_scores(q.astype(np.float32), X[::-1].astype(np.float32), metric)[::-1]
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.signbit(rg.restate_scores(np.zeros(4, np.float32), np.ones((1, 4), np.float32), "cosine"))[0]   # -0.0: reported as 0


def test_score_restatement_within_the_bound_of_float64():
    rs = np.random.RandomState(12)
    assert [rg.lane_terms(D) for D in (1, 256, 257, 1000, 16384)] == [4, 4, 8, 16, 256]
    for D in DS + (4096,):
        for half in (False, True):
            dt = np.float16 if half else np.float32
            q = rs.standard_normal(D).astype(dt)
            X = np.concatenate([rs.standard_normal((8, D)), q[None, :] + 1e-3 * rs.standard_normal((4, D)),
                                np.zeros((1, D)), 1e-20 * rs.standard_normal((1, D))]).astype(dt)
            for metric in rg.METRICS:
                got = rg.restate_scores(q, X, metric).astype(np.float64)
                err = np.abs(got - rg.exact_scores(q, X, metric))
                bound = rg.error_bound(q, X, metric)
                assert (err <= bound).all(), (D, half, metric, err.max(), bound.max())


def test_claims_of_the_gpu_cases():
    c = rg.constants()
    seen = set()
    for x in rg.CASES:
        q, X, short, row_of = rg.make(x)
        assert q.shape == (x.Q, x.D) and X.shape == (x.B, x.D) and short.shape == (x.Q, x.S) and x.B <= 5000
        got = rg.reach(x, short, row_of, c)
        assert got == {f: getattr(x, f) for f in got}, (x.name, got)
        seen |= {f for f, v in got.items() if v}
        pos, row = rg.candidates(short, x.B, row_of)
        assert ((row >= 0) == (pos >= 0)).all() and (row < x.B).all()
        if x.short == "pad":
            assert (short[x.Q // 2] == -1).all() and (short[0, -1] == -1) and short[0, x.S // 2] == -1 and short[0, 0] >= 0
        if x.short == "junk":
            assert {x.B if row_of is None else len(row_of), 2 ** 40, -7} <= set(short.ravel().tolist())
        if x.short == "dups":
            assert all(len(set(r.tolist())) < x.S for r in short)
        if x.row_of == "perm_bad":
            assert ((row_of < 0) | (row_of >= x.B)).any() and ((pos < 0) & (short >= 0) & (short < len(row_of))).any()
    assert seen == {"parts", "one_part", "short_row", "empty_row", "all_enter", "elementwise", "chunks", "ragged"}
    assert {x.D for x in rg.CASES} >= {1, 3, 4, 30, 64, 252, 256, 260, 512, 1000, 16384}
    assert sum(x.D == 16384 for x in rg.CASES) == 1
    assert {(x.qhalf, x.xhalf) for x in rg.CASES} == {(False, False), (False, True), (True, False), (True, True)}
    assert {x.k for x in rg.CASES} >= {1, 10, 64, 65, 100, 1024} and {x.Q for x in rg.CASES} >= {1, 17, 300}
    assert {x.S for x in rg.CASES} >= {0, 1, 63, 64, 65, 1024, 1025, 3000} and {x.S - x.k for x in rg.CASES} >= {-1, 0, 1}
    assert {x.metric for x in rg.CASES} == set(rg.METRICS) and {x.row_of for x in rg.CASES} == {None, "perm", "perm_bad", "arange"}
    assert any(x.view and not x.xhalf for x in rg.CASES) and any(x.view and x.xhalf for x in rg.CASES)
    assert any(x.D * (2 if x.xhalf else 4) % 16 != 0 for x in rg.CASES)


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    from quantization_amd import rerank
    q, x = torch.zeros(3, 24), torch.zeros(50, 24)
    short = torch.zeros(3, 7, dtype=torch.int64)
    order = torch.arange(50)
    for k in (1, 10, 1024):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            rerank(q, x, short, k)
        with pytest.raises(m.McqError):
            rerank(q.half(), x.half(), short.int(), k, metric="cosine", row_of=order)
    with pytest.raises(ValueError, match="metric"):
        rerank(q, x, short, 10, metric="dot")
    for k in (0, 1025, -1, 2.0, True):
        with pytest.raises(ValueError, match="k ="):
            rerank(q, x, short, k)
    with pytest.raises(ValueError, match="vectors"):
        rerank(q, x.double(), short, 10)
    with pytest.raises(ValueError, match="vectors"):
        rerank(q, x[0], short, 10)
    with pytest.raises(ValueError, match="contiguous"):
        rerank(q, torch.zeros(24, 50).t(), short, 10)
    with pytest.raises(ValueError, match="dim"):
        rerank(torch.zeros(3, 16385), torch.zeros(2, 16385), short, 10)
    with pytest.raises(ValueError, match="queries"):
        rerank(torch.zeros(3, 23), x, short, 10)
    with pytest.raises(ValueError, match="queries"):
        rerank(q.to(torch.bfloat16), x, short, 10)
    with pytest.raises(ValueError, match="shortlist"):
        rerank(q, x, short[:2], 10)
    with pytest.raises(ValueError, match="shortlist"):
        rerank(q, x, short.float(), 10)
    with pytest.raises(ValueError, match="shortlist"):
        rerank(q.reshape(3, 1, 24), x, short, 10)
    with pytest.raises(ValueError, match="row_of"):
        rerank(q, x, short, 10, row_of=order.int())
    with pytest.raises(ValueError, match="row_of"):
        rerank(q, x, short, 10, row_of=order.reshape(5, 10))
