"""Host-side checks of the top-k search past 64 neighbours (no GPU; include/mcq_wide.h rules 24-27): the four entries of the
companion header are declared as _lib.WIDE_SIGNATURES binds them, exported and bound, and disjoint from the other tables;
include/mcq.h keeps its 64 declarations; every argument check of the two entries answers in search_check's order before
anything touches the device (fake pointers, no launch), with the cap at 1,024; the size queries and the mirror of wide_plan
(tests/search_wide_grid.py) agree; the claims of the GPU case table hold; the numpy helpers equal a plain double loop, with
+-0.0 ties and NaN; the value lists of launch_wide are the cells the GPU test launches; and the argument errors of the Python
interface precede any device work."""
import ctypes

import numpy as np
import pytest

import search_bias_grid as bg
import search_lists_grid as lg
import search_metric_grid as mg
import search_selection_grid as sel
import search_wide_grid as wg
import test_search_lists_host as lh

NEW = ("mcq_search_wide_workspace_bytes", "mcq_search_wide", "mcq_search_wide_lists_workspace_bytes", "mcq_search_wide_lists")
WIDE_HDR = sel.API.replace("quantization_amd/csrc/mcq_api.hip", "include/mcq_wide.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(WIDE_HDR)
    assert tuple(hdr) == NEW == m.WIDE_SYMBOLS == tuple(m.WIDE_SIGNATURES)
    assert ab.mismatches(hdr, m.WIDE_SIGNATURES) == []
    for other in (m.SYMBOLS, m.RESIDUAL_SYMBOLS, m.PROBE_SYMBOLS):
        assert not set(NEW) & set(other)
    assert not set(NEW) & set(ab.header_signatures()) and len(ab.header_signatures()) == 64 == len(m.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == list(m.WIDE_SIGNATURES[name][1])
    # the argument lists are those of mcq_search_scan_masked and mcq_search_scan_lists_bias, the size queries' those of theirs
    assert m.WIDE_SIGNATURES["mcq_search_wide"] == m.SIGNATURES["mcq_search_scan_masked"]
    assert m.WIDE_SIGNATURES["mcq_search_wide_lists"] == m.RESIDUAL_SIGNATURES["mcq_search_scan_lists_bias"]
    assert m.WIDE_SIGNATURES["mcq_search_wide_workspace_bytes"] == m.SIGNATURES["mcq_search_workspace_bytes"]
    assert m.WIDE_SIGNATURES["mcq_search_wide_lists_workspace_bytes"] == m.SIGNATURES["mcq_search_lists_workspace_bytes"]
    text = open(WIDE_HDR).read()
    for rule in (" 24. ", " 25. ", " 26. ", " 27. "):
        assert rule in text
    assert '#include "mcq_residual.h"' in text and L.mcq_abi_version() == 7
    doctored = dict(m.WIDE_SIGNATURES)                        # the comparison can fail: a long turned into an int
    r, args = doctored["mcq_search_wide"]
    doctored["mcq_search_wide"] = (r, args[:4] + (ctypes.c_int,) + args[5:])
    assert len(ab.mismatches(hdr, doctored)) == 1


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 3)
    at = lambda o: ctypes.c_void_p((1 << 20) + o)

    def lists(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, outs, ws, ws_bytes, k=10):
        return L.mcq_search_wide_lists(tables, Q, codes, w, B, N, K, k, metric, mask, off, nl, probes, P, bias, outs, outs, ws,
                                       ws_bytes, None)

    def whole(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, outs, ws, ws_bytes, k=10):
        return L.mcq_search_wide(tables, Q, codes, w, B, N, K, k, metric, mask, outs, outs, ws, ws_bytes, None)

    for f, is_lists in ((lists, True), (whole, False)):
        def need(k):
            return L.mcq_search_wide_lists_workspace_bytes(4, 8, 8, 256, k) if is_lists else L.mcq_search_wide_workspace_bytes(4, 1000, 8, 256, k)
        for mask in (fake, None):
            for bias in (fake, None):
                # the domain, with its status codes, before any pointer is looked at
                for K in (512, 1024, 8, 2048):
                    assert f(None, 4, None, None, 4, 4, K, 0, mask, None, 16, None, 8, bias, None, None, 0) == U
                assert f(None, 4, None, None, 4, 128, 256, 0, mask, None, 16, None, 8, bias, None, None, 0) == U
                assert f(None, 4, None, None, 4, 3, 256, 0, mask, None, 16, None, 8, bias, None, None, 0) == I
                # k: the cap is 1,024, answered before Q, B and the metric are looked at; k = 0 with them
                for k in (1025, 1 << 20):
                    assert f(None, -1, None, None, -1, 8, 256, 9, mask, None, 16, None, 8, bias, None, None, 0, k=k) == U
                for k in (0, -3):
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, bias, fake, fake, 1 << 30, k=k) == I
                assert f(None, -1, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, bias, None, None, 0) == I
                assert f(None, 4, None, None, -1, 8, 256, 0, mask, None, 16, None, 8, bias, None, None, 0) == I
                assert f(None, 1 << 31, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, bias, None, None, 0) == I
                for metric in (-1, 3):
                    assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, bias, fake, fake, need(10)) == I
                assert f(None, 4, None, None, 1 << 31, 8, 256, 0, mask, None, 16, None, 8, bias, None, None, 0) == U
                if is_lists:
                    assert f(None, 4, None, None, 1000, 8, 256, 0, mask, None, 16, None, 4097, bias, None, None, 0) == U
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, -1, bias, fake, fake, need(10)) == I
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, -1, fake, 8, bias, fake, fake, need(10)) == I
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, None, 16, fake, 8, bias, fake, fake, need(10)) == I   # no offsets
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, None, 8, bias, fake, fake, need(10)) == I   # no probes
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, at(4), 16, fake, 8, bias, fake, fake, need(10)) == I
                    assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, at(2), 8, bias, fake, fake, need(10)) == I
                # the pointers and the alignments
                assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, bias, None, fake, need(10)) == I      # no outputs
                assert f(None, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, bias, fake, fake, need(10)) == I      # no tables
                assert f(fake, 4, None, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, bias, fake, fake, need(10)) == I      # no codes
                assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, bias, fake, None, need(10)) == I      # no workspace
                assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_L2, mask, fake, 16, fake, 8, bias, fake, fake, need(10)) == I
                assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_COS, mask, fake, 16, fake, 8, bias, fake, fake, need(10)) == I
                assert f(fake, 4, at(4), fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, bias, fake, fake, need(10)) == I
                # last the workspace: k = 1,024 passes every check, and one byte less than the size query is refused
                for k in (1, 64, 65, 1024):
                    for metric in (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS):
                        assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, bias, fake, fake, need(k) - 1, k=k) == W
                    assert need(k) > 256
                assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, mask, fake, 16, fake, 8, bias, fake, fake, 0, k=1024) == W
        for o in (1, 2, 4, 7, 12):                           # rule 10: the mask is read as 8-byte words
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, at(o), fake, 16, fake, 8, fake, fake, fake, need(10)) == I
        if is_lists:                                         # rule 23: a misaligned bias, after the alignments of rule 16
            for o in (1, 2, 3, 6):
                assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, at(o), fake, fake, 0) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, at(4), fake, fake, need(10) - 1) == W
        # no queries: 0, and no input is looked at; the limits still come first
        assert f(None, 0, odd, None, 1000, 8, 256, 0, odd, odd, 16, odd, 8, odd, None, None, 0, k=1024) == 0
        assert f(None, 0, odd, None, 1000, 8, 256, 0, odd, odd, 16, odd, 8, odd, None, None, 0, k=1025) == U
        # a call without a candidate needs its outputs and looks at nothing else (with them the fill is a launch)
        for B, nl, P in ((0, 16, 8),) + (((1000, 0, 8), (1000, 16, 0)) if is_lists else ()):
            assert f(None, 4, odd, None, B, 8, 256, 0, odd, odd, nl, odd, P, odd, None, None, 0) == I
    # the older entries answer what they answered
    assert L.mcq_search_scan_masked(fake, 4, fake, fake, 1000, 8, 256, 65, 0, None, fake, fake, fake, 1 << 30, None) == U
    assert L.mcq_search_scan_lists(fake, 4, fake, fake, 1000, 8, 256, 65, 0, None, fake, 16, fake, 8, fake, fake, fake, 1 << 30, None) == U
    assert L.mcq_search_workspace_bytes(4, 1000, 8, 256, 65) == 256 == L.mcq_search_lists_workspace_bytes(4, 8, 8, 256, 65)


def test_size_queries_equal_the_mirror():
    m = _lib()
    L = m.lib()
    c = wg.constants()
    shapes = [(x.Q, 1, x.N, x.K, x.k) for x in wg.CASES if x.B > 0] + \
             [(1, 1, 1, 16, 1), (3, 64, 16, 256, 64), (17, 7, 2, 64, 100), (64, 32, 8, 256, 512), (64, 32, 8, 256, 513),
              (1024, 128, 8, 256, 1000), (5000, 4096, 64, 256, 1024), (1, 4096, 64, 256, 1024), (wg.ORDER_Q, 1, 1, 16, 1024)]
    for Q, P, N, K, k in shapes:
        plan = wg.wide_plan(Q, P, N, K, k, c)
        assert L.mcq_search_wide_lists_workspace_bytes(Q, P, N, K, k) == plan.ws_bytes, (Q, P, N, K, k)
        if P == 1:
            for B in (1, 1000, (1 << 31) - 1):               # it does not depend on B
                assert L.mcq_search_wide_workspace_bytes(Q, B, N, K, k) == plan.ws_bytes, (Q, B, N, K, k)
        assert 1 <= plan.parts <= c["kWideMergeEntries"] // plan.half and plan.lds <= 160 * 1024
        assert plan.parts * plan.half <= c["kWideMergeEntries"]
    # the largest accepted shape fits the CU's LDS; the merge of one query never streams lists_plan's 256 lists
    assert wg.wide_plan(1, c["kListMaxProbes"], 64, 256, 1024, c).lds == 128 * 1024 + 16 + 16 * 1024 + 64
    assert {wg.wide_plan(1, 8, 8, 256, k, c).parts for k in (1, 64, 512)} == {128}
    assert {wg.wide_plan(1, 8, 8, 256, k, c).parts for k in (513, 1024)} == {64}
    assert {wg.wide_plan(Q, 8, 8, 256, 100, c).parts for Q in (17, 64, 1024, 5000)} == {60, 16, 1}
    for bad in ((0, 1000, 8, 256, 10), (4, 0, 8, 256, 10), (4, 1 << 31, 8, 256, 10), (4, 1000, 8, 512, 10), (4, 1000, 8, 256, 1025),
                (4, 1000, 8, 256, 0), (4, 1000, 3, 256, 10)):
        assert L.mcq_search_wide_workspace_bytes(*bad) == 256
    for bad in ((0, 8, 8, 256, 10), (4, 0, 8, 256, 10), (4, 4097, 8, 256, 10), (4, 8, 8, 512, 10), (4, 8, 8, 256, 1025), (4, 8, 8, 256, 0)):
        assert L.mcq_search_wide_lists_workspace_bytes(*bad) == 256


def test_claims_of_the_gpu_cases():
    c = wg.constants()
    seen = set()
    for x in wg.CASES:
        plan = wg.wide_plan(x.Q, 1, x.N, x.K, x.k, c)
        got = wg.reach(x.B, plan, x.k, c)
        got["one_part"] = plan.parts == 1
        assert got == {f: getattr(x, f) for f in got}, (x.name, got)
        seen |= {f for f, v in got.items() if v}
    assert seen == {"parts", "empty_part", "partial", "short", "flush", "merge_flush", "one_part"}
    assert {x.k for x in wg.CASES} >= set(wg.KS)
    assert {(x.N, x.K) for x in wg.CASES} >= {(1, 16), (2, 256), (8, 256), (16, 16), (64, 16), (64, 256)}
    assert {x.Q for x in wg.CASES} >= {1, 17, 200}
    for x in wg.CASES:                                       # B in {0, k - 1, k, k + 1, 63, 64, 4,099, 100,003}
        assert x.B in (0, x.k - 1, x.k, x.k + 1, 63, 64, 4099, 100_003) or x.one_part
    assert {0, 63, 64, 4099, 100_003} <= {x.B for x in wg.CASES}
    assert {x.B - x.k for x in wg.CASES} >= {-1, 0, 1}
    # the hand-made orders: a hostile order flushes inside the loop at both k, and the merge at the larger
    for k in wg.ORDER_KS:
        plan = wg.wide_plan(wg.ORDER_Q, 1, wg.ORDER_N, wg.ORDER_K, k, c)
        got = wg.reach(wg.ORDER_B, plan, k, c)
        assert got["flush"] and got["parts"] and got["merge_flush"] == (k == 1024)
    w = wg.order_w("nan_short")
    assert (~np.isnan(w)).sum() == 500 and np.isnan(wg.order_w("nan")).sum() > wg.ORDER_B // 3
    z = wg.order_w("zeros")
    assert (z == 0).all() and 0 < np.signbit(z).sum() < len(z)
    i = wg.order_w("inf")
    assert np.isposinf(i).sum() > wg.ORDER_B - 1024 and np.isneginf(i).any() and 100 < np.isfinite(i).sum() < 1024
    # the widest lists cell is the largest LDS request
    big = wg.BIG
    assert wg.wide_plan(big.Q, big.P, big.N, big.K, big.k, c).lds == wg.wide_plan(1, c["kListMaxProbes"], 64, 256, 1024, c).lds


def _plain(s, k, keep=None):
    """rule 26 by a double loop: insertion into a sorted python list under (s, b), NaN skipped"""
    out_s, out_i = [], []
    for row in s:
        best = []
        for b, v in enumerate(row):
            if np.isnan(v) or (keep is not None and not keep[b]):
                continue
            j = 0
            while j < len(best) and (best[j][0] < v or (best[j][0] == v and best[j][1] < b)):
                j += 1
            best.insert(j, (v, b))
        best = best[:k]
        out_s.append([x[0] for x in best] + [np.float32(np.inf)] * (k - len(best)))
        out_i.append([x[1] for x in best] + [-1] * (k - len(best)))
    return np.array(out_s, dtype=np.float32).reshape(len(s), k), np.array(out_i, dtype=np.int64).reshape(len(s), k)


def test_restatement_against_a_plain_loop():
    rs = np.random.RandomState(4)
    Q, B = 5, 90
    s = (rs.randint(-6, 7, size=(Q, B)) / 2.0).astype(np.float32)             # many ties
    s[0, rs.rand(B) < 0.3] = -0.0                                            # -0.0 and +0.0 are one score
    s[0, rs.rand(B) < 0.3] = 0.0
    s[1, rs.rand(B) < 0.5] = np.nan
    s[2, :] = np.nan
    s[2, 7] = 1.0
    s[3, rs.rand(B) < 0.4] = np.inf
    s[3, 5] = -np.inf
    s[4, :] = np.nan                                                        # no candidate: the fill
    keep = rs.rand(B) < 0.6
    for k in (1, 10, 64, 65, 89, 90, 91, 300):
        for kp in (None, keep):
            got, want = wg.restate_topk_valid(s, k, kp), _plain(s, k, kp)
            assert np.array_equal(got[1], want[1]), (k, kp is not None)
            assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), "a reported score keeps its own bits"
            assert not np.isnan(got[0]).any() and (got[1][4] == -1).all() and np.isposinf(got[0][4]).all()
    # both zeros occur in the result of row 0, in ascending position among themselves
    zs, zi = wg.restate_topk_valid(s[:1], 90)
    at = np.flatnonzero(zs[0] == 0)
    assert len(set(np.signbit(zs[0][at]).tolist())) == 2 and (np.diff(zi[0][at]) > 0).all()
    # without NaN it is restate_topk; over lists it is restate_lists of the biased scores
    clean = np.nan_to_num(s, nan=2.5)
    a, b = wg.restate_topk_valid(clean, 20), wg.sg.restate_topk(clean, 20)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    Qt, N, K, Bt, T, codes, t, r, off, probes = lh._tiny()
    S = mg.restate_sums(T, codes)
    bias = np.zeros(probes.shape, dtype=np.float32)
    flat = bg.biased_scores(S, off, probes, bias, t, "l2")
    for k in (10, 100):
        a, b = wg.restate_topk_valid(flat, k), lg.restate_lists(flat, off, probes, k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def test_launch_wide_selects_exactly_the_cells_the_gpu_test_launches():
    assert wg.wide_pick_lists() == sel.NS == tuple(sel.pick_lists("launch_lists")["N"])
    with open(sel.API) as f:
        src = f.read()
    body = src[src.index("int launch_wide("):]
    body = body[:body.index("\n}\n")]
    # the bias is no template axis: the codebook count, the metric, the mask, and the code type of launch_wide<T>
    assert "li.bias != nullptr" not in body and "k_search_wide<NN, M, MASKED, T>" in body and "k_search_wide<NN, M, MASKED, T," not in body
    # the parsed launchers and the cap of the older entries stand as they stood
    assert src.count("    if (k > 64) return MCQ_EUNSUPPORTED;\n") == 1


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    from quantization_amd import Quantizer
    q = Quantizer(24, 16, 4)
    B = 130
    codes, x = torch.zeros(B, 4, dtype=torch.uint8), torch.zeros(3, 24)
    off = torch.tensor([0, 50, 130], dtype=torch.int64)
    probes = torch.zeros(3, 2, dtype=torch.int32)
    for k in (10, 200, 1025):
        with pytest.raises(m.McqError):                      # CPU tensors: no fallback
            q.search_wide(x, codes, k)
        with pytest.raises(m.McqError):
            q.search_lists_wide(x, codes, off, probes, k)
        with pytest.raises(ValueError):
            q.search_wide(x, codes, k, metric="dot")
        with pytest.raises(ValueError, match="mask"):
            q.search_wide(x, codes, k, mask=torch.zeros(B - 1, dtype=torch.bool))
        with pytest.raises(ValueError, match="probe_bias"):
            q.search_lists_wide(x, codes, off, probes, k, probe_bias=torch.zeros(3, 3))
        with pytest.raises(ValueError, match="probes"):
            q.search_lists_wide(x, codes, off, probes[:2], k)
    with pytest.raises(ValueError, match="probe_bias"):
        q._search_wide_scan(torch.zeros(3, 4, 16), codes, torch.zeros(B), 200, bias=torch.zeros(3, 2))      # a bias without lists
    with pytest.raises(m.McqError):
        q._search_wide_scan(torch.zeros(3, 4, 16), codes, torch.zeros(B), 200)
    from quantization_amd import search
    assert search.WIDE_MAX_K == wg.constants()["kWideMaxK"] and search.NARROW_MAX_K == 64
