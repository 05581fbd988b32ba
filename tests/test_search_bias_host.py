"""Host-side checks of the search over residual codes (no GPU; include/mcq_residual.h rules 21-23): the five entries of the
companion header are declared as _lib.RESIDUAL_SIGNATURES binds them, exported and bound; the numpy restatement of the
biased score (tests/search_bias_grid.py) equals a plain loop over (query, slot, position); the restatement of the based
norms equals exact arithmetic on dyadic data; every argument check of the new entries answers in the documented order
before anything touches the device (fake pointers, no launch); the argument errors of the Python interface precede any
device work; the value lists of the two list launchers are exactly the cells the GPU tests launch with a bias; and list_assign /
probe_bias against numpy."""
import ctypes

import numpy as np
import pytest

import search_bias_grid as bg
import search_lists_grid as lg
import search_metric_grid as mg
import search_range_lists_grid as rl
import search_selection_grid as sel
import test_search_lists_host as lh

NEW = ("mcq_search_scan_lists_bias", "mcq_search_range_lists_bias_count", "mcq_search_range_lists_bias_fill",
       "mcq_code_norms_based", "mcq_code_rnorms_based")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


RESIDUAL_HDR = sel.API.replace("quantization_amd/csrc/mcq_api.hip", "include/mcq_residual.h")


def test_symbols_are_declared_exported_and_bound():
    """the companion header against _lib.RESIDUAL_SIGNATURES, as tests/test_abi_signatures_host.py compares include/mcq.h with
    _lib.SIGNATURES (its parser and its comparison); include/mcq.h and its table keep what they had"""
    import test_abi_signatures_host as ab
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(RESIDUAL_HDR)
    assert tuple(hdr) == NEW == m.RESIDUAL_SYMBOLS == tuple(m.RESIDUAL_SIGNATURES)
    assert ab.mismatches(hdr, m.RESIDUAL_SIGNATURES) == []
    assert not set(NEW) & set(m.SYMBOLS) and not set(NEW) & set(ab.header_signatures())
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == list(m.RESIDUAL_SIGNATURES[name][1])
    assert len(L.mcq_search_scan_lists_bias.argtypes) == len(L.mcq_search_scan_lists.argtypes) + 1
    assert len(L.mcq_search_range_lists_bias_count.argtypes) == len(L.mcq_search_range_lists_count.argtypes) + 1
    assert len(L.mcq_search_range_lists_bias_fill.argtypes) == len(L.mcq_search_range_lists_fill.argtypes) + 1
    assert len(L.mcq_code_norms_based.argtypes) == len(L.mcq_code_norms.argtypes) + 3
    # the biased entries are the unbiased ones with one pointer after P; the based norms take base, L, assign after D
    for new, old, at in (("mcq_search_scan_lists_bias", "mcq_search_scan_lists", 14),
                         ("mcq_search_range_lists_bias_count", "mcq_search_range_lists_count", 13),
                         ("mcq_search_range_lists_bias_fill", "mcq_search_range_lists_fill", 13)):
        a, b = m.RESIDUAL_SIGNATURES[new][1], m.SIGNATURES[old][1]
        assert a[:at] + a[at + 1:] == b and a[at] is ctypes.c_void_p
    a, b = m.RESIDUAL_SIGNATURES["mcq_code_norms_based"][1], m.SIGNATURES["mcq_code_norms"][1]
    assert a[:6] + a[9:] == b and a[6:9] == (ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p)
    text = open(RESIDUAL_HDR).read()
    for rule in (" 21. ", " 22. ", " 23. "):
        assert rule in text
    assert '#include "mcq.h"' in text and L.mcq_abi_version() == 7
    # the comparison can fail: a long turned into an int
    doctored = dict(m.RESIDUAL_SIGNATURES)
    r, args = doctored["mcq_code_norms_based"]
    doctored["mcq_code_norms_based"] = (r, args[:7] + (ctypes.c_int,) + args[8:])
    assert len(ab.mismatches(hdr, doctored)) == 1


# ------------------------------------------------------------------ the restatements
def _tiny_bias(Q, P):
    rs = np.random.RandomState(12)
    bias = (rs.randint(-40, 40, size=(Q, P)) / 8.0).astype(np.float32)       # dyadic, like the tables of _tiny
    bias[0, 2] = 0.0
    bias[1, 0] = -0.0
    return bias


@pytest.mark.parametrize("metric", bg.METRICS)
def test_biased_restatement_against_a_plain_loop(metric):
    Q, N, K, B, T, codes, t, r, off, probes = lh._tiny()
    k, nl = 10, len(off) - 1
    bias = _tiny_bias(Q, probes.shape[1])
    w = {"l2": t, "ip": None, "cosine": r}[metric]
    S = mg.restate_sums(T, codes)
    got_s, got_i = lg.restate_lists(bg.biased_scores(S, off, probes, bias, w, metric), off, probes, k)
    thr = np.array([np.inf, 1.0, np.inf, -2.0, 0.5, np.nan], dtype=np.float32)
    lims, r_pos, r_val = bg.restate_range_lists_bias(S, off, probes, bias, w, metric, thr)
    for q in range(Q):
        pairs, listed = [], []
        for p in range(probes.shape[1]):
            l = int(probes[q, p])
            if not 0 <= l < nl:
                continue
            for b in range(int(off[l]), int(off[l + 1])):
                s = 0.0
                for n in range(N):
                    s += float(T[q, n, codes[b, n]])                        # (dyadic: every sum is exact)
                s += float(bias[q, p])
                sc = s + float(t[b]) if metric == "l2" else (s if metric == "ip" else float(np.float32(s) * r[b]))
                pairs.append((sc, b))
                if sc <= thr[q]:
                    listed.append((b, sc))
        assert len(pairs) == len(lg.candidates(off, probes[q]))
        want = (sorted(pairs) + [(np.inf, -1)] * k)[:k]
        assert got_s[q].astype(np.float64).tolist() == [x[0] for x in want] and got_i[q].tolist() == [x[1] for x in want]
        lo, hi = lims[q], lims[q + 1]
        assert r_pos[lo:hi].tolist() == [x[0] for x in listed]                # the row's own order, slot by slot
        assert r_val[lo:hi].astype(np.float64).tolist() == [x[1] for x in listed]
    assert lims[3] == lims[2] and lims[-1] == len(r_pos) > 0
    # a zero bias is the unbiased restatement, bit for bit, signed zeros included; the bias moves some query's result
    for zero in (0.0, -0.0):
        flat = bg.biased_scores(S, off, probes, np.full(probes.shape, zero, dtype=np.float32), w, metric)
        plain = mg.restate_metric_scores(T, w, codes, metric)
        a, b = lg.restate_lists(flat, off, probes, k), lg.restate_lists(plain, off, probes, k)
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    plain_i = lg.restate_lists(mg.restate_metric_scores(T, w, codes, metric), off, probes, k)[1]
    assert any(not np.array_equal(plain_i[q], got_i[q]) for q in bg.rows_with_two_lists(off, probes))
    # a list named twice is listed twice, each time with the bias of that naming's slot
    twice = np.array([[2, 5, 2]], dtype=np.int32)
    b2 = np.array([[1.0, 0.5, -3.0]], dtype=np.float32)
    l2, p2, v2 = bg.restate_range_lists_bias(S[:1], off, twice, b2, w, metric, np.array([np.inf], dtype=np.float32))
    n2, n5 = int(off[3] - off[2]), int(off[6] - off[5])
    assert l2[1] == 2 * n2 + n5 and np.array_equal(p2[:n2], p2[n2 + n5:])
    if metric == "ip":
        assert np.array_equal(v2[:n2] - np.float32(4.0), v2[n2 + n5:])


def test_bias_of_a_gpu_case_has_what_it_promises():
    for case in lg.CASES:
        off, probes = lg.layout(case)
        T, codes, t = lg.host_data(case)
        bias = bg.bias_for(mg.restate_sums(T, codes), off, probes)
        named = bg.named_slots(off, probes)
        assert bias.dtype == np.float32 and bias.shape == probes.shape and np.isfinite(bias).all()
        vals = np.array([bias[s] for s in named])
        assert (vals == 0).any() and (vals < 0).any() or len(named) <= 2
        assert len(named) <= 1 or np.signbit(bias[named[-1]]) and bias[named[-1]] == 0          # the one -0.0


def test_based_norms_restatement_on_exact_data():
    rs = np.random.RandomState(3)
    for N, K, D in ((1, 16, 24), (4, 16, 40), (2, 16, 260)):
        Dp, B, L = sg_padded(D), 50, 3
        C = np.zeros((N, K, Dp), dtype=np.float32)
        C[:, :, :D] = rs.randint(-8, 9, size=(N, K, D)) / 4.0                   # dyadic: every fp32 operation below is exact
        codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
        base = (rs.randint(-8, 9, size=(L, D)) / 4.0).astype(np.float32)
        assign = rs.randint(-1, L + 1, size=B).astype(np.int32)
        assert (assign == -1).any() and (assign == L).any()
        got = bg.restate_norms_based(C, codes, base, assign, D)
        dec = sum(C[n].astype(np.float64)[codes[:, n]] for n in range(N))[:, :D]
        ok = (assign >= 0) & (assign < L)
        full = dec + np.where(ok[:, None], base.astype(np.float64)[np.clip(assign, 0, L - 1)], 0.0)
        assert np.array_equal(got.astype(np.float64), (full ** 2).sum(1))
        assert np.array_equal(bg.restate_norms_based(C, codes, None, None, D).astype(np.float64), (dec ** 2).sum(1))


def sg_padded(D):
    import search_grid as sg
    return sg.padded(D)


# ------------------------------------------------------------------ the C entries
def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 3)
    need = L.mcq_search_lists_workspace_bytes(4, 8, 8, 256, 10)
    rneed = L.mcq_search_range_lists_workspace_bytes(4, 8, 8, 256)

    def scan(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, outs, ws, ws_bytes, k=10):
        return L.mcq_search_scan_lists_bias(tables, Q, codes, w, B, N, K, k, metric, mask, off, nl, probes, P, bias, outs, outs, ws,
                                            ws_bytes, None)

    def count(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, outs, ws, ws_bytes, thr=fake):
        return L.mcq_search_range_lists_bias_count(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, thr, outs,
                                                   ws, ws_bytes, None)

    def fill(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, outs, ws, ws_bytes, thr=fake, cap=5):
        return L.mcq_search_range_lists_bias_fill(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, bias, thr, outs,
                                                  fake, fake, cap, ws, ws_bytes, None)

    for f, enough in ((scan, need), (count, rneed), (fill, rneed)):
        for bias in (fake, None):                            # probe_bias == NULL is accepted: every answer is the same
            # the limits of rules 16 and 19, with their status codes, before any pointer is looked at
            for K in (512, 1024, 8, 2048):
                assert f(None, 4, None, None, 4, 4, K, 0, None, None, 16, None, 8, bias, None, None, 0) == U
            assert f(None, 4, None, None, 4, 128, 256, 0, None, None, 16, None, 8, bias, None, None, 0) == U
            assert f(None, 4, None, None, 1 << 31, 8, 256, 0, None, None, 16, None, 8, bias, None, None, 0) == U
            assert f(None, 4, None, None, 4, 3, 256, 0, None, None, 16, None, 8, bias, None, None, 0) == I
            assert f(None, -1, None, None, 4, 8, 256, 0, None, None, 16, None, 8, bias, None, None, 0) == I
            assert f(None, 4, None, None, -1, 8, 256, 0, None, None, 16, None, 8, bias, None, None, 0) == I
            for metric in (-1, 3):
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, None, fake, 16, fake, 8, bias, fake, fake, enough) == I
            assert f(None, 4, None, None, 1000, 8, 256, 0, None, None, 16, None, 4097, bias, None, None, 0) == U
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, -1, bias, fake, fake, enough) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, -1, fake, 8, bias, fake, fake, enough) == I
            # the pointers and the alignments of rule 16
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, bias, None, fake, enough) == I    # no outputs / lims
            assert f(None, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, bias, fake, fake, enough) == I    # no tables
            assert f(fake, 4, None, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, bias, fake, fake, enough) == I    # no codes
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, bias, fake, None, enough) == I    # no workspace
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, None, 16, fake, 8, bias, fake, fake, enough) == I    # no offsets
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, None, 8, bias, fake, fake, enough) == I    # no probes
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_L2, None, fake, 16, fake, 8, bias, fake, fake, enough) == I
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_COS, None, fake, 16, fake, 8, bias, fake, fake, enough) == I
            assert f(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, bias, fake, fake, enough) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, ctypes.c_void_p((1 << 20) + 4), fake, 16, fake, 8, bias, fake, fake, enough) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, ctypes.c_void_p((1 << 20) + 4), 16, fake, 8, bias, fake, fake, enough) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, ctypes.c_void_p((1 << 20) + 2), 8, bias, fake, fake, enough) == I
            # last a short workspace: everything else passed, a NULL bias included
            for metric in (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS):
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, None, fake, 16, fake, 8, bias, fake, fake, enough - 1) == W
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, fake, fake, 16, fake, 8, bias, fake, fake, 0) == W
        # rule 23: a misaligned bias is MCQ_EINVAL, before thr and the size of the workspace are looked at
        for o in (1, 2, 3, 6):
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, ctypes.c_void_p((1 << 20) + o), fake, fake, 0) == I
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, ctypes.c_void_p((1 << 20) + 4), fake, fake, enough - 1) == W
        # no queries: 0, and no input is looked at -- a misaligned bias neither (count still writes lims[0]: a launch, which
        # tests/test_gpu_search_range_lists_bias.py makes)
        if f is not count:
            assert f(None, 0, odd, None, 1000, 8, 256, 0, odd, odd, 16, odd, 8, odd, fake, None, 0) == 0
        # the limits still come first
        assert f(None, 0, None, None, 1000, 8, 256, 0, None, None, 16, None, 4097, odd, None, None, 0) == U
    # the range pair: thr after the alignments (a misaligned bias answers first, and both are MCQ_EINVAL), then the workspace
    for f in (count, fill):
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, fake, fake, fake, rneed - 1, thr=None) == I
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, fake, fake, fake, rneed - 1) == W
        for B, nl, P in ((0, 16, 8), (1000, 0, 8), (1000, 16, 0)):           # empty: lims is needed, nothing else is looked at
            assert f(None, 4, odd, None, B, 8, 256, 0, odd, odd, nl, odd, P, odd, None, None, 0) == I
    assert fill(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, fake, fake, fake, rneed, cap=-1) == I
    assert fill(None, 4, odd, None, 0, 8, 256, 0, odd, odd, 16, odd, 8, odd, fake, None, 0) == 0      # empty: writes nothing
    for B, nl, P in ((0, 16, 8), (1000, 0, 8), (1000, 16, 0)):               # the scan: an empty call needs its outputs
        assert scan(None, 4, odd, None, B, 8, 256, 0, odd, odd, nl, odd, P, odd, None, None, 0) == I


def test_based_norms_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 2)
    for f in (L.mcq_code_norms_based, L.mcq_code_rnorms_based):
        # the domain and the checks of mcq_code_norms
        assert f(None, 4, None, 8, 512, 24, None, 3, None, None, None) == U
        assert f(None, 4, None, 3, 256, 24, None, 3, None, None, None) == I
        assert f(None, -1, None, 8, 256, 24, None, 3, None, None, None) == I
        assert f(None, 1 << 31, None, 8, 256, 24, None, 3, None, None, None) == U
        assert f(fake, 4, fake, 8, 256, 24, fake, -1, fake, fake, None) == I          # L < 0
        assert f(None, 0, None, 8, 256, 24, None, -1, None, None, None) == I          # ... before the empty call
        assert f(None, 0, None, 8, 256, 24, None, 0, None, None, None) == 0           # B == 0 looks at nothing
        for hole in range(5):                                                         # codes, prepared, base, assign, out
            args = [fake, 4, fake, 8, 256, 24, fake, 3, fake, fake, None]
            args[(0, 2, 6, 8, 9)[hole]] = None
            assert f(*args) == I, hole
        assert f(fake, 4, fake, 8, 256, 24, odd, 3, fake, fake, None) == I
        assert f(fake, 4, fake, 8, 256, 24, fake, 3, odd, fake, None) == I


# ------------------------------------------------------------------ the Python interface
def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    from quantization_amd import Quantizer
    q = Quantizer(24, 16, 4)
    B = 130
    codes, x = torch.zeros(B, 4, dtype=torch.uint8), torch.zeros(3, 24)
    off = torch.tensor([0, 50, 130], dtype=torch.int64)
    probes = torch.zeros(3, 2, dtype=torch.int32)
    for call in (lambda **kw: q.search_lists(x, codes, off, probes, **kw), lambda **kw: q.range_search_lists(x, codes, off, probes, 1.0, **kw)):
        for bad in (torch.zeros(3, 3), torch.zeros(2, 2), torch.zeros(6), torch.zeros(3, 2, dtype=torch.int32), [[0.0, 0.0]] * 3):
            for metric in ("l2", "ip"):
                with pytest.raises(ValueError, match="probe_bias"):
                    call(probe_bias=bad, metric=metric)
        for good in (torch.zeros(3, 2), torch.zeros(3, 2, dtype=torch.float16), torch.zeros(3, 2, dtype=torch.float64)):
            with pytest.raises(m.McqError):                  # right, but not on the device: the error of every other input
                call(probe_bias=good)
        with pytest.raises(ValueError):
            call(probe_bias=torch.zeros(3, 2), metric="dot")
    with pytest.raises(ValueError, match="probe_bias"):
        q.search_lists(x.reshape(1, 3, 24), codes, off, probes.reshape(1, 3, 2), probe_bias=torch.zeros(3, 2))
    with pytest.raises(ValueError, match="probe_bias"):
        q._search_scan(torch.zeros(3, 4, 16), codes, torch.zeros(B), 10, lists=(off, probes), bias=torch.zeros(3, 1))
    with pytest.raises(ValueError, match="probe_bias"):
        q._search_scan(torch.zeros(3, 4, 16), codes, torch.zeros(B), 10, bias=torch.zeros(3, 2))       # a bias without lists
    with pytest.raises(ValueError, match="probe_bias"):
        q._search_range(torch.zeros(3, 4, 16), codes, torch.zeros(B), torch.zeros(3), lists=(off, probes), bias=torch.zeros(2, 2))
    base, assign = torch.zeros(2, 24), torch.zeros(B, dtype=torch.int64)
    for f in (q.code_norms, q.code_rnorms):
        with pytest.raises(ValueError, match="base and assign"):
            f(codes, base=base)
        with pytest.raises(ValueError, match="base and assign"):
            f(codes, assign=assign)
        for bad in (torch.zeros(2, 23), torch.zeros(24), torch.zeros(2, 24, dtype=torch.int32)):
            with pytest.raises(ValueError, match="base"):
                f(codes, base=bad, assign=assign)
        for bad in (assign[:-1], assign.to(torch.float32), assign.reshape(1, B), assign.to(torch.bool)):
            with pytest.raises(ValueError, match="assign"):
                f(codes, base=base, assign=bad)
        with pytest.raises(m.McqError):
            f(codes, base=base, assign=assign)


def test_a_call_without_a_bias_takes_the_entries_it_took():
    _lib()
    from quantization_amd import search
    assert search._ENTRIES[0][0] == "bias" and [row[0] for row in search._ENTRIES[1:]] == ["lists", "mask", "metric", None]
    assert search._ENTRIES[0][1:] == ("mcq_search_scan_lists_bias", "mcq_search_lists_workspace_bytes",
                                      "mcq_search_range_lists_bias_count", "mcq_search_range_lists_bias_fill",
                                      "mcq_search_range_lists_workspace_bytes")


# ------------------------------------------------------------------ selection
def test_the_launchers_of_the_biased_kernels_select_exactly_the_cells_the_gpu_tests_launch():
    got = bg.coverage()
    assert got == {"launch_lists": 7 * 3 * 2, "launch_range_lists": 4 * 2 * 2}
    # the same value lists as without a bias: a call moves between the two by its bias alone.  One launcher each, whose
    # bias flag is the innermost selection, below every pick<...> list
    with open(sel.API) as f:
        src = f.read()
    assert "launch_lists_bias" not in src and "launch_range_lists_bias" not in src
    for launcher in ("launch_lists", "launch_range_lists"):
        assert sel.DISPATCHERS[launcher][1] == 2
        body = src[src.index("int " + launcher + "("):]
        body = body[:body.index("\n}\n")]
        assert body.count("pick_bool(li.bias != nullptr,") == 1
        assert body.rindex("pick<") < body.index("pick_bool(li.bias != nullptr,") < body.index("hipLaunchKernelGGL(")
    assert sel.range_chunk_cap(launcher="launch_range_lists") == sel.range_chunk_cap()
    # a value added to a list has no cell: coverage() says so
    import os
    import tempfile
    for launcher, old, new in (("launch_lists", "pick<1, 2, 4, 8, 16, 32, 64>", "pick<1, 2, 4, 8, 16, 32, 64, 128>"),
                               ("launch_lists", "pick<kMetricL2, kMetricIP, kMetricCos>", "pick<kMetricL2, kMetricIP, kMetricCos, 3>"),
                               ("launch_range_lists", "pick<1, 2, 4, 8>", "pick<1, 2, 4, 8, 16>")):
        at = src.index("int " + launcher + "(")
        changed = src[:at] + src[at:].replace(old, new, 1)
        assert changed != src
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "api.hip")
            with open(path, "w") as f:
                f.write(changed)
            with pytest.raises(AssertionError, match=launcher + ":"):
                bg.coverage(path)
    # the cells exist: the lists layout of the selection grid has two lists that are not empty in every row
    off, probes = sel.lists_layout()
    assert sorted(bg.rows_with_two_lists(off, probes)) == [0, 1, 2]


# ------------------------------------------------------------------ ivf.py
def test_list_assign_and_probe_bias_against_numpy():
    import torch
    _lib()
    from quantization_amd import list_assign, probe_bias
    off = np.array([4, 4, 9, 30, 30, 100, 141], dtype=np.int64)          # a gap before the first list, two empty lists
    B = 150
    got = list_assign(torch.from_numpy(off), B)
    assert got.dtype == torch.int32 and tuple(got.shape) == (B,)
    want = np.full(B, -1, dtype=np.int32)
    for l in range(len(off) - 1):
        want[off[l]:off[l + 1]] = l
    assert np.array_equal(got.numpy(), want) and (want[:4] == -1).all() and (want[141:] == -1).all()
    assert 0 not in want and 3 not in want
    assert list_assign(torch.from_numpy(off), 0).numel() == 0
    assert list_assign(torch.zeros(1, dtype=torch.int64), 5).tolist() == [-1] * 5                # no list at all
    for bad in (lambda: list_assign(torch.from_numpy(off).to(torch.int32), B), lambda: list_assign(torch.from_numpy(off), -1),
                lambda: list_assign(off, B)):
        with pytest.raises(ValueError):
            bad()

    rs = np.random.RandomState(8)
    Q, L, D, P = 5, 6, 24, 4
    x = rs.randn(Q, D).astype(np.float32)
    cen = rs.randn(L, D).astype(np.float32)
    probes = rs.randint(0, L, size=(Q, P)).astype(np.int32)
    probes[0, 1] = -1
    probes[2, 0] = L
    probes[3, 3] = -7
    for dtype in (torch.int32, torch.int64):
        got = probe_bias(torch.from_numpy(x), torch.from_numpy(cen), torch.from_numpy(probes).to(dtype))
        assert got.dtype == torch.float32 and tuple(got.shape) == (Q, P)
        named = (probes >= 0) & (probes < L)
        want = -2.0 * (x.astype(np.float64) @ cen.astype(np.float64).T)[np.arange(Q)[:, None], np.clip(probes, 0, L - 1)]
        g = got.numpy()
        assert (g[~named] == 0).all() and not np.signbit(g[~named]).any()
        assert np.abs(g[named] - want[named]).max() <= 2 * (D + 2) * 2.0 ** -24 * (np.abs(x) @ np.abs(cen).T).max()
    wide = probe_bias(torch.from_numpy(x).reshape(1, Q, D), torch.from_numpy(cen), torch.from_numpy(probes).reshape(1, Q, P))
    assert tuple(wide.shape) == (1, Q, P) and torch.equal(wide[0], got)
    for bad in (lambda: probe_bias(torch.from_numpy(x), torch.from_numpy(cen[:, :5]), torch.from_numpy(probes)),
                lambda: probe_bias(torch.from_numpy(x), torch.from_numpy(cen), torch.from_numpy(probes[:-1])),
                lambda: probe_bias(torch.from_numpy(x), torch.from_numpy(cen), torch.from_numpy(probes).float())):
        with pytest.raises(ValueError):
            bad()
    # the unused claim check of the range grid's thresholds: the biased scores of a case give no hit, some and all
    case = rl.CASES[1]
    off, probes = rl.layout(case)
    T, codes, t = lg.host_data(case.base)
    S = mg.restate_sums(T, codes)
    bias = bg.bias_for(S, off, probes)
    s = bg.biased_scores(S, off, probes, bias, t, "l2")
    thr = rl.thresholds_for(s, off, probes)
    n = np.diff(bg.restate_range_lists_bias(S, off, probes, bias, t, "l2", thr)[0])
    cand = np.array([len(rl.row_positions(off, row)) for row in probes])
    assert (n == 0).any() and (n == cand)[cand > 0].any() and ((n > 0) & (n < cand)).any()
