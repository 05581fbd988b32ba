"""Host-side checks of the range search list by list (no GPU): the three symbols are exported and bound, every argument check of
rule 19 of include/mcq.h answers before anything touches the device (fake pointers, no launch), the size query equals the
mirror of range_lists_plan and depends on neither B nor L, the numpy restatement of rules 17 and 18
(tests/search_range_lists_grid.py) equals a brute-force double loop and, for ascending rows, the masked range restatement
under the union mask of each query, the claims of the GPU case table, and the argument errors of the Python interface that
precede any device work."""
import ctypes

import numpy as np
import pytest

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_lists_grid as rl


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


NAMES = ("mcq_search_range_lists_workspace_bytes", "mcq_search_range_lists_count", "mcq_search_range_lists_fill")


def test_symbols_are_exported_and_bound():
    m = _lib()
    L = m.lib()
    hdr = open(sg.HDR.replace("quantization_amd/csrc/mcq_search_kernels.h", "include/mcq.h")).read()
    for name in NAMES:
        assert name in m.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert L.mcq_search_range_lists_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.mcq_search_range_lists_workspace_bytes.argtypes) == 4
    assert len(L.mcq_search_range_lists_count.argtypes) == 18 and len(L.mcq_search_range_lists_fill.argtypes) == 21
    for rule in (" 17. ", " 18. ", " 19. ", " 20. "):
        assert rule in hdr
    assert L.mcq_abi_version() == 7
    from quantization_amd import Quantizer
    assert callable(Quantizer.range_search_lists)


def _calls(L):
    """count and fill behind one signature: (tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, thr, lims, ws, bytes)"""
    fake = ctypes.c_void_p(1 << 20)

    def count(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, thr, lims, ws, ws_bytes):
        return L.mcq_search_range_lists_count(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, thr, lims, ws,
                                              ws_bytes, None)

    def fill(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, thr, lims, ws, ws_bytes):
        return L.mcq_search_range_lists_fill(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, thr, lims, fake, fake,
                                             1 << 20, ws, ws_bytes, None)
    return count, fill


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    odd = ctypes.c_void_p((1 << 20) + 3)
    need = L.mcq_search_range_lists_workspace_bytes(4, 8, 8, 256)
    for f in _calls(L):
        for mask in (fake, None):
            # the limits of rule 16 without k, with its status codes, before any pointer is looked at
            for K in (512, 1024, 8, 2048):
                assert f(None, 4, None, None, 4, 4, K, 0, mask, None, 16, None, 8, None, None, None, 0) == U
            assert f(None, 4, None, None, 4, 128, 256, 0, mask, None, 16, None, 8, None, None, None, 0) == U      # N > 64
            assert f(None, 4, None, None, 1 << 31, 8, 256, 0, mask, None, 16, None, 8, None, None, None, 0) == U  # B > 2^31 - 1
            assert f(None, 4, None, None, 4, 3, 256, 0, mask, None, 16, None, 8, None, None, None, 0) == I        # N = 3
            assert f(None, -1, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, None, None, None, 0) == I
            assert f(None, 4, None, None, -1, 8, 256, 0, mask, None, 16, None, 8, None, None, None, 0) == I
            assert f(None, 1 << 31, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, None, None, None, 0) == I  # Q > 2^31 - 1
            for metric in (-1, 3, 7):
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, fake, fake, fake, need) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 4097, fake, fake, fake, 1 << 30) == U
            assert f(None, 4, None, None, 1000, 8, 256, 0, mask, None, 16, None, 4097, None, None, None, 0) == U
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, -1, fake, fake, fake, need) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, -1, fake, 8, fake, fake, fake, need) == I  # a negative L
            # the pointers of rule 16
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, None, 16, fake, 8, fake, fake, fake, need) == I  # no offsets
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, None, 8, fake, fake, fake, need) == I  # no probes
            assert f(None, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, fake, need) == I  # no tables
            assert f(fake, 4, None, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, fake, need) == I  # no codes
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, None, need) == I  # no workspace
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_L2, mask, fake, 16, fake, 8, fake, fake, fake, need) == I
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_COS, mask, fake, 16, fake, 8, fake, fake, fake, need) == I
            for o in (1, 2, 4, 7, 12):
                assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, ctypes.c_void_p((1 << 20) + o), 16, fake, 8, fake, fake, fake,
                         need) == I
            for o in (1, 2, 3, 6):                           # misaligned probes
                assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, ctypes.c_void_p((1 << 20) + o), 8, fake, fake, fake,
                         need) == I
            assert f(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, fake, need) == I
            assert f(fake, 4, ctypes.c_void_p((1 << 20) + 8), fake, 1000, 16, 256, 0, mask, fake, 16, fake, 8, fake, fake, fake,
                     need * 4) == I                          # misaligned codes
            # thr and lims
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, None, fake, fake, need) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, None, fake, need) == I
            # last, a short workspace: whatever the metric, and only after everything else has passed
            for metric in (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS):
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, fake, fake, fake, need - 1) == W
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, fake, fake, fake, 0) == W
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, mask, fake, 16, fake, 8, fake, fake, fake, need - 1) == W
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, None, fake, fake, need - 1) == I   # thr first
        for o in (1, 2, 4, 7, 12):                           # rule 10: the mask is read as 8-byte words
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, ctypes.c_void_p((1 << 20) + o), fake, 16, fake, 8, fake, fake, fake, need) == I
        # an empty call needs lims and looks at nothing else: without lims it is rejected (with it count launches the zeroing,
        # which tests/test_gpu_search_range_lists.py does)
        for Q, B, nl, P in ((0, 1000, 16, 8), (4, 0, 16, 8), (4, 1000, 0, 8), (4, 1000, 16, 0)):
            assert f(None, Q, odd, None, B, 8, 256, 0, odd, odd, nl, odd, P, None, None, None, 0) == I
        # the limits still come first
        assert f(None, 0, None, None, 1000, 8, 256, 0, None, None, 16, None, 4097, None, fake, None, 0) == U
        assert f(None, 4, None, None, 0, 8, 256, 0, None, None, -1, None, 8, None, fake, None, 0) == I
    # fill on an empty call stores nothing and launches nothing: 0 with lims alone; a negative capacity is rejected
    for Q, B, nl, P in ((0, 1000, 16, 8), (4, 0, 16, 8), (4, 1000, 0, 8), (4, 1000, 16, 0)):
        assert L.mcq_search_range_lists_fill(None, Q, odd, None, B, 8, 256, 0, odd, odd, nl, odd, P, None, fake, None, None, 0,
                                             None, 0, None) == 0
    assert L.mcq_search_range_lists_fill(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, fake, fake, fake, fake, -1,
                                         fake, need, None) == I
    assert L.mcq_search_range_lists_fill(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, fake, fake, None, None, 0,
                                         fake, need, None) == 0                      # no room: nothing to store into
    assert L.mcq_search_range_lists_fill(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, 16, fake, 8, fake, fake, None, fake, 5,
                                         fake, need, None) == I                      # room, but no out_score


def test_size_query_equals_the_mirror_and_ignores_B_and_L():
    m = _lib()
    L = m.lib()
    fake = ctypes.c_void_p(1 << 20)
    c = rl.constants()
    assert 1 <= c["kRangeListWaves"] <= 16
    for Q, P, N, K in ((1, 1, 1, 16), (3, 64, 16, 256), (5, 3, 4, 16), (17, 7, 2, 64), (64, 32, 8, 256), (1024, 128, 8, 256),
                       (5000, 4096, 64, 256), (1, 4096, 8, 256)):
        plan = rl.range_lists_plan(Q, P, N, K, c)
        got = L.mcq_search_range_lists_workspace_bytes(Q, P, N, K)
        assert got == plan.ws_bytes >= Q * plan.parts * plan.waves * 8, (Q, P, N, K)
        assert plan.parts == lg.lists_plan(Q, P, N, K, 10, c).parts and plan.lds <= 160 * 1024
        for mask in (fake, None):                            # the same size whatever B and L, and one byte less is refused
            for B, nl in ((1000, 16), (1 << 30, 1 << 20)):
                assert L.mcq_search_range_lists_count(fake, Q, fake, fake, B, N, K, 0, mask, fake, nl, fake, P, fake, fake, fake,
                                                      got - 1, None) == m.MCQ_EWORKSPACE
    assert rl.range_lists_plan(1, c["kListMaxProbes"], 64, 256, c).lds <= 160 * 1024
    for bad in ((0, 8, 8, 256), (4, 0, 8, 256), (4, 4097, 8, 256), (4, 8, 8, 512), (4, 8, 3, 256)):
        assert L.mcq_search_range_lists_workspace_bytes(*bad) == 256


def _tiny():
    rs = np.random.RandomState(9)
    Q, N, K, B = 7, 4, 16, 150
    T = (rs.randint(-64, 64, size=(Q, N, K)) / 8.0).astype(np.float32)      # dyadic: every float32 sum is exact
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    codes[7] = codes[31] = codes[3] = codes[20] = codes[140]
    t = (rs.randint(1, 64, size=B) / 4.0).astype(np.float32)
    t[[3, 7, 20, 31, 140]] = 0.5
    off = np.array([2, 2, 9, 30, 30, 100, 141, 148], dtype=np.int64)        # 7 lists from position 2 on, two empty, 148.. in none
    probes = np.array([[0, 1, 2, 3, 4, 5, 6], [6, 2, 0, -1, 7, 99, -3], [-1] * 7, [1, 3, -1, -1, -1, -1, -1],
                       [5, 4, 2, 1, -1, -1, -1], [2, -1, -1, -1, -1, -1, -1], [5, 2, 5, -1, -1, -1, -1]], dtype=np.int32)
    return Q, N, K, B, T, codes, t, mg.restate_rnorms(t), off, probes


@pytest.mark.parametrize("metric", rl.METRICS)
@pytest.mark.parametrize("pattern", rl.PATTERNS + ("all", "none"))
def test_restatement_against_a_double_loop_and_against_the_union_mask(pattern, metric):
    Q, N, K, B, T, codes, t, r, off, probes = _tiny()
    keep = None if pattern is None else kg.keep_for(pattern, B, 1, 10)
    w = {"l2": t, "ip": None, "cosine": r}[metric]
    s = mg.restate_metric_scores(T, w, codes, metric)
    nl = len(off) - 1
    for shift in range(6):                                   # every query meets every kind of threshold
        thr = rl.thresholds_for(s, off, probes, keep, shift)
        lims, pos, val = rl.restate_range_lists(s, off, probes, thr, keep)
        assert lims[0] == 0 and len(pos) == len(val) == lims[-1]
        for q in range(Q):
            want = []
            for l in probes[q].tolist():                     # the row's own order; a list named twice is walked twice
                if not 0 <= l < nl:
                    continue
                for b in range(int(off[l]), int(off[l + 1])):
                    if keep is not None and not keep[b]:
                        continue
                    S = 0.0
                    for n in range(N):
                        S += float(T[q, n, codes[b, n]])
                    sc = S + float(t[b]) if metric == "l2" else (S if metric == "ip" else float(np.float32(S) * r[b]))
                    if sc <= float(thr[q]):                  # (a NaN threshold compares false)
                        want.append((b, sc))
            got_p, got_v = pos[lims[q]:lims[q + 1]], val[lims[q]:lims[q + 1]]
            assert got_p.tolist() == [b for b, _ in want] and got_v.astype(np.float64).tolist() == [v for _, v in want], (q, shift)
            mode, n_cand = (q + shift) % 6, len(rl.row_positions(off, probes[q]) if keep is None else
                                                 [b for b in rl.row_positions(off, probes[q]) if keep[b]])
            if mode in (0, 5) or n_cand == 0:
                assert len(got_p) == 0
            elif mode == 4:
                assert len(got_p) == n_cand
            elif mode == 1:                                  # inclusive: the smallest score itself is listed
                assert len(got_p) >= 1 and (got_v == got_v.min()).all()
            # rule 18: an ascending row of distinct lists is the masked range restatement under the union mask
            row = rl.sorted_rows(probes[q:q + 1], nl)
            if rl.distinct(off, row[0]):
                a_l, a_p, a_v = rl.restate_range_lists(s[q:q + 1], off, row, thr[q:q + 1], keep)
                u_l, u_p, u_v = kg.restate_range_masked(s[q:q + 1], lg.union_mask(off, row[0], B, keep), thr[q:q + 1])
                assert np.array_equal(a_l, u_l) and np.array_equal(a_p, u_p) and np.array_equal(a_v.view(np.uint32), u_v.view(np.uint32))
                assert sorted(a_p.tolist()) == a_p.tolist() == sorted(got_p.tolist())
    # the row that names list 5 twice lists its hits twice, the second block where the second naming stands
    thr = np.full(Q, np.inf, dtype=np.float32)
    lims, pos, _ = rl.restate_range_lists(s, off, probes, thr, None)
    mine = pos[lims[6]:lims[7]].tolist()
    five, two = list(range(100, 141)), list(range(9, 30))
    assert mine == five + two + five


@pytest.mark.parametrize("case", rl.CASES, ids=lambda c: c.name)
def test_gpu_case_reaches_what_it_claims(case):
    c = rl.constants()
    plan = rl.range_lists_plan(case.Q, case.P, case.N, case.K, c)
    off, probes = rl.layout(case)
    L = len(off) - 1
    assert probes.shape == (case.Q, case.P) and probes.dtype == np.int32 and off.dtype == np.int64
    assert case.B <= 20_000 and case.P <= c["kListMaxProbes"] and 0 <= off[0] and off[-1] <= case.B and (np.diff(off) >= 0).all()
    assert any(not rl.distinct(off, row) for row in probes) == case.twice
    s = rl.host_scores(case)
    thr = rl.thresholds_for(s, off, probes)
    got = rl.reach(s, thr, off, probes, case.B, plan.parts, plan.waves)
    for flag in rl.CLAIMS:
        assert got[flag] == getattr(case, flag), (flag, got)
    # the kinds of threshold the case's queries take, and what they list
    lims, pos, val = rl.restate_range_lists(s, off, probes, thr)
    n = np.diff(lims)
    for q in range(case.Q):
        cand = len(rl.row_positions(off, probes[q]))
        if q % 6 in (0, 5) or cand == 0:
            assert n[q] == 0
        elif q % 6 == 4:
            assert n[q] == cand
        else:
            assert 1 <= n[q] <= cand


def test_case_table_covers_the_ground():
    cs = rl.CASES
    assert [c.base for c in cs[:7]] == lg.CASES and cs[7].base is rl.N4        # the seven of the top-k search, and N = 4
    n4 = cs[7]
    assert (n4.N, n4.K, n4.D, n4.Q, n4.B, n4.P, n4.lists) == (4, 16, 24, 5, 700, 3, "mixed")
    assert {min(c.N, 8) for c in cs} == {1, 2, 4, 8}                           # every chunk width of the dispatcher
    for flag in rl.CLAIMS + ("twice",):
        assert any(getattr(c, flag) for c in cs), flag
    off, probes = rl.layout(n4)
    assert set(np.diff(off).tolist()) >= {0, 1, 63, 64, 65, 130} and any(row.tolist() != sorted(row.tolist()) for row in probes)
    assert any(c.covering for c in cs) and any(c.Q >= 12 for c in cs)          # all six kinds of threshold twice


def test_python_argument_errors_precede_device_work():
    """on CPU tensors: lists of the wrong dtype or shape are a ValueError; right ones that are not on the device are the
    McqError of every other search input"""
    import torch
    m = _lib()
    from quantization_amd import Quantizer
    q = Quantizer(24, 16, 4)
    B = 130
    codes, x = torch.zeros(B, 4, dtype=torch.uint8), torch.zeros(3, 24)
    off = torch.tensor([0, 50, 130], dtype=torch.int64)
    probes = torch.zeros(3, 2, dtype=torch.int32)
    for bad_off in (off.to(torch.int32), off.reshape(1, 3), torch.zeros(0, dtype=torch.int64), [0, 50, 130]):
        with pytest.raises(ValueError, match="list_offsets"):
            q.range_search_lists(x, codes, bad_off, probes, 1.0)
    for bad in (probes.to(torch.float32), torch.zeros((), dtype=torch.int32), [[0, 1]] * 3):
        with pytest.raises(ValueError, match="probes"):
            q.range_search_lists(x, codes, off, bad, 1.0)
    for bad in (torch.zeros(2, 2, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="3 queries"):
            q.range_search_lists(x, codes, off, bad, 1.0)
    with pytest.raises(ValueError):
        q.range_search_lists(x, codes, off, probes, 1.0, metric="dot")
    with pytest.raises(ValueError, match="130"):
        q.range_search_lists(x, codes, off, probes, 1.0, mask=torch.zeros(B - 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        q._search_range(torch.zeros(3, 4, 16), codes, torch.zeros(B), torch.zeros(3), lists=(off.to(torch.int32), probes))
    for good in (probes, probes.to(torch.int64), probes.reshape(1, 3, 2)):
        xq = x.reshape(1, 3, 24) if good.ndim == 3 else x
        for metric in ("l2", "ip", "cosine"):
            with pytest.raises(m.McqError):
                q.range_search_lists(xq, codes, off, good, 1.0, metric=metric)
    with pytest.raises(m.McqError):
        q._search_range(torch.zeros(3, 4, 16), codes, torch.zeros(B), torch.zeros(3), lists=(off, probes))
