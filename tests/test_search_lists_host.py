"""Host-side checks of the search list by list (no GPU): the two symbols are exported and bound, every argument check of rule
16 of include/mcq.h answers before anything touches the device (fake pointers, no launch), the size query equals the mirror
of lists_plan, the numpy restatement of rules 13-15 (tests/search_lists_grid.py) equals a brute-force double loop and the
masked restatement under the union mask of each query, the claims of the GPU case table, the argument errors of the Python
interface that precede any device work, and build_lists / probe_lists against numpy."""
import ctypes

import numpy as np
import pytest

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_exported_and_bound():
    m = _lib()
    L = m.lib()
    hdr = open(sg.HDR.replace("quantization_amd/csrc/mcq_search_kernels.h", "include/mcq.h")).read()
    for name in ("mcq_search_lists_workspace_bytes", "mcq_search_scan_lists"):
        assert name in m.SYMBOLS and hasattr(L, name) and name + "(" in hdr
    assert L.mcq_search_lists_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.mcq_search_scan_lists.argtypes) == 19 and len(L.mcq_search_lists_workspace_bytes.argtypes) == 5
    for rule in (" 13. ", " 14. ", " 15. ", " 16. "):
        assert rule in hdr


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    need = L.mcq_search_lists_workspace_bytes(4, 8, 8, 256, 10)

    def f(tables, Q, codes, w, B, N, K, metric, mask, off, nl, probes, P, outs, ws, ws_bytes, k=10):
        return L.mcq_search_scan_lists(tables, Q, codes, w, B, N, K, k, metric, mask, off, nl, probes, P, outs, outs, ws, ws_bytes,
                                       None)

    for mask in (fake, None):
        # the limits of mcq_search_scan_masked, with its status codes, before any pointer is looked at
        for K in (512, 1024, 8, 2048):
            assert f(None, 4, None, None, 4, 4, K, 0, mask, None, 16, None, 8, None, None, 0) == U
        assert f(None, 4, None, None, 4, 128, 256, 0, mask, None, 16, None, 8, None, None, 0) == U        # N > 64
        assert f(None, 4, None, None, 1 << 31, 8, 256, 0, mask, None, 16, None, 8, None, None, 0) == U    # B > 2^31 - 1
        assert f(None, 4, None, None, 4, 3, 256, 0, mask, None, 16, None, 8, None, None, 0) == I          # N not a power of two
        assert f(None, -1, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, None, None, 0) == I
        assert f(None, 4, None, None, -1, 8, 256, 0, mask, None, 16, None, 8, None, None, 0) == I
        assert f(None, 1 << 31, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, None, None, 0) == I    # Q > 2^31 - 1
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, 1 << 30, k=65) == U
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, 1 << 30, k=0) == I
        for metric in (-1, 3, 7):
            assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, fake, fake, need) == I
        # the new limits
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 4097, fake, fake, 1 << 30) == U
        assert f(None, 4, None, None, 1000, 8, 256, 0, mask, None, 16, None, 4097, None, None, 0) == U
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, -1, fake, fake, need) == I
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, -1, fake, 8, fake, fake, need) == I
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, None, 16, fake, 8, fake, fake, need) == I    # no offsets, L > 0
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, None, 8, fake, fake, need) == I    # no probes, P > 0
        for o in (1, 2, 4, 7, 12):
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, ctypes.c_void_p((1 << 20) + o), 16, fake, 8, fake, fake, need) == I
        for o in (1, 2, 3, 6):
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, ctypes.c_void_p((1 << 20) + o), 8, fake, fake, need) == I
        # the pointers of the masked scan
        assert f(None, 4, None, None, 4, 8, 256, 0, mask, None, 16, None, 8, None, None, 0) == I
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, None, fake, need) == I    # no outputs
        assert f(None, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, need) == I    # no tables
        assert f(fake, 4, None, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, need) == I    # no codes
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, None, need) == I    # no workspace
        assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_L2, mask, fake, 16, fake, 8, fake, fake, need) == I
        assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_COS, mask, fake, 16, fake, 8, fake, fake, need) == I
        assert f(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 0, mask, fake, 16, fake, 8, fake, fake, need) == I
        assert f(fake, 4, ctypes.c_void_p((1 << 20) + 8), fake, 1000, 16, 256, 0, mask, fake, 16, fake, 8, fake, fake, need * 4) == I
        for metric in (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS):                               # a short workspace
            assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, fake, fake, need - 1) == W
            assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, 16, fake, 8, fake, fake, 0) == W
        assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, mask, fake, 16, fake, 8, fake, fake, need - 1) == W
    for o in (1, 2, 4, 7, 12):                               # rule 10: the mask is read as 8-byte words
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, ctypes.c_void_p((1 << 20) + o), fake, 16, fake, 8, fake, fake, need) == I
    # no queries: 0, and no input is looked at (misaligned pointers, no outputs)
    odd = ctypes.c_void_p((1 << 20) + 3)
    assert f(None, 0, odd, None, 1000, 8, 256, 0, odd, odd, 16, odd, 8, None, None, 0) == 0
    assert f(None, 0, None, None, 0, 8, 256, 0, odd, None, 0, None, 0, None, None, 0) == 0
    # an empty store, no lists or no probes need the outputs and look at nothing else: without outputs they are rejected
    # (with them the fill is a launch, which tests/test_gpu_search_lists.py makes)
    for B, nl, P in ((0, 16, 8), (1000, 0, 8), (1000, 16, 0)):
        assert f(None, 4, odd, None, B, 8, 256, 0, odd, odd, nl, odd, P, None, None, 0) == I
    # the limits still come first
    assert f(None, 0, None, None, 1000, 8, 256, 0, None, None, 16, None, 4097, None, None, 0) == U
    assert f(None, 4, None, None, 0, 8, 256, 0, None, None, -1, None, 8, None, None, 0) == I


def test_size_query_equals_the_mirror():
    m = _lib()
    L = m.lib()
    fake = ctypes.c_void_p(1 << 20)
    c = lg.constants()
    for Q, P, N, K, k in ((1, 1, 1, 16, 1), (3, 64, 16, 256, 64), (17, 7, 2, 64, 10), (64, 32, 8, 256, 10), (1024, 128, 8, 256, 10),
                          (5000, 4096, 64, 256, 64), (1, 4096, 8, 256, 10)):
        plan = lg.lists_plan(Q, P, N, K, k, c)
        got = L.mcq_search_lists_workspace_bytes(Q, P, N, K, k)
        assert got == plan.ws_bytes, (Q, P, N, K, k)
        assert 1 <= plan.parts <= c["kScanMaxSlices"] and plan.lds <= 160 * 1024
        for mask in (fake, None):                            # it does not depend on B or L, and one byte less is refused
            for B, nl in ((1000, 16), (1 << 30, 1 << 20)):
                assert L.mcq_search_scan_lists(fake, Q, fake, fake, B, N, K, k, 0, mask, fake, nl, fake, P, fake, fake, fake, got - 1,
                                               None) == m.MCQ_EWORKSPACE
    assert lg.lists_plan(1, c["kListMaxProbes"], 64, 256, 64, c).lds <= 160 * 1024 < lg.lists_plan(1, 2 * c["kListMaxProbes"], 64, 256, 64, c).lds
    assert {lg.lists_plan(Q, 8, 8, 256, 10, c).parts for Q in (1, 3, 17, 64, 1024, 5000)} == {256, 60, 16, 1}
    for bad in ((0, 8, 8, 256, 10), (4, 0, 8, 256, 10), (4, 4097, 8, 256, 10), (4, 8, 8, 512, 10), (4, 8, 8, 256, 65)):
        assert L.mcq_search_lists_workspace_bytes(*bad) == 256


def _tiny():
    rs = np.random.RandomState(9)
    Q, N, K, B = 6, 4, 16, 150
    T = (rs.randint(-64, 64, size=(Q, N, K)) / 8.0).astype(np.float32)      # dyadic: every float32 sum is exact
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    codes[7] = codes[31] = codes[3] = codes[20] = codes[140]
    t = (rs.randint(1, 64, size=B) / 4.0).astype(np.float32)
    t[[3, 7, 20, 31, 140]] = 0.5
    off = np.array([2, 2, 9, 30, 30, 100, 141, 148], dtype=np.int64)        # 7 lists from position 2 on, two empty, 148.. in none
    probes = np.array([[0, 1, 2, 3, 4, 5, 6], [6, 2, 0, -1, 7, 99, -3], [-1] * 7, [1, 3, -1, -1, -1, -1, -1],
                       [5, 4, 2, 1, -1, -1, -1], [2, -1, -1, -1, -1, -1, -1]], dtype=np.int32)
    return Q, N, K, B, T, codes, t, mg.restate_rnorms(t), off, probes


@pytest.mark.parametrize("metric", lg.METRICS)
@pytest.mark.parametrize("pattern", lg.PATTERNS + ("all", "none"))
def test_restatement_against_a_double_loop_and_against_the_union_mask(pattern, metric):
    Q, N, K, B, T, codes, t, r, off, probes = _tiny()
    k = 10
    keep = None if pattern is None else kg.keep_for(pattern, B, 1, k)
    w = {"l2": t, "ip": None, "cosine": r}[metric]
    s = mg.restate_metric_scores(T, w, codes, metric)
    got_s, got_i = lg.restate_lists(s, off, probes, k, keep)
    nl = len(off) - 1
    for q in range(Q):
        pairs = []
        for b in range(B):
            named = any(0 <= l < nl and off[l] <= b < off[l + 1] for l in probes[q].tolist())
            if not named or (keep is not None and not keep[b]):
                continue
            S = 0.0
            for n in range(N):
                S += float(T[q, n, codes[b, n]])
            sc = S + float(t[b]) if metric == "l2" else (S if metric == "ip" else float(np.float32(S) * r[b]))
            pairs.append((sc, b))
        pairs.sort()
        assert len(pairs) == len(lg.candidates(off, probes[q], keep))
        pairs = (pairs + [(np.inf, -1)] * k)[:k]
        assert got_s[q].astype(np.float64).tolist() == [p[0] for p in pairs] and got_i[q].tolist() == [p[1] for p in pairs]
        # rule 14: row 0 of the masked restatement with this one query and the union mask
        u_s, u_i = kg.restate_topk_masked(s[q:q + 1], lg.union_mask(off, probes[q], B, keep), k)
        assert np.array_equal(u_s[0].view(np.uint32), got_s[q].view(np.uint32)) and np.array_equal(u_i[0], got_i[q])
    assert (got_i[2] == -1).all() and np.isinf(got_s[2]).all()                  # a row of padding
    assert pattern is not None or (got_i[3] >= 0).sum() == 7                    # fewer than k candidates


@pytest.mark.parametrize("case", lg.CASES, ids=lambda c: c.name)
def test_gpu_case_reaches_what_it_claims(case):
    c = lg.constants()
    plan = lg.lists_plan(case.Q, case.P, case.N, case.K, case.k, c)
    off, probes = lg.layout(case)
    L = len(off) - 1
    assert probes.shape == (case.Q, case.P) and probes.dtype == np.int32 and off.dtype == np.int64
    assert case.B <= 20_000 and case.P <= c["kListMaxProbes"]
    for row in probes:                                       # rule 13: a row holds distinct lists
        named = [l for l in row.tolist() if 0 <= l < L]
        assert len(named) == len(set(named))
    lens = np.diff(off)
    assert (int(off[0]) == 0 and int(off[-1]) == case.B) == case.covering
    named_rows = [[l for l in row.tolist() if 0 <= l < L] for row in probes]
    assert any(lens[l] == 0 for row in named_rows for l in row) == case.empty_list
    n_cand = [len(lg.candidates(off, row)) for row in probes]
    assert any(0 < n < case.k for n in n_cand) == case.short
    assert any(row != sorted(row) for row in named_rows) == case.unordered
    assert any((row == -1).all() for row in probes) == case.pad_row
    assert any((row == -1).any() and (row == L).any() and ((row > L) | (row < -1)).any() and len(named) > 0
               for row, named in zip(probes, named_rows)) == case.mixed_row
    got = lg.reach(off, probes, case.B, plan.parts, c["kListWaves"])
    for flag in ("cut", "two_steps", "boundary", "empty_part"):
        assert got[flag] == getattr(case, flag), (flag, got)
    # a tie decided across lists: in some query's results one score sits at positions of two different lists
    T, codes, t = lg.host_data(case)
    s = mg.restate_metric_scores(T, t, codes, "l2")
    top_s, top_i = lg.restate_lists(s, off, probes, case.k)
    tie = False
    for q in range(case.Q):
        of = np.searchsorted(off, top_i[q][top_i[q] >= 0], side="right") - 1
        sc = top_s[q][top_i[q] >= 0]
        tie |= any(sc[a] == sc[a + 1] and of[a] != of[a + 1] for a in range(len(sc) - 1))
    assert tie == case.tie_across


def test_case_table_covers_the_ground():
    cs = lg.CASES
    offs = {c.name: lg.layout(c)[0] for c in cs}
    lens = set(np.diff(offs["n2_k64_mixed_p7"]).tolist())
    assert lens >= {0, 1, 63, 64, 65, 130}
    assert any(int(o) % 64 for off in offs.values() for o in off[:-1])          # a list that starts off a multiple of 64
    for flag in ("empty_list", "short", "cut", "two_steps", "boundary", "empty_part", "tie_across", "unordered", "pad_row",
                 "mixed_row", "covering"):
        assert any(getattr(c, flag) for c in cs), flag
    assert {c.Q for c in cs} == {1, 3, 17} and {c.P for c in cs} == {1, 2, 7, 64, 130, 4096}
    assert {(c.N, c.K) for c in cs} == {(1, 16), (2, 64), (8, 256), (16, 256), (64, 256)} and {c.k for c in cs} == {1, 10, 64}
    ones = [c for c in cs if c.P == 4096]
    assert len(ones) == 1 and set(np.diff(offs[ones[0].name]).tolist()) == {1, 2} and len(offs[ones[0].name]) == 4097
    assert any(c.tie_across and c.codes == "dup16" for c in cs)


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
    for bad_off in (off.to(torch.int32), off.to(torch.float32), off.reshape(1, 3), torch.zeros(0, dtype=torch.int64), [0, 50, 130]):
        with pytest.raises(ValueError, match="list_offsets"):
            q.search_lists(x, codes, bad_off, probes)
    for bad in (probes.to(torch.float32), probes.to(torch.int16), torch.zeros((), dtype=torch.int32), [[0, 1]] * 3):
        with pytest.raises(ValueError, match="probes"):
            q.search_lists(x, codes, off, bad)
    for bad in (torch.zeros(2, 2, dtype=torch.int32), torch.zeros(4, 2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(ValueError, match="3 queries"):
            q.search_lists(x, codes, off, bad)
        with pytest.raises(ValueError, match="3 queries"):
            q.search_lists(x, codes, off, bad, metric="ip")
    with pytest.raises(ValueError):
        q.search_lists(x, codes, off, probes, metric="dot")
    with pytest.raises(ValueError, match="130"):
        q.search_lists(x, codes, off, probes, mask=torch.zeros(B - 1, dtype=torch.bool))
    with pytest.raises(ValueError):
        q._search_scan(torch.zeros(3, 4, 16), codes, torch.zeros(B), 10, lists=(off.to(torch.int32), probes))
    for good in (probes, probes.to(torch.int64), probes.reshape(1, 3, 2)):
        xq = x.reshape(1, 3, 24) if good.ndim == 3 else x
        for metric in ("l2", "ip", "cosine"):
            with pytest.raises(m.McqError):
                q.search_lists(xq, codes, off, good, metric=metric)
    with pytest.raises(m.McqError):
        q._search_scan(torch.zeros(3, 4, 16), codes, torch.zeros(B), 10, lists=(off, probes))


def test_build_lists_and_probe_lists_against_numpy():
    import torch
    _lib()
    from quantization_amd import build_lists, probe_lists
    rs = np.random.RandomState(4)
    B, L, D, Q = 1000, 37, 24, 9
    assign = rs.randint(0, L, size=B)
    assign[assign == 5] = 6                                  # an empty list
    for dtype in (torch.int64, torch.int32, torch.uint8):
        order, off = build_lists(torch.from_numpy(assign).to(dtype), L)
        assert order.dtype == torch.int64 and off.dtype == torch.int64 and tuple(order.shape) == (B,) and tuple(off.shape) == (L + 1,)
        assert np.array_equal(order.numpy(), np.argsort(assign, kind="stable"))
        assert np.array_equal(off.numpy(), np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=L))]))
        for l in range(L):
            mine = order.numpy()[off[l]:off[l + 1]]
            assert (assign[mine] == l).all() and (np.diff(mine) > 0).all()
    order, off = build_lists(torch.zeros(0, dtype=torch.int64), 4)
    assert order.numel() == 0 and off.tolist() == [0] * 5
    for bad in (lambda: build_lists(torch.zeros(4), 3), lambda: build_lists(torch.zeros(2, 2, dtype=torch.int64), 3),
                lambda: build_lists(torch.tensor([0, 3]), 3), lambda: build_lists(torch.tensor([-1, 0]), 3),
                lambda: build_lists([0, 1], 3)):
        with pytest.raises(ValueError):
            bad()
    x = rs.randn(Q, D).astype(np.float32)
    cen = rs.randn(L, D).astype(np.float32)
    x64, c64 = x.astype(np.float64), cen.astype(np.float64)
    want = {"l2": -((x64[:, None, :] - c64[None]) ** 2).sum(2), "ip": x64 @ c64.T,
            "cosine": x64 @ c64.T / np.sqrt((c64 ** 2).sum(1))[None, :]}
    for metric, sim in want.items():
        for nprobe in (1, 5, L):
            got = probe_lists(torch.from_numpy(x), torch.from_numpy(cen), nprobe, metric=metric)
            assert got.dtype == torch.int32 and tuple(got.shape) == (Q, nprobe)
            g = got.numpy()
            assert all(len(set(row)) == nprobe for row in g.tolist()) and g.min() >= 0 and g.max() < L
            # the lists it picks are the nprobe best in float64, up to near-ties at the edge; best first
            kth = np.sort(sim, axis=1)[:, ::-1][:, nprobe - 1]
            picked = np.take_along_axis(sim, g.astype(np.int64), axis=1)
            assert (picked >= kth[:, None] - 1e-4).all() and (np.diff(picked, axis=1) <= 1e-4).all()
    got = probe_lists(torch.from_numpy(x).reshape(3, 3, D), torch.from_numpy(cen), 4)
    assert tuple(got.shape) == (3, 3, 4)
    for bad in (lambda: probe_lists(torch.from_numpy(x), torch.from_numpy(cen), 0), lambda: probe_lists(torch.from_numpy(x), torch.from_numpy(cen), L + 1),
                lambda: probe_lists(torch.from_numpy(x), torch.from_numpy(cen[:, :5]), 2),
                lambda: probe_lists(torch.from_numpy(x), torch.from_numpy(cen), 2, metric="dot")):
        with pytest.raises(ValueError):
            bad()
