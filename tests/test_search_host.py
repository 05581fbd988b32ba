"""Host-side checks of the search over stored codes (no GPU): argument validation that precedes any launch, the workspace
rules, the numpy restatement of rules 3 and 4 (tests/search_grid.py) against a brute-force float64 ranking, and the claims of
the GPU case table against the mirror of the launch arithmetic."""
import ctypes

import numpy as np
import pytest

import search_grid as sg


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    # the domain: one-byte codes, the (N, K) domain of the library, k <= 64, B <= 2^31 - 1 -- before any pointer is looked at
    for K in (512, 1024, 8, 2048):
        assert L.mcq_search_tables(None, 0, 4, None, 4, K, 64, None, None) == U
        assert L.mcq_code_norms(None, 4, None, 4, K, 64, None, None) == U
        assert L.mcq_search_scan(None, 4, None, None, 4, 4, K, 10, None, None, None, 0, None) == U
    assert L.mcq_search_scan(None, 4, None, None, 4, 128, 256, 10, None, None, None, 0, None) == U     # N > 64
    assert L.mcq_search_scan(None, 4, None, None, 4, 8, 256, 65, None, None, None, 0, None) == U       # k > 64
    assert L.mcq_search_scan(None, 4, None, None, 1 << 31, 8, 256, 10, None, None, None, 0, None) == U  # B > 2^31 - 1
    assert L.mcq_code_norms(None, 1 << 31, None, 8, 256, 64, None, None) == U
    assert L.mcq_search_tables(None, 0, 4, None, 8, 256, 20000, None, None) == U                       # dim past 16,384
    # bad shapes, negative sizes, null pointers
    assert L.mcq_search_scan(None, 4, None, None, 4, 3, 256, 10, None, None, None, 0, None) == I       # N not a power of two
    assert L.mcq_search_scan(None, 4, None, None, 4, 8, 256, 0, None, None, None, 0, None) == I        # k < 1
    assert L.mcq_search_scan(None, -1, None, None, 4, 8, 256, 10, None, None, None, 0, None) == I
    assert L.mcq_search_scan(None, 4, None, None, -1, 8, 256, 10, None, None, None, 0, None) == I
    assert L.mcq_search_scan(None, 4, None, None, 4, 8, 256, 10, None, None, None, 0, None) == I       # null pointers
    assert L.mcq_search_tables(None, 0, -1, None, 8, 256, 64, None, None) == I
    assert L.mcq_search_tables(None, 0, 4, None, 8, 256, 64, None, None) == I
    assert L.mcq_code_norms(None, -1, None, 8, 256, 64, None, None) == I
    assert L.mcq_code_norms(None, 4, None, 8, 256, 64, None, None) == I
    # nothing to do: no pointer is needed
    assert L.mcq_search_tables(None, 0, 0, None, 8, 256, 64, None, None) == 0
    assert L.mcq_code_norms(None, 0, None, 8, 256, 64, None, None) == 0
    assert L.mcq_search_scan(None, 0, None, None, 4, 8, 256, 10, None, None, None, 0, None) == 0
    # a short workspace and misaligned codes are refused before the device is touched: the pointers below are never read
    fake = ctypes.c_void_p(1 << 20)
    need = L.mcq_search_workspace_bytes(4, 1000, 8, 256, 10)
    assert L.mcq_search_scan(fake, 4, fake, fake, 1000, 8, 256, 10, fake, fake, fake, need - 1, None) == W
    assert L.mcq_search_scan(fake, 4, fake, fake, 1000, 8, 256, 10, fake, fake, fake, 0, None) == W
    assert L.mcq_search_scan(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 10, fake, fake, fake, need, None) == I
    assert L.mcq_search_scan(fake, 4, fake, fake, 1000, 8, 256, 10, fake, fake, None, need, None) == I  # no workspace at all


def test_workspace_rules():
    L = _lib().lib()
    c = sg.constants()
    w = L.mcq_search_workspace_bytes
    # partial lists only: k entries of 8 bytes per (query, slice); nothing depends on D (the query has no such argument)
    a, b, big, bigger = w(64, 1000, 8, 256, 10), w(64, 65536, 8, 256, 10), w(64, 1 << 20, 8, 256, 10), w(64, 1 << 30, 8, 256, 10)
    assert a < b <= big and big == bigger                      # the slice count reached its cap: the workspace stops growing
    assert big <= 2 * sg.align256(64 * c["kScanMaxSlices"] * 10 * 4)
    assert w(1, 1 << 30, 8, 256, 64) <= 2 * sg.align256(c["kScanMaxSlices"] * 64 * 4)
    assert w(64, 1 << 20, 8, 256, 64) > w(64, 1 << 20, 8, 256, 10) > w(64, 1 << 20, 8, 256, 1)
    assert w(1024, 1 << 20, 8, 256, 10) > w(64, 1 << 20, 8, 256, 10) // 4
    # outside the domain: slack only
    assert w(64, 1000, 8, 512, 10) == w(64, 1000, 8, 256, 65) == w(0, 1000, 8, 256, 10) == w(64, 0, 8, 256, 10) == 256
    # the mirror is the library's arithmetic
    for Q in (1, 2, 15, 16, 17, 200, 1024, 5000):
        for B in (1, 63, 64, 65, 511, 512, 513, 4099, 100_003, sg.BIG, (1 << 31) - 1):
            for N, K in ((1, 16), (8, 256), (64, 256), (16, 16), (2, 64), (32, 256)):
                for k in (1, 10, 64):
                    p = sg.scan_plan(Q, B, N, K, k, c)
                    assert w(Q, B, N, K, k) == p.ws_bytes, (Q, B, N, K, k)
                    assert 1 <= p.slices <= c["kScanMaxSlices"] and p.slices * p.per_slice >= B > (p.slices - 1) * p.per_slice
                    assert p.per_slice % 64 == 0 and p.lds <= c["kScanTableLds"] and p.qt * p.qtiles >= Q


def test_restatement_breaks_ties_by_position():
    """rules 3 and 4 in numpy (what the GPU tests compare with, bit for bit) against a brute-force float64 ranking: dyadic
    table entries make every float32 sum exact, and planted duplicate codes make ties decide the list"""
    rs = np.random.RandomState(5)
    Q, N, K, B, k = 3, 4, 16, 40, 12
    T = (rs.randint(-64, 64, size=(Q, N, K)) / 8.0).astype(np.float32)
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    codes[7] = codes[31] = codes[3] = codes[20]              # four identical rows
    codes[11] = codes[2]
    t = (rs.randint(0, 64, size=B) / 4.0).astype(np.float32)
    t[[3, 7, 20, 31]] = 0.0                                    # ... with equal norms: equal scores, and small ones
    t[11] = t[2] = 0.25
    for q in range(Q):
        for n in range(N):
            T[q, n, codes[20, n]] = -8.0                       # make the duplicated row the best of every query
    got_s, got_i = sg.restate(T, t, codes, k)
    for q in range(Q):
        s64 = [sum(float(T[q, n, codes[b, n]]) for n in range(N)) + float(t[b]) for b in range(B)]
        order = sorted(range(B), key=lambda b: (s64[b], b))[:k]
        assert got_i[q].tolist() == order
        assert got_s[q].astype(np.float64).tolist() == [s64[b] for b in order]
        assert got_i[q, :4].tolist() == [3, 7, 20, 31]         # the tie is broken by position
    # fewer candidates than k: the tail is (+inf, -1)
    s, i = sg.restate(T, t[:5], codes[:5], k)
    assert (i[:, 5:] == -1).all() and np.isinf(s[:, 5:]).all() and (i[:, :5] >= 0).all()
    s, i = sg.restate(T, t[:0], codes[:0], k)
    assert (i == -1).all() and np.isinf(s).all()
    # the large-store path of restate_topk (partition first) agrees with the plain stable sort
    B2 = 500
    codes2 = rs.randint(0, 2, size=(B2, N)).astype(np.uint8)   # 16 distinct rows: every score is shared
    s2 = sg.restate_scores(T, np.zeros(B2, np.float32), codes2)
    a_s, a_i = sg.restate_topk(s2, k)
    for q in range(Q):
        order = np.argsort(s2[q], kind="stable")[:k]
        assert a_i[q].tolist() == order.tolist() and a_s[q].tolist() == s2[q][order].tolist()


def test_gpu_cases_reach_what_they_claim():
    c = sg.constants()
    seen = dict(tiles=0, sliced=0, partial=0, short=0, strided=0)
    for case in sg.CASES:
        p = sg.scan_plan(case.Q, case.B, case.N, case.K, case.k, c)
        assert (p.qtiles > 1) == case.tiles, (case.name, p)
        assert (p.slices > 1) == case.sliced, (case.name, p)
        assert p.last_step_partial(case.B) == case.partial, (case.name, p)
        assert (case.B < case.k) == case.short, case.name
        assert (p.per_slice // 64 > c["kScanWaves"]) == case.strided, (case.name, p)
        assert p.lds <= c["kScanTableLds"]
        if case.tiles:
            assert case.Q % p.qt != 0, case.name                 # ... and the last tile is a partial one
        for f in seen:
            seen[f] += bool(getattr(case, f))
    assert all(v >= 2 for v in seen.values()), seen
    # the table kernel: more than one query tile, and a partial last one, wherever the scan has them
    for case in sg.CASES:
        gq, gr = sg.tables_grid(case.Q, case.N, case.K, c)
        if case.Q > c["kTabQueries"]:
            assert gq > 1 and case.Q % c["kTabQueries"] != 0
        assert gr * c["kTabRows"] >= case.N * case.K
    # ties decide whole lists both where arrival order is position order and where it is not
    assert {cs.strided for cs in sg.CASES if cs.codes == "dup16" and cs.k == 64} == {False, True}
    assert {cs.N for cs in sg.CASES} >= {1, 2, 8, 16, 64} and {cs.K for cs in sg.CASES} == {16, 64, 256}
    assert {cs.D for cs in sg.CASES} == {24, 40, 512, 1000} and {cs.Q for cs in sg.CASES} == {1, 5, 17, 200}
    assert {sg.padded(cs.D) % c["kTabChunk"] for cs in sg.CASES} == {0, 16}      # whole chunks, and half a last one
    assert {cs.k for cs in sg.CASES} == {1, 10, 64}
    assert {cs.B for cs in sg.CASES} >= {1, 63, 64, 65, 9, 100_003, 1_048_576 + 17}
