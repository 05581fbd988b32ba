"""Host-side checks of the range search over stored codes (no GPU): argument validation that precedes any launch (rule 9 of
include/mcq.h), the workspace rules, the numpy restatement of rules 7 and 8 (tests/search_range_grid.py) against a brute-force
double loop, and the claims of the GPU case table against the mirror of the launch arithmetic and against the restatement."""
import ctypes

import numpy as np
import pytest

import search_grid as sg
import search_metric_grid as mg
import search_range_grid as rg


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def _count(L, tables, Q, codes, w, B, N, K, metric, thr, lims, ws, ws_bytes):
    return L.mcq_search_range_count(tables, Q, codes, w, B, N, K, metric, thr, lims, ws, ws_bytes, None)


def _fill(L, tables, Q, codes, w, B, N, K, metric, thr, lims, out_s, out_i, cap, ws, ws_bytes):
    return L.mcq_search_range_fill(tables, Q, codes, w, B, N, K, metric, thr, lims, out_s, out_i, cap, ws, ws_bytes, None)


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    need = L.mcq_search_range_workspace_bytes(4, 1000, 8, 256)
    for call in ("count", "fill"):
        def f(tables, Q, codes, w, B, N, K, metric, thr, lims, ws, ws_bytes, out=fake, cap=100):
            if call == "count":
                return _count(L, tables, Q, codes, w, B, N, K, metric, thr, lims, ws, ws_bytes)
            return _fill(L, tables, Q, codes, w, B, N, K, metric, thr, lims, out, out, cap, ws, ws_bytes)
        # the domain, before any pointer is looked at: one-byte codes, the (N, K) domain of the library, B <= 2^31 - 1
        for K in (512, 1024, 8, 2048):
            assert f(None, 4, None, None, 4, 4, K, 0, None, None, None, 0) == U
        assert f(None, 4, None, None, 4, 128, 256, 0, None, None, None, 0) == U            # N > 64
        assert f(None, 4, None, None, 1 << 31, 8, 256, 0, None, None, None, 0) == U        # B > 2^31 - 1
        # bad shapes, negative sizes, an unknown metric, null pointers
        assert f(None, 4, None, None, 4, 3, 256, 0, None, None, None, 0) == I              # N not a power of two
        assert f(None, -1, None, None, 4, 8, 256, 0, None, None, None, 0) == I
        assert f(None, 4, None, None, -1, 8, 256, 0, None, None, None, 0) == I
        assert f(None, 1 << 31, None, None, 4, 8, 256, 0, None, None, None, 0) == I        # Q > 2^31 - 1
        for metric in (-1, 3, 7):
            assert f(fake, 4, fake, fake, 1000, 8, 256, metric, fake, fake, fake, need) == I
        assert f(None, 4, None, None, 4, 8, 256, 0, None, None, None, 0) == I              # null pointers
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, fake, None, fake, need) == I        # no lims
        assert f(None, 0, None, None, 4, 8, 256, 0, None, None, None, 0) == I              # ... which even Q == 0 needs
        assert f(None, 4, fake, fake, 1000, 8, 256, 0, fake, fake, fake, need) == I        # no tables
        assert f(fake, 4, None, fake, 1000, 8, 256, 0, fake, fake, fake, need) == I        # no codes
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, None, fake, fake, need) == I        # no thresholds
        assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_L2, fake, fake, fake, need) == I      # w == NULL only for IP
        assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_COS, fake, fake, fake, need) == I
        # a short workspace and misaligned codes are refused before the device is touched: the pointers are never read
        for metric in (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS):
            assert f(fake, 4, fake, fake, 1000, 8, 256, metric, fake, fake, fake, need - 1) == W
            assert f(fake, 4, fake, fake, 1000, 8, 256, metric, fake, fake, fake, 0) == W
        assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, fake, fake, fake, need - 1) == W  # (w is not missed)
        assert f(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 0, fake, fake, fake, need) == I
        assert f(fake, 4, ctypes.c_void_p((1 << 20) + 8), fake, 1000, 16, 256, 0, fake, fake, fake, need * 4) == I
        assert f(fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, None, need) == I        # no workspace at all
    # the fill alone: a negative capacity, no output arrays; no room means nothing to do
    assert _fill(L, fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, fake, fake, -1, fake, need) == I
    assert _fill(L, fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, None, fake, 10, fake, need) == I
    assert _fill(L, fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, fake, None, 10, fake, need) == I
    assert _fill(L, fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, None, None, 0, fake, need) == 0
    # rule 9: an empty store or no queries leave the fill nothing to write, whatever else is null
    assert _fill(L, None, 0, None, None, 1000, 8, 256, 0, None, fake, None, None, 0, None, 0) == 0
    assert _fill(L, None, 4, None, None, 0, 8, 256, 0, None, fake, None, None, 10, None, 0) == 0


def test_workspace_rules():
    L = _lib().lib()
    c = rg.constants()
    w = L.mcq_search_range_workspace_bytes
    # one int64 per (query, slice, wave): nothing depends on D (there is no such argument) nor on the number of results
    a, b, big, bigger = w(64, 1000, 8, 256), w(64, 65536, 8, 256), w(64, 1 << 20, 8, 256), w(64, (1 << 31) - 1, 8, 256)
    assert a < b <= big and big == bigger                      # the slice count reached its cap: the workspace stops growing
    assert big <= sg.align256(64 * c["kScanMaxSlices"] * c["kRangeWaves"] * 8)
    assert w(1, (1 << 31) - 1, 8, 256) <= sg.align256(c["kScanMaxSlices"] * c["kRangeWaves"] * 8)
    assert w(1024, 1 << 20, 8, 256) > w(64, 1 << 20, 8, 256) // 4
    # outside the domain: slack only
    assert w(64, 1000, 8, 512) == w(0, 1000, 8, 256) == w(64, 0, 8, 256) == w(64, 1 << 31, 8, 256) == w(64, 1000, 3, 256) == 256
    # the mirror is the library's arithmetic
    for Q in (1, 2, 3, 15, 16, 17, 200, 1024, 5000):
        for B in (1, 63, 64, 65, 1023, 1024, 1025, 4099, 100_003, rg.BIG, (1 << 31) - 1):
            for N, K in ((1, 16), (8, 256), (64, 256), (16, 16), (2, 64), (32, 256), (16, 256)):
                p = rg.range_plan(Q, B, N, K, c)
                assert w(Q, B, N, K) == p.ws_bytes, (Q, B, N, K)
                assert 1 <= p.slices <= c["kScanMaxSlices"] and p.slices * p.per_slice >= B > (p.slices - 1) * p.per_slice
                assert p.per_slice % 64 == 0 and p.qt * p.qtiles >= Q
                assert p.lds <= c["kScanTableLds"] + c["kRangeWaves"] * c["kScanQTMax"] * 8 <= 160 * 1024
                for s in (0, p.slices - 1):                     # every step of a slice belongs to exactly one wave
                    steps = (p.slice_len(B, s) + 63) // 64
                    assert p.run(B, s) * p.waves >= steps > (p.run(B, s) - 1) * p.waves


def test_restatement_against_a_double_loop():
    """rules 7 and 8 in numpy (what the GPU tests compare with, bit for bit) against a brute-force double loop in float64:
    dyadic table entries make every float32 sum exact, planted duplicate codes make ties sit on the threshold"""
    rs = np.random.RandomState(5)
    Q, N, K, B = 6, 4, 16, 90
    T = (rs.randint(-64, 64, size=(Q, N, K)) / 8.0).astype(np.float32)
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    codes[7] = codes[31] = codes[3] = codes[20]              # four identical rows
    t = (rs.randint(0, 64, size=B) / 4.0).astype(np.float32)
    t[[3, 7, 20, 31]] = 0.5
    r = mg.restate_rnorms(t)
    for metric, w in (("l2", t), ("ip", None), ("cosine", r)):
        s = mg.restate_metric_scores(T, w, codes, metric)
        thr = np.array([s[0, 20], -np.inf, np.inf, np.nan, np.median(s[4]), s[5].min()], dtype=np.float32)
        got_thr, lims, pos, val = rg.restate(T, w, codes, metric, thr=thr, qchunk=4)
        assert np.array_equal(got_thr.view(np.uint32), thr.view(np.uint32)) and lims[0] == 0 and len(lims) == Q + 1
        want_pos, want_val, want_lims = [], [], [0]
        for q in range(Q):
            for b in range(B):
                S = 0.0
                for n in range(N):
                    S += float(T[q, n, codes[b, n]])
                sc = S + float(t[b]) if metric == "l2" else (S if metric == "ip" else float(np.float32(S) * r[b]))
                if sc <= float(thr[q]):
                    want_pos.append(b)
                    want_val.append(sc)
            want_lims.append(len(want_pos))
        assert lims.tolist() == want_lims and pos.tolist() == want_pos
        assert val.astype(np.float64).tolist() == want_val
        assert lims[2] == lims[1] and lims[3] - lims[2] == B and lims[4] == lims[3]       # -inf, +inf, NaN
        assert {3, 7, 20, 31} <= set(pos[:lims[1]].tolist())                               # the tie on the threshold is listed whole
        assert lims[6] - lims[5] >= 1                                                       # inclusive: the minimum itself
    # the thresholds of the case table: by q mod 4 a score that occurs, -inf, +inf, a value between two scores
    s = mg.restate_metric_scores(T, t, codes, "l2")
    thr = rg.thresholds_for(s)
    n, _, _ = rg.restate_range(s, thr)
    assert thr[0] in s[0] and thr[4] in s[4] and n[0] >= 10 and n[1] == 0 and n[2] == B and 1 <= n[3] < 10
    assert np.array_equal(rg.thresholds_for(s[2:], 2), thr[2:])
    # a NaN score is never listed, not even under +inf
    s[2, 5] = np.nan
    assert rg.restate_range(s, thr)[0][2] == B - 1


@pytest.mark.parametrize("case", rg.CASES, ids=lambda c: c.name)
def test_gpu_case_reaches_what_it_claims(case):
    c = rg.constants()
    p = rg.range_plan(case.Q, case.B, case.N, case.K, c)
    assert (p.qtiles > 1) == case.tiles, p
    assert (p.slices > 1) == case.sliced, p
    assert p.multi_step(case.B) == case.multi, p
    assert p.last_step_partial(case.B) == case.partial, p
    assert p.idle_waves(case.B) == case.idle, p
    if case.tiles:
        assert case.Q % p.qt != 0                               # ... and the last tile is a partial one
    # the shape of the result, on grid-valued tables (exact ties exist) and codes of the case's kind
    rs = np.random.RandomState(case.B % 1009 + case.N)
    T = (rs.randint(-64, 64, size=(case.Q, case.N, case.K)) / 8.0).astype(np.float32)
    codes = rg.host_codes(case, rs)
    t = (rs.randint(1, 64, size=case.B) / 4.0).astype(np.float32)
    for metric in rg.METRICS:
        w = None if metric == "ip" else (t if metric == "l2" else mg.restate_rnorms(t))
        thr, lims, pos, val = rg.restate(T, w, codes, metric)
        n = np.diff(lims)
        assert lims[0] == 0 and lims[-1] == len(pos) == len(val) and (n >= 0).all()
        for q in range(case.Q):
            a = pos[lims[q]:lims[q + 1]]
            assert (np.diff(a) > 0).all()                       # ascending position
        on_thr = [int((val[lims[q]:lims[q + 1]] == thr[q]).sum()) for q in range(case.Q)]
        assert all(on_thr[q] >= 1 for q in range(0, case.Q, 4))   # inclusivity: the threshold is a score that occurs, and is listed
        if case.empty:
            assert (n == 0).any()
        if case.full:
            assert (n == case.B).any()
        if case.ties:
            assert max(on_thr) >= 8


def test_case_table_covers_the_ground():
    cs = rg.CASES
    for flag in ("tiles", "sliced", "multi", "partial", "idle", "empty", "full", "ties"):
        assert sum(bool(getattr(c, flag)) for c in cs) >= 2, flag
        assert not all(getattr(c, flag) for c in cs), flag
    assert {c.N for c in cs} >= {1, 2, 8, 16, 64} and {c.K for c in cs} == {16, 64, 256}
    assert any(c.packed and c.K == 16 for c in cs) and any(c.queries == "fp16" for c in cs)
    assert any(c.state == "decode_only" for c in cs) and any(c.state == "trained" for c in cs)
    assert any(c.codes == "dup16" and c.ties for c in cs)
    assert any(c.B == 1_048_576 + 17 for c in cs) and {c.B for c in cs} >= {1, 63, 64, 65}
    assert {c.Q for c in cs} >= {1, 17, 200}
