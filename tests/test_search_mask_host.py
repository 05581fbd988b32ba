"""Host-side checks of the search under a mask (no GPU): argument validation that precedes any launch for the three masked
calls and for mcq_search_pack_mask (rules 10-12 of include/mcq.h), the workspace sizes, the numpy restatement of rules 10 and
11 (tests/search_mask_grid.py) against a brute-force double loop and against "compact, restate without a mask, map back", the
claims of the GPU case table, and the argument errors of the Python interface that precede any device work."""
import ctypes

import numpy as np
import pytest

import search_grid as sg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def _calls(L, fake):
    """the three masked calls with one argument list: (tables, Q, codes, w, B, N, K, metric, mask, thr, lims, ws, ws_bytes);
    the scan takes k = 10 and out arrays where the sweeps take thr and lims (both stand or fall with `lims` here)"""
    def scan(tables, Q, codes, w, B, N, K, metric, mask, thr, lims, ws, ws_bytes):
        return L.mcq_search_scan_masked(tables, Q, codes, w, B, N, K, 10, metric, mask, lims, lims, ws, ws_bytes, None)

    def count(tables, Q, codes, w, B, N, K, metric, mask, thr, lims, ws, ws_bytes):
        return L.mcq_search_range_count_masked(tables, Q, codes, w, B, N, K, metric, mask, thr, lims, ws, ws_bytes, None)

    def fill(tables, Q, codes, w, B, N, K, metric, mask, thr, lims, ws, ws_bytes):
        return L.mcq_search_range_fill_masked(tables, Q, codes, w, B, N, K, metric, mask, thr, lims, fake, fake, 100, ws,
                                              ws_bytes, None)
    return {"scan": scan, "count": count, "fill": fill}


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    fake = ctypes.c_void_p(1 << 20)
    needs = {"scan": L.mcq_search_workspace_bytes(4, 1000, 8, 256, 10), "count": L.mcq_search_range_workspace_bytes(4, 1000, 8, 256),
             "fill": L.mcq_search_range_workspace_bytes(4, 1000, 8, 256)}
    for name, f in _calls(L, fake).items():
        need = needs[name]
        for mask in (fake, None):                                # the table of test_search_range_host.py, with and without a mask
            for K in (512, 1024, 8, 2048):
                assert f(None, 4, None, None, 4, 4, K, 0, mask, None, None, None, 0) == U
            assert f(None, 4, None, None, 4, 128, 256, 0, mask, None, None, None, 0) == U          # N > 64
            assert f(None, 4, None, None, 1 << 31, 8, 256, 0, mask, None, None, None, 0) == U      # B > 2^31 - 1
            assert f(None, 4, None, None, 4, 3, 256, 0, mask, None, None, None, 0) == I            # N not a power of two
            assert f(None, -1, None, None, 4, 8, 256, 0, mask, None, None, None, 0) == I
            assert f(None, 4, None, None, -1, 8, 256, 0, mask, None, None, None, 0) == I
            assert f(None, 1 << 31, None, None, 4, 8, 256, 0, mask, None, None, None, 0) == I      # Q > 2^31 - 1
            for metric in (-1, 3, 7):
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, fake, fake, need) == I
            assert f(None, 4, None, None, 4, 8, 256, 0, mask, None, None, None, 0) == I            # null pointers
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, None, fake, need) == I      # no lims / no outputs
            assert f(None, 4, fake, fake, 1000, 8, 256, 0, mask, fake, fake, fake, need) == I      # no tables
            assert f(fake, 4, None, fake, 1000, 8, 256, 0, mask, fake, fake, fake, need) == I      # no codes
            if name != "scan":
                assert f(None, 0, None, None, 4, 8, 256, 0, mask, None, None, None, 0) == I        # lims: even Q == 0 needs it
                assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, None, fake, fake, need) == I  # no thresholds
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_L2, mask, fake, fake, fake, need) == I   # w == NULL: IP only
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_COS, mask, fake, fake, fake, need) == I
            for metric in (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS):                    # a short workspace
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, fake, fake, need - 1) == W
                assert f(fake, 4, fake, fake, 1000, 8, 256, metric, mask, fake, fake, fake, 0) == W
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, mask, fake, fake, fake, need - 1) == W
            assert f(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 0, mask, fake, fake, fake, need) == I
            assert f(fake, 4, ctypes.c_void_p((1 << 20) + 8), fake, 1000, 16, 256, 0, mask, fake, fake, fake, need * 4) == I
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, mask, fake, fake, None, need) == I      # no workspace at all
        # rule 10: the mask is read as 8-byte words
        for off in (1, 2, 4, 7, 12):
            assert f(fake, 4, fake, fake, 1000, 8, 256, 0, ctypes.c_void_p((1 << 20) + off), fake, fake, fake, need) == I
            assert f(fake, 4, fake, None, 1000, 8, 256, m.MCQ_SEARCH_IP, ctypes.c_void_p((1 << 20) + off), fake, fake, fake, need) == I
    # rules 4 and 9: no queries or an empty store look at no input, the mask included (a misaligned one too)
    odd = ctypes.c_void_p((1 << 20) + 3)
    assert L.mcq_search_scan_masked(None, 0, None, None, 1000, 8, 256, 10, 0, odd, None, None, None, 0, None) == 0
    assert L.mcq_search_range_fill_masked(None, 0, None, None, 1000, 8, 256, 0, odd, None, fake, None, None, 0, None, 0, None) == 0
    assert L.mcq_search_range_fill_masked(None, 4, None, None, 0, 8, 256, 0, odd, None, fake, None, None, 10, None, 0, None) == 0
    assert L.mcq_search_range_fill_masked(fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, fake, fake, fake, -1, fake, needs["fill"],
                                          None) == I
    assert L.mcq_search_range_fill_masked(fake, 4, fake, fake, 1000, 8, 256, 0, fake, fake, fake, None, None, 0, fake, needs["fill"],
                                          None) == 0                                               # no room: nothing to do
    assert L.mcq_search_scan_masked(fake, 4, fake, fake, 1000, 8, 256, 65, 0, fake, fake, fake, fake, 1 << 30, None) == U   # k > 64
    assert L.mcq_search_scan_masked(fake, 4, fake, fake, 1000, 8, 256, 0, 0, fake, fake, fake, fake, 1 << 30, None) == I    # k < 1


def test_pack_mask_validation_without_launch():
    m = _lib()
    L = m.lib()
    fake = ctypes.c_void_p(1 << 20)
    assert L.mcq_search_pack_mask(None, 0, None, None) == 0                                        # B == 0 writes nothing
    assert L.mcq_search_pack_mask(fake, -1, fake, None) == m.MCQ_EINVAL
    assert L.mcq_search_pack_mask(None, 1 << 31, None, None) == m.MCQ_EUNSUPPORTED                 # B > 2^31 - 1
    assert L.mcq_search_pack_mask(None, 100, fake, None) == m.MCQ_EINVAL
    assert L.mcq_search_pack_mask(fake, 100, None, None) == m.MCQ_EINVAL
    assert L.mcq_search_pack_mask(fake, 100, ctypes.c_void_p((1 << 20) + 4), None) == m.MCQ_EINVAL


def test_masked_workspace_sizes_are_the_unmasked_ones():
    """there is no size query of its own: the plan of a call does not depend on the mask, and a workspace one byte short of
    what the unmasked query returns is refused with a mask as without"""
    m = _lib()
    L = m.lib()
    fake = ctypes.c_void_p(1 << 20)
    calls = _calls(L, fake)
    for Q, B, N, K in ((1, 1, 1, 16), (17, 4099, 8, 256), (200, 40_000, 8, 256), (258, 70_000, 64, 256), (64, 1 << 20, 8, 256)):
        scan, sweep = L.mcq_search_workspace_bytes(Q, B, N, K, 10), L.mcq_search_range_workspace_bytes(Q, B, N, K)
        assert scan == sg.scan_plan(Q, B, N, K, 10).ws_bytes and sweep == rg.range_plan(Q, B, N, K).ws_bytes
        for name, need in (("scan", scan), ("count", sweep), ("fill", sweep)):
            for mask in (fake, None):
                assert calls[name](fake, Q, fake, fake, B, N, K, 0, mask, fake, fake, fake, need - 1) == m.MCQ_EWORKSPACE


def _tiny():
    rs = np.random.RandomState(9)
    Q, N, K, B = 5, 4, 16, 150
    T = (rs.randint(-64, 64, size=(Q, N, K)) / 8.0).astype(np.float32)      # dyadic: every float32 sum is exact
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    codes[7] = codes[31] = codes[3] = codes[20] = codes[140]
    t = (rs.randint(1, 64, size=B) / 4.0).astype(np.float32)
    t[[3, 7, 20, 31, 140]] = 0.5
    return Q, N, K, B, T, codes, t, mg.restate_rnorms(t)


def test_packing_is_numpy_packbits():
    for B in (1, 63, 64, 65, 130, 4099):
        for pattern in kg.PATTERNS:
            keep, words = kg.words_for(pattern, B, 3, 10)
            assert words.dtype == np.int64 and words.shape == (kg.words_of(B),)
            for b in (0, B // 2, B - 1):
                assert bool((int(words.view(np.uint64)[b >> 6]) >> (b & 63)) & 1) == bool(keep[b])
            assert np.array_equal(kg.unpack(words, B), keep)
            raw = np.packbits(keep, bitorder="little")
            if pattern != "garbage_tail":
                assert np.array_equal(words.view(np.uint8)[:len(raw)], raw) and not words.view(np.uint8)[len(raw):].any()
            elif B % 64:
                assert int(words.view(np.uint64)[-1]) >> (B % 64) == (1 << (64 - B % 64)) - 1


@pytest.mark.parametrize("metric", kg.METRICS)
@pytest.mark.parametrize("pattern", kg.PATTERNS)
def test_restatement_against_a_double_loop_and_against_compaction(pattern, metric):
    Q, N, K, B, T, codes, t, r = _tiny()
    k = 10
    keep, words = kg.words_for(pattern, B, 1, k)
    assert np.array_equal(kg.unpack(words, B), keep)
    w = {"l2": t, "ip": None, "cosine": r}[metric]
    s = mg.restate_metric_scores(T, w, codes, metric)
    thr = np.array([s[0, 20], -np.inf, np.inf, np.median(s[3]), s[4].min()], dtype=np.float32)
    got_s, got_i = kg.restate_topk_masked(s, keep, k)
    lims, pos, val = kg.restate_range_masked(s, keep, thr)
    # the double loop, in float64 (exact on these tables)
    want_lims, want_pos, want_val = [0], [], []
    for q in range(Q):
        pairs = []
        for b in range(B):
            if not (int(words.view(np.uint64)[b >> 6]) >> (b & 63)) & 1:
                continue
            S = 0.0
            for n in range(N):
                S += float(T[q, n, codes[b, n]])
            sc = S + float(t[b]) if metric == "l2" else (S if metric == "ip" else float(np.float32(S) * r[b]))
            pairs.append((sc, b))
            if sc <= float(thr[q]):
                want_pos.append(b)
                want_val.append(sc)
        want_lims.append(len(want_pos))
        pairs.sort()
        pairs = (pairs + [(np.inf, -1)] * k)[:k]
        assert got_s[q].astype(np.float64).tolist() == [p[0] for p in pairs] and got_i[q].tolist() == [p[1] for p in pairs]
    assert lims.tolist() == want_lims and pos.tolist() == want_pos and val.astype(np.float64).tolist() == want_val
    # rule 11's equivalence: the unmasked restatement over the compacted store, mapped back
    c_s, c_i = kg.compact_topk(T, w, codes, k, metric, keep)
    assert np.array_equal(c_s.view(np.uint32), got_s.view(np.uint32)) and np.array_equal(c_i, got_i)
    c_lims, c_pos, c_val = kg.compact_range(T, w, codes, metric, keep, thr)
    assert np.array_equal(c_lims, lims) and np.array_equal(c_pos, pos) and np.array_equal(c_val.view(np.uint32), val.view(np.uint32))
    if keep.sum() < k:
        assert (got_i[:, keep.sum():] == -1).all() and np.isinf(got_s[:, keep.sum():]).all()
    if pattern == "all":
        u_s, u_i = mg.restate_metric(T, w, codes, k, metric)
        assert np.array_equal(u_s.view(np.uint32), got_s.view(np.uint32)) and np.array_equal(u_i, got_i)


@pytest.mark.parametrize("case", kg.CASES, ids=lambda c: c.name)
def test_gpu_case_reaches_what_it_claims(case):
    c = kg.constants()
    scan = sg.scan_plan(case.Q, case.B, case.N, case.K, case.k, c)
    sweep = rg.range_plan(case.Q, case.B, case.N, case.K, c)
    T, codes, t = kg.host_data(case)
    s = mg.restate_metric_scores(T, t, codes, "l2")
    best = s.argmin(axis=1)
    got = dict(skips=[False, False], dead_wave=[False, False], dead_slice=[False, False], short=False, best_cleared=False,
               tie_at_k=False)
    for pattern in kg.PATTERNS:
        keep, words = kg.words_for(pattern, case.B, 1, case.k)
        assert np.array_equal(kg.unpack(words, case.B), keep)
        n = int(keep.sum())
        assert {"all": n == case.B, "none": n == 0, "one_last": n == 1 and keep[-1], "one_first": n == 1 and keep[0],
                "few": n == min(case.k - 1, case.B), "run": n == max(1, case.B // 100)}.get(pattern, True), pattern
        if n == 0:
            continue
        for i, (plan, waves, strided) in enumerate(((scan, c["kScanWaves"], True), (sweep, c["kRangeWaves"], False))):
            skips, dead_wave, dead_slice = kg.reach(keep, plan, case.B, waves, strided)
            got["skips"][i] |= bool(skips)
            got["dead_wave"][i] |= bool(dead_wave)
            got["dead_slice"][i] |= bool(dead_slice)
        got["short"] |= n < case.k
        got["best_cleared"] |= bool((~keep[best]).any())
        if n >= case.k:
            top_s, _ = kg.restate_topk_masked(s, keep, case.k)
            cleared = s[:, ~keep]
            got["tie_at_k"] |= bool((cleared == top_s[:, case.k - 1:case.k]).any())
    for flag in ("skips", "dead_wave", "dead_slice"):
        assert all(got[flag]) == getattr(case, flag), (flag, got[flag])
    for flag in ("short", "best_cleared", "tie_at_k"):
        assert got[flag] == getattr(case, flag), (flag, got[flag])
    # the long run: a wave of the scan and a wave of the sweeps own more steps than one refill of the mask window reads
    window = c["kMaskWindow"]
    longest = (kg.longest_run(scan, case.B, c["kScanWaves"], True), kg.longest_run(sweep, case.B, c["kRangeWaves"], False))
    assert (min(longest) > window) == case.long_run, (longest, window)
    if case.long_run:
        keep = kg.keep_for("run", case.B, 1, case.k)              # ... and under `run` some wave finds a whole window empty
        assert kg.refills_on_empty(keep, scan, case.B, c["kScanWaves"], True, window)
        assert kg.refills_on_empty(keep, sweep, case.B, c["kRangeWaves"], False, window)


def test_case_table_covers_the_ground():
    cs = kg.CASES
    for flag in ("skips", "dead_wave", "dead_slice", "short", "best_cleared"):
        assert sum(bool(getattr(c, flag)) for c in cs) >= 2, flag
    assert any(c.tie_at_k and c.codes == "dup16" for c in cs) and sum(c.long_run for c in cs) == 1
    assert {(c.N, c.K, c.Q, c.B) for c in cs} >= {(1, 16, 1, 1), (2, 64, 17, 63), (8, 256, 17, 64), (16, 16, 17, 65),
                                                  (8, 256, 17, 4099), (8, 256, 200, 40_000), (64, 256, 17, 100_003),
                                                  (8, 256, 1, 100_003), (8, 64, 17, 4099), (64, 256, 258, 70_000)}
    assert any(c.packed and c.K == 16 for c in cs) and any(c.queries == "fp16" for c in cs)
    assert any(c.state == "decode_only" for c in cs) and any(c.k == 1 for c in cs)
    assert len(kg.PATTERNS) == 11 and all(c.restate or c.long_run for c in cs)


def test_python_argument_errors_precede_device_work():
    """on CPU tensors: a mask of the wrong length or dtype is a ValueError that names both lengths; a mask that is right but
    not on the device is the McqError of every other search input"""
    import torch
    m = _lib()
    from quantization_amd import Quantizer
    q = Quantizer(24, 16, 4)
    B = 130
    tables, codes, norms = torch.zeros(3, 4, 16), torch.zeros(B, 4, dtype=torch.uint8), torch.zeros(B)
    packed16 = torch.zeros(B, 2, dtype=torch.uint8)             # packed 16-entry codes: B still counts stored vectors
    x = torch.zeros(3, 24)
    thr = torch.zeros(3)
    for bad, both in ((torch.zeros(B - 1, dtype=torch.bool), ("129", "130")), (torch.zeros(2, dtype=torch.int64), ("2", "130", "3")),
                      (torch.zeros(4, dtype=torch.int64), ("4", "130", "3"))):
        for call in (lambda: q.search(x, codes, mask=bad), lambda: q.search(x, packed16, mask=bad),
                     lambda: q.search(x, codes, metric="ip", mask=bad), lambda: q.range_search(x, packed16, 1.0, mask=bad),
                     lambda: q._search_scan(tables, codes, norms, 10, mask=bad),
                     lambda: q._search_range(tables, codes, norms, thr, mask=bad)):
            with pytest.raises(ValueError) as e:
                call()
            assert all(n in str(e.value) for n in both), str(e.value)
    for bad in (torch.zeros(B), torch.zeros(B, dtype=torch.uint8), torch.zeros(B, 1, dtype=torch.bool), [True] * B):
        with pytest.raises(ValueError):
            q.search(x, codes, mask=bad)
        with pytest.raises(ValueError):
            q.range_search(x, codes, 1.0, mask=bad)
    for good in (torch.zeros(B, dtype=torch.bool), torch.zeros(3, dtype=torch.int64)):
        for call in (lambda: q.search(x, codes, mask=good), lambda: q.range_search(x, codes, 1.0, mask=good),
                     lambda: q._search_scan(tables, codes, norms, 10, mask=good),
                     lambda: q._search_range(tables, codes, norms, thr, mask=good)):
            with pytest.raises(m.McqError):
                call()
    with pytest.raises(ValueError):
        q.pack_mask(torch.zeros(B))
    with pytest.raises(ValueError):
        q.pack_mask(torch.zeros(B, 2, dtype=torch.bool))
    with pytest.raises(m.McqError):
        q.pack_mask(torch.zeros(B, dtype=torch.bool))
    with pytest.raises(m.McqError):
        q.pack_mask(torch.zeros(B, dtype=torch.uint8))
