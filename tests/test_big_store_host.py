"""tests/big_store.py on the CPU: the planted lists of the three stores hold every position they are meant to, the background
is separated from the planted rows for the committed seeds, and -- on a miniature store of 5,000 rows built by the same builder
and restated IN FULL -- the reference "compact store plus background tail" is the answer bit for bit, while a store whose
loads wrap at a crossing gives another one in every case."""
import numpy as np
import pytest

import big_store as bs
import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg
import search_range_lists_grid as rl

COUNTS = (256, 56)
LISTS = [(st, count, None) for st in bs.STORES for count in COUNTS] + [(bs.EDGE, 56, (100, 40)), (bs.MINI, 256, None),
                                                                       (bs.MINI, 56, None)]


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("st,count,last", LISTS, ids=lambda v: getattr(v, "name", str(v)))
def test_planted_lists(st, count, last):
    pos = bs.planted(st, count, last)
    B = st.B
    assert len(pos) == count and (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < B
    have = set(pos.tolist())
    # the ends of the store and of a step of 64
    assert {0, 1, 63, 64, B - 1, B - 2, (B - 1) // 64 * 64} <= have and ((B - 1) // 64 * 64 < B - 1 or B % 64 == 1)
    # both sides of every row at which the byte offset of the codes crosses 2^31 / 2^32
    for x in st.crossings:
        r = x // st.N
        if r < B:
            assert r * st.N <= x < (r + 1) * st.N
            assert {p for p in (r - 1, r, r + 1) if p < B} <= have, (st.name, x)
    if st is bs.BYTES:
        assert {2 ** 25 - 1, 2 ** 25, 2 ** 25 + 1, 2 ** 26 - 1, 2 ** 26, 2 ** 26 + 1} <= have
        assert (2 ** 25 - 1) * 64 < 2 ** 31 <= 2 ** 25 * 64 and (2 ** 26 - 1) * 64 < 2 ** 32 <= 2 ** 26 * 64
    if st in (bs.ROWS, bs.EDGE):
        assert not bs.crossing_rows(st)                               # fewer than 2^31 bytes of codes
    if st is bs.EDGE:
        assert {2 ** 31 - 2, 2 ** 31 - 3} <= have and pos[-1] == sg.constants()["kNoIndex"] - 1
    # the first and last row of the first, a middle and the last slice of the scan's plan
    plan = sg.scan_plan(bs.Q, B, st.N, st.K, 64)
    mid = plan.slices // 2
    for s in (0, mid, plan.slices - 1):
        assert {s * plan.per_slice, min(B, (s + 1) * plan.per_slice) - 1} <= have, (st.name, s)
    if st is not bs.MINI:
        assert plan.slices == sg.constants()["kScanMaxSlices"] and 0 < mid < plan.slices - 1 and plan.last_step_partial(B)
    if last:
        assert int((pos >= B - last[0]).sum()) == last[1]
    # no planted row at an alias of a planted row, except between the required rows themselves
    req = set(bs.required(st).tolist())
    assert req <= have
    for p, p2 in bs.alias_pairs(st, pos):
        assert p in req and p2 in req, (st.name, p, p2)
    if st in (bs.ROWS, bs.EDGE):
        assert not bs.alias_pairs(st, pos)
    # ... and there a wrapped load is noticed because the two rows score differently, for every query and metric
    T = bs.tables(st)
    at = {int(p): j for j, p in enumerate(pos)}
    for m in bs.METRICS:
        s = bs.compact_scores(st, T, count, m)
        for p, p2 in bs.alias_pairs(st, pos):
            assert (s[:, at[p]] != s[:, at[p2]]).all(), (st.name, m, p, p2)


@pytest.mark.parametrize("st,count,last", LISTS, ids=lambda v: getattr(v, "name", str(v)))
def test_background_is_separated(st, count, last):
    for queries in (bs.Q, 40):
        T = bs.tables(st, queries)
        assert (T[:, :, 0] == bs.BACKGROUND).all() and np.abs(T[:, :, 1:]).max() <= 1
        assert bs.separated(st, T, count)
    d = bs.digits(st, count)
    assert d.min() >= 1 and d.max() <= st.K - 1 and d.shape == (count, st.N)
    # the background's score is exact: rule 3's chain over N entries of 1000, then + 0 or * 1
    zeros = np.zeros((2, st.N), dtype=np.uint8)
    T = bs.tables(st)
    for m in bs.METRICS:
        w = None if m == "ip" else np.full(2, bs.background_w(m), dtype=np.float32)
        assert (_u32(mg.restate_metric_scores(T, w, zeros, m)) == _u32(st.bg())).all()
        w_p = bs.planted_w(st, count, m)
        assert w_p is None or (w_p > 0).all() if m == "cosine" else w_p is None or ((w_p >= 0) & (w_p < 1)).all()
        thr = bs.thresholds(st, T, count, m)
        assert np.isneginf(thr[2]) and np.isfinite(thr[:2]).all()


# ------------------------------------------------------------------ the miniature, restated in full
def _mini(count, metric):
    st = bs.MINI
    pos = bs.planted(st, count)
    codes, w = bs.build(st, pos, metric)
    return st, pos, bs.tables(st), codes, w


@pytest.mark.parametrize("metric", bs.METRICS)
@pytest.mark.parametrize("count,k", ((256, 64), (56, 64), (256, 300)))
def test_reference_is_the_full_restatement(count, k, metric):
    st, pos, T, codes, w = _mini(count, metric)
    assert codes.shape == (st.B, st.N) and int((codes != 0).any(1).sum()) == count and (codes[pos] == bs.digits(st, count)).all()
    want_s, want_i = mg.restate_metric(T, w, codes, k, metric)
    got_s, got_i = bs.reference_topk(st, T, pos, k, metric)
    assert np.array_equal(got_i, want_i) and np.array_equal(_u32(got_s), _u32(want_s))
    if count < k:
        assert (_u32(got_s[:, count:]) == _u32(st.bg())).all() and (np.diff(got_i[:, count:]) > 0).all()
    # under a mask that clears every third planted row, and one that keeps the last 100 rows only
    for kept, keep_from in ((np.arange(count) % 3 != 0, 0), (pos >= st.B - 100, st.B - 100)):
        keep = np.zeros(st.B, dtype=bool)
        keep[keep_from:] = True
        keep[pos] = kept
        s = mg.restate_metric_scores(T, w, codes, metric)
        want_s, want_i = kg.restate_topk_masked(s, keep, k)
        got_s, got_i = bs.reference_topk(st, T, pos, k, metric, kept=kept, keep_from=keep_from)
        assert np.array_equal(got_i, want_i) and np.array_equal(_u32(got_s), _u32(want_s))
    # the range search: the background is never listed
    thr = bs.thresholds(st, T, count, metric)
    _, lims, p, v = rg.restate(T, w, codes, metric, thr=thr)
    g_lims, g_p, g_v = bs.reference_range(st, T, pos, metric, thr)
    assert np.array_equal(lims, g_lims) and np.array_equal(p, g_p) and np.array_equal(_u32(v), _u32(g_v)) and lims[-1] > 10
    # list by list, without and with a bias per slot
    off, probes = bs.list_layout(st)
    s = mg.restate_metric_scores(T, w, codes, metric)
    want_s, want_i = lg.restate_lists(s, off, probes, k)
    got_s, got_i = bs.reference_lists(st, T, pos, off, probes, k, metric)
    assert np.array_equal(got_i, want_i) and np.array_equal(_u32(got_s), _u32(want_s))
    assert (got_i[2] == -1).all() and (got_i[1, :64] >= 0).all() and _u32(got_s[1][got_i[1] >= 0][-1]) == _u32(st.bg())
    import search_bias_grid as bg
    bias = bias_of(probes)
    sb = bg.biased_scores(mg.restate_sums(T, codes), off, probes, bias, w, metric)
    want_s, want_i = lg.restate_lists(sb, off, probes, k)
    got_s, got_i = bs.reference_lists(st, T, pos, off, probes, k, metric, bias=bias)
    assert np.array_equal(got_i, want_i) and np.array_equal(_u32(got_s), _u32(want_s))
    w_lims, w_p, w_v = rl.restate_range_lists(s, off, probes, thr)
    g_lims, g_p, g_v = bs.reference_range_lists(st, T, pos, off, probes, metric, thr)
    assert np.array_equal(w_lims, g_lims) and np.array_equal(w_p, g_p) and np.array_equal(_u32(w_v), _u32(g_v))


def bias_of(probes):
    """a bias per (query, slot) in [-2, 2]: far below the gap between the planted rows and the background"""
    return np.random.RandomState(5).uniform(-2.0, 2.0, size=probes.shape).astype(np.float32)


@pytest.mark.parametrize("metric", bs.METRICS)
@pytest.mark.parametrize("count,k", ((256, 64), (56, 64)))
@pytest.mark.parametrize("wrap_row", (1250, 2500))
def test_a_store_whose_loads_wrap_gives_another_answer(wrap_row, count, k, metric):
    st, pos, T, codes, w = _mini(count, metric)
    assert wrap_row * st.N in st.crossings
    bad = bs.wrapped(st, codes, wrap_row)
    assert np.array_equal(bad[:wrap_row], codes[:wrap_row]) and np.array_equal(bad[wrap_row:2 * wrap_row], codes[:wrap_row])
    got_s, got_i = bs.reference_topk(st, T, pos, k, metric)
    bad_s, bad_i = mg.restate_metric(T, w, bad, k, metric)
    assert not (np.array_equal(got_i, bad_i) and np.array_equal(_u32(got_s), _u32(bad_s)))
    assert all(not np.array_equal(got_i[q], bad_i[q]) or not np.array_equal(_u32(got_s[q]), _u32(bad_s[q])) for q in range(bs.Q))
    thr = bs.thresholds(st, T, count, metric)
    _, lims, p, v = rg.restate(T, w, bad, metric, thr=thr)
    g_lims, g_p, g_v = bs.reference_range(st, T, pos, metric, thr)
    assert not (np.array_equal(lims, g_lims) and np.array_equal(p, g_p) and np.array_equal(_u32(v), _u32(g_v)))


def test_a_piece_of_a_launch_stays_below_2_32_threads():
    """the kernels that spend a wave or more on a row are launched over at most kPieceRows rows (fewer by the factor where a
    row takes more than 64 threads: launch_in_pieces of mcq_api.hip): a piece is 2^31 threads, below the 2^32 at which the
    runtime starts to drop threads; the `rows` store of the device tests needs more than one piece, and a store of 2^25 rows
    still takes one launch"""
    c = sg.constants()
    piece = c["kPieceRows"]
    assert piece * 64 < 2 ** 32 and piece % (64 * c["kNormWaves"]) == 0 and piece >= 2 ** 25
    for threads in (64, 128, 256, 512):                                  # 8 slices x 4 .. 64 lanes of k_decode_sliced
        rows = piece * 64 // max(threads, 64)
        assert rows * threads < 2 ** 32 and rows % 64 == 0
    assert bs.ROWS.B > piece and bs.ROWS.B * 64 >= 2 ** 32 and -(-bs.ROWS.B // piece) == 3
    with open(sg.ROOT + "/quantization_amd/csrc/mcq_api.hip") as f:
        src = f.read()
    assert "(long)kPieceRows * 64 / (threads_per_row > 64 ? threads_per_row : 64)" in src
    assert src.count("launch_in_pieces(") == 5                          # its definition, the norms and three decode launchers


def test_pack_reference_of_the_device_test():
    """the words the device test forms with torch (view as (words, 64), times powers of two, summed in int64, the ragged last
    word apart) are search_mask_grid.pack, in numpy here"""
    for B in (1, 63, 64, 65, 4096 + 321):
        keep = (np.arange(B) % 3 != 0) | (np.arange(B) % 517 == 0)
        full = B // 64
        pw = (np.uint64(1) << np.arange(64, dtype=np.uint64)).view(np.int64)
        words = (keep[:full * 64].reshape(full, 64).astype(np.int64) * pw[None, :]).sum(1)
        if B % 64:
            words = np.concatenate([words, [(keep[full * 64:].astype(np.int64) * pw[:B % 64]).sum()]])
        assert np.array_equal(words.astype(np.int64), kg.pack(keep))
