"""The top-k search past 64 neighbours on the GPU (mcq_search_wide and mcq_search_wide_lists through
Quantizer._search_wide_scan, which ALWAYS runs the wide kernels; Quantizer.search_wide / search_lists_wide; include/mcq_wide.h
rules 24-27), BIT FOR BIT -- scores as int32 views, and positions -- against the numpy restatements.  No tolerance appears
before the last test, whose bound is that of tests/test_gpu_search_residual.py.

  whole store   the cases of tests/search_wide_grid.py (k on both sides of the old cap and of both sizes of the list; B = 0,
                k - 1, k, k + 1, 63, 64, 4,099, 100,003; Q = 1, 17, 200 and one Q whose plan has a single part; 1 x 16 to
                64 x 256 tables) x three metrics x no mask and four patterns of tests/search_mask_grid.py
  orders        hand-made per-candidate arrays over 20,000 candidates at k = 1,024 and 100: descending (every candidate enters,
                the flush runs throughout), ascending, all equal, -0.0 and +0.0 mixed, +inf, NaN, NaN leaving fewer than k;
                dup16 codes (mass ties by position)
  old, new      at k = 1, 10, 64 the wide kernels return the bits of the older entries: scan, masked, lists, bias
  prefix        the k = 100 result is the first 100 columns of the k = 1,024 result
  lists         the `single` and `mixed` layouts of tests/search_lists_grid.py (padding, a row of padding only), masks, a bias;
                every list probed against the call over the whole store; P = 4,096 with 64 x 256 tables at k = 1,024 once
  selection     every cell of launch_wide once, over the whole store and list by list
  public calls  shapes, leading dimensions, packed codes, fp16 queries, the errors; search(k = 65) still raises
  end to end    the residual recipe of tests/test_gpu_search_residual.py at k = 300, within that test's derived bound"""
import dataclasses

import numpy as np
import pytest
import torch

import search_bias_grid as bg
import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_selection_grid as sel
import search_wide_grid as wg
import test_gpu_search as base
import test_gpu_search_lists as tl

pytestmark = pytest.mark.gpu

SEED = wg.SEED
_WHOLE = {}


def _i32(t):
    return t.view(torch.int32)


def _same(got, want, what):
    (gs, gi), (want_s, want_i) = got, want
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gs.shape == gi.shape == want_i.shape, what
    assert np.array_equal(gi, want_i), f"{what}: positions differ from rule 26 in rows {np.flatnonzero((gi != want_i).any(1))[:8]}"
    assert np.array_equal(gs.view(np.uint32), want_s.view(np.uint32)), f"{what}: scores differ from rule 25"
    tail = want_i == -1
    assert (gi[tail] == -1).all() and np.isposinf(gs[tail]).all(), f"{what}: the tail is not (+inf, -1)"
    return int(tail.sum())


def _equal(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(_i32(a[0]), _i32(b[0]))


def _whole(x):
    """the quantizer, the store, the tables and the per-candidate arrays of a whole-store case, on the device and in numpy; the
    restated scores per metric are added as they are first needed"""
    if _WHOLE.get("name") != x.name:
        _WHOLE.clear()
        case = dataclasses.replace(x.case(), B=max(x.B, 1))                # (an empty store is a slice of a store of one)
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, _ = base._queries(case, q, kept)
        tables = q.search_tables(xq).contiguous()
        norms = q.code_norms(kept)
        rnorms = q.rnorms_from_norms(norms)
        flat, norms, rnorms = flat[:x.B], norms[:x.B].contiguous(), rnorms[:x.B].contiguous()
        _WHOLE.update(name=x.name, scores={},
                      v=(q, flat, torch.from_numpy(flat).cuda(), tables, tables.cpu().numpy(),
                         {"l2": norms, "ip": None, "cosine": rnorms},
                         {"l2": norms.cpu().numpy(), "ip": None, "cosine": rnorms.cpu().numpy()}))
    return _WHOLE["v"]


def _scores(x, metric):
    q, flat, flat_d, tables, T, w_d, w_h = _whole(x)
    if metric not in _WHOLE["scores"]:
        _WHOLE["scores"][metric] = mg.restate_metric_scores(T, w_h[metric], flat, metric)
    return _WHOLE["scores"][metric]


# ------------------------------------------------------------------ the whole store
@pytest.mark.parametrize("metric", wg.METRICS)
@pytest.mark.parametrize("x", wg.CASES, ids=lambda c: c.name)
def test_whole_store_case(x, metric):
    q, flat, flat_d, tables, T, w_d, w_h = _whole(x)
    s = _scores(x, metric)
    for pattern in wg.MASKS if x.B > 0 else (None,):
        keep = None if pattern is None else kg.keep_for(pattern, x.B, SEED, x.k)
        keep_d = None if keep is None else torch.from_numpy(keep).cuda()
        got = q._search_wide_scan(tables, flat_d, w_d[metric], x.k, metric=metric, mask=keep_d)
        tail = _same(got, wg.restate_topk_valid(s, x.k, keep), f"{x.name} {metric} {pattern}")
        n = x.B if keep is None else int(keep.sum())
        assert tail == x.Q * max(x.k - n, 0)
    again = q._search_wide_scan(tables, flat_d, w_d[metric], x.k, metric=metric)
    assert _equal(again, q._search_wide_scan(tables, flat_d, w_d[metric], x.k, metric=metric)), "a second call differs"


@pytest.mark.parametrize("metric", wg.METRICS)
def test_prefix_property(metric):
    x = next(c for c in wg.CASES if c.name == "n8_k256_b4099_k1024")
    q, flat, flat_d, tables, T, w_d, w_h = _whole(x)
    keep_d = torch.from_numpy(kg.keep_for("half", x.B, SEED, x.k)).cuda()
    for mask in (None, keep_d):
        full = q._search_wide_scan(tables, flat_d, w_d[metric], 1024, metric=metric, mask=mask)
        for k in (100, 513):
            part = q._search_wide_scan(tables, flat_d, w_d[metric], k, metric=metric, mask=mask)
            assert torch.equal(part[1], full[1][:, :k]) and torch.equal(_i32(part[0]), _i32(full[0][:, :k])), (metric, k)


# ------------------------------------------------------------------ hand-made orders
def _order_quantizer():
    return base._quantizer(sg.Case("wide_orders", wg.ORDER_N, wg.ORDER_K, 24, wg.ORDER_Q, wg.ORDER_B, 1, state="decode_only"))


@pytest.mark.parametrize("k", wg.ORDER_KS)
@pytest.mark.parametrize("order", wg.ORDERS)
def test_hand_made_order(order, k):
    q = _order_quantizer()
    Q, B = wg.ORDER_Q, wg.ORDER_B
    T = np.full((Q, wg.ORDER_N, wg.ORDER_K), -0.0, dtype=np.float32)        # a zero query: every table entry is -0.0
    codes = np.random.RandomState(9).randint(0, wg.ORDER_K, size=(B, wg.ORDER_N)).astype(np.uint8)
    w = wg.order_w(order)
    metric = "ip" if order == "all_equal" else "l2"                        # the inner product of a zero query: a store of -0.0
    s = mg.restate_metric_scores(T[:1], w, codes, metric)
    if metric == "l2":
        assert np.array_equal(s[0].view(np.uint32), w.view(np.uint32))      # the score IS w[b], bit for bit
    else:
        assert (s == 0).all() and np.signbit(s).all()
    want_s, want_i = wg.restate_topk_valid(s, k)
    got = q._search_wide_scan(torch.from_numpy(T).cuda(), torch.from_numpy(codes).cuda(),
                              None if metric == "ip" else torch.from_numpy(w).cuda(), k, metric=metric)
    tail = _same(got, (np.repeat(want_s, Q, axis=0), np.repeat(want_i, Q, axis=0)), f"{order} k={k}")
    valid = int((~np.isnan(s[0])).sum())
    assert tail == Q * max(k - valid, 0) and (order != "nan_short" or (tail > 0) == (k == 1024))
    if order in ("all_equal", "zeros", "ascending"):
        assert want_i[0].tolist() == list(range(k))
    if order == "descending":
        assert want_i[0].tolist() == list(range(B - 1, B - 1 - k, -1))
    if order == "zeros":
        assert len(set(np.signbit(want_s[0]).tolist())) == 2                # both zeros leave with their own bits
    if order == "inf":
        assert np.isneginf(want_s[0][0]) and (np.isposinf(want_s[0][-1]) == (k == 1024)) and (want_i[0] >= 0).all()


@pytest.mark.parametrize("k", wg.ORDER_KS)
def test_dup16_codes_tie_by_position(k):
    case = wg.dup16_case()
    q = base._quantizer(case)
    kept, flat = base._store(case, q)
    xq, _ = base._queries(case, q, kept)
    tables, norms = q.search_tables(xq).contiguous(), q.code_norms(kept)
    s = mg.restate_metric_scores(tables.cpu().numpy(), norms.cpu().numpy(), flat, "l2")
    want = wg.restate_topk_valid(s, k)
    assert len(np.unique(want[0][0])) <= 16 < k                            # mass ties: at most 16 distinct scores
    _same(q._search_wide_scan(tables, kept, norms, k), want, f"dup16 k={k}")


# ------------------------------------------------------------------ the older entries
@pytest.mark.parametrize("case", (lg.CASES[1], lg.CASES[2]), ids=lambda c: c.name)
def test_old_against_new(case):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tl._prepared(case)
    tables, flat_d = tables.contiguous(), flat_d.contiguous()
    keep_d = torch.from_numpy(kg.keep_for("half", case.B, SEED, 10)).cuda()
    S = mg.restate_sums(tables.cpu().numpy(), flat)
    bias_d = torch.from_numpy(bg.bias_for(S, off, probes, SEED)).cuda()
    for metric in wg.METRICS:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        for k in (1, 10, 64):
            for kw in (dict(), dict(mask=keep_d), dict(lists=(off_d, probes_d)), dict(lists=(off_d, probes_d), mask=keep_d),
                       dict(lists=(off_d, probes_d), bias=bias_d), dict(lists=(off_d, probes_d), bias=bias_d, mask=keep_d)):
                new, old = q._search_wide_scan(tables, flat_d, w, k, metric=metric, **kw), q._search_scan(tables, flat_d, w, k, metric=metric, **kw)
                assert _equal(new, old), (case.name, metric, k, sorted(kw))


# ------------------------------------------------------------------ the lists
@pytest.mark.parametrize("metric", wg.METRICS)
@pytest.mark.parametrize("k", wg.LISTS_KS)
@pytest.mark.parametrize("case", (lg.CASES[0], lg.CASES[1]), ids=lambda c: c.name)
def test_lists_case(case, k, metric):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tl._prepared(case)
    w, s = tl._per_metric(case, metric)
    tables, flat_d = tables.contiguous(), flat_d.contiguous()
    S = mg.restate_sums(tables.cpu().numpy(), flat)
    bias = bg.bias_for(S, off, probes, SEED)
    bias_d = torch.from_numpy(bias).cuda()
    sb = bg.biased_scores(S, off, probes, bias, None if w is None else w.cpu().numpy(), metric)
    two = bg.rows_with_two_lists(off, probes)
    for pattern in lg.PATTERNS:
        keep = None if pattern is None else kg.keep_for(pattern, case.B, SEED, k)
        keep_d = None if keep is None else torch.from_numpy(keep).cuda()
        plain = q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d))
        _same(plain, lg.restate_lists(s, off, probes, k, keep), f"{case.name} k={k} {metric} {pattern}")
        biased = q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d), bias=bias_d)
        _same(biased, lg.restate_lists(sb, off, probes, k, keep), f"{case.name} k={k} {metric} {pattern} bias")
        if two and pattern is None:
            rows = torch.tensor(two, device="cuda")
            assert not (torch.equal(biased[1][rows], plain[1][rows]) and torch.equal(_i32(biased[0][rows]), _i32(plain[0][rows])))
    if case.lists == "mixed":                                # a row of padding only: the fill
        got = q._search_wide_scan(tables, flat_d, w, k, metric=metric, lists=(off_d, probes_d))
        assert (probes[0] == -1).all() and bool((got[1][0] == -1).all()) and bool(torch.isposinf(got[0][0]).all())


@pytest.mark.parametrize("metric", wg.METRICS)
def test_every_list_probed_is_the_whole_store(metric):
    case = lg.CASES[2]
    assert case.covering
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tl._prepared(case)
    w, s = tl._per_metric(case, metric)
    tables, flat_d = tables.contiguous(), flat_d.contiguous()
    every = torch.from_numpy(lg.all_probes(case, len(off) - 1)).cuda()
    for k in wg.LISTS_KS:
        for keep in (None, kg.keep_for("half", case.B, SEED, k)):
            keep_d = None if keep is None else torch.from_numpy(keep).cuda()
            a = q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, every))
            b = q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=keep_d)
            assert _equal(a, b), (metric, k, keep is not None)
            _same(b, wg.restate_topk_valid(s, k, keep), f"{case.name} whole k={k} {metric}")


def test_largest_lds_cell_4096_probes_of_64x256_tables_at_k_1024():
    case = wg.BIG
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tl._prepared(case)
    assert tuple(probes.shape) == (1, 4096) and (case.N, case.K, case.k) == (64, 256, 1024)
    w, s = tl._per_metric(case, "l2")
    got = q._search_wide_scan(tables.contiguous(), flat_d.contiguous(), w, case.k, lists=(off_d, probes_d))
    assert _same(got, lg.restate_lists(s, off, probes, case.k), case.name) == 0


# ------------------------------------------------------------------ every cell of launch_wide
@pytest.mark.parametrize("N", sel.NS)
def test_every_cell_of_launch_wide(N):
    case = sel.lists_case(N)
    q = base._quantizer(case)
    kept, flat = base._store(case, q)
    xq, _ = base._queries(case, q, kept)
    tables, norms = q.search_tables(xq).contiguous(), q.code_norms(kept)
    rnorms = q.rnorms_from_norms(norms)
    T, flat_d, k = tables.cpu().numpy(), torch.from_numpy(flat).cuda(), 100
    off, probes = sel.lists_layout()
    off_d, probes_d = torch.from_numpy(off).cuda(), torch.from_numpy(probes).cuda()
    keep, words = sel.mask_for(case.B)
    words_d = torch.from_numpy(words).cuda()
    S = mg.restate_sums(T, flat)
    bias = bg.bias_for(S, off, probes, SEED)
    for metric in wg.METRICS:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        wh = None if w is None else w.cpu().numpy()
        s = mg.restate_metric_scores(T, wh, flat, metric)
        sb = bg.biased_scores(S, off, probes, bias, wh, metric)
        for masked in (False, True):
            what = f"wide {N} x {case.K} {metric}{' masked' if masked else ''}"
            m, kp = (words_d, keep) if masked else (None, None)
            _same(q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=m), wg.restate_topk_valid(s, k, kp), what)
            _same(q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=m, lists=(off_d, probes_d)),
                  lg.restate_lists(s, off, probes, k, kp), what + " lists")
            _same(q._search_wide_scan(tables, flat_d, w, k, metric=metric, mask=m, lists=(off_d, probes_d), bias=torch.from_numpy(bias).cuda()),
                  lg.restate_lists(sb, off, probes, k, kp), what + " bias")


# ------------------------------------------------------------------ the public calls
def _public(name):
    case = next(c for c in sg.CASES if c.name == name)
    q = base._quantizer(case)
    kept, flat = base._store(case, q)
    xq, _ = base._queries(case, q, kept)
    return case, q, kept, xq


@pytest.mark.parametrize("name", ("fp16_queries", "n16_k16_packed_b65", "stored_queries_clamp"))
def test_public_calls(name):
    from quantization_amd._lib import McqError
    case, q, kept, xq = _public(name)
    Q, B, D = case.Q, case.B, case.D
    norms = q.code_norms(kept)
    off = torch.tensor([0, B // 3, B // 3, B], dtype=torch.int64, device="cuda")
    probes = torch.tensor([[2, 0, -1]] * Q, dtype=torch.int32, device="cuda")
    for metric in wg.METRICS:
        val, idx = q.search_wide(xq, kept, 200, metric=metric)
        assert val.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(val.shape) == tuple(idx.shape) == (Q, 200)
        lead = q.search_wide(xq.reshape(1, Q, D), kept, 200, norms=norms, metric=metric)
        assert tuple(lead[0].shape) == tuple(lead[1].shape) == (1, Q, 200) and _equal((lead[0][0], lead[1][0]), (val, idx))
        old = q.search(xq, kept, k=64, metric=metric)
        assert _equal((val[:, :64].contiguous(), idx[:, :64].contiguous()), old), "the first 64 columns are search(k=64)"
        assert _equal(q.search_wide(xq, kept, 64, metric=metric), old)
        if B < 200:                                          # a short store: the tail of search()
            fill = float("inf") if metric == "l2" else float("-inf")
            assert bool((idx[:, B:] == -1).all()) and bool((val[:, B:] == fill).all()) and bool((idx[:, :B] >= 0).all())
        lv, li = q.search_lists_wide(xq, kept, off, probes, 200, metric=metric)
        assert tuple(lv.shape) == tuple(li.shape) == (Q, 200)
        assert _equal((lv[:, :64].contiguous(), li[:, :64].contiguous()), q.search_lists(xq, kept, off, probes, k=64, metric=metric))
        every = q.search_lists_wide(xq, kept, off, torch.tensor([[1, 2, 0]] * Q, device="cuda"), 200, norms=norms, metric=metric)
        assert _equal(every, (val, idx)), "every list probed is the whole store"
    for call in (lambda k: q.search_wide(xq, kept, k), lambda k: q.search_lists_wide(xq, kept, off, probes, k)):
        with pytest.raises(McqError):
            call(1025)
        with pytest.raises(McqError):
            call(0)
        assert tuple(call(1024)[0].shape) == (Q, 1024)
    with pytest.raises(McqError):
        q.search_wide(xq.cpu(), kept, 200)
    with pytest.raises(McqError):
        q.search_wide(xq, kept.cpu(), 200)
    with pytest.raises(McqError):
        q.search(xq, kept, k=65)                             # the older calls keep their cap
    with pytest.raises(McqError):
        q.search_lists(xq, kept, off, probes, k=65)


# ------------------------------------------------------------------ end to end
@pytest.mark.parametrize("metric", wg.METRICS)
def test_residual_recipe_at_k_300(metric):
    import test_gpu_search_residual as res
    q, xq_d, codes, off, probes, bias, norms, rnorms, exact, bound, cand = res._setup()
    k = 300
    val, idx = q.search_lists_wide(xq_d, codes, off, probes, k, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias)
    assert tuple(val.shape) == tuple(idx.shape) == (res.Q, k)
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    ex, bd = exact[metric], bound[metric]
    sign = 1.0 if metric == "l2" else -1.0
    worst = 0.0
    for j in range(res.Q):
        c = cand[j]
        m = min(k, len(c))
        got = idx[j, :m]
        assert (idx[j, m:] == -1).all() and np.isin(got, c).all() and len(set(got.tolist())) == m
        err = np.abs(val[j, :m] - ex[j, got])
        assert (err <= bd[j, got]).all(), (j, err.max(), bd[j, got].min())
        worst = max(worst, float((err / bd[j, got]).max()))
        # the index set of the float64 ranking, except where two float64 values lie closer than the bound
        by = c[np.argsort(sign * ex[j, c], kind="stable")]
        want = by[:m]
        E = float(bd[j, c].max())
        edge = ex[j, by[m - 1]]
        for b in np.setxor1d(got, want):
            assert abs(ex[j, b] - edge) <= 2 * E, (j, int(b), abs(ex[j, b] - edge), E)
    print(f"[wide residual] {metric}: largest error / bound {worst:.4f}")
