"""The search over stores of two-byte codes on the GPU (include/mcq_code16.h rules 32-35: mcq_search_tables_u16,
mcq_code_norms_u16, mcq_search_topk_u16, mcq_search_range_u16_count / _fill; Quantizer.pack_codes and every search method with
codebook_size 512 or 1,024), BIT FOR BIT -- scores as int32 views, and positions -- against the numpy restatements the one-byte
entries are held to: they index tables with `digit & (K - 1)` and are generic in K and in the element type.  No tolerance
appears before the last test, whose bounds are the project's derived fp32 bounds.

  digit stream  the cases of tests/search_code16_grid.py: the four chunk widths, one, two and four chunks per row, stores of 0 to
                4,099 vectors, k on both sides of 64 up to 1,024; tables, norms, reciprocal roots and the top-k under three
                metrics, without a mask and with one
  masks         four patterns of tests/search_mask_grid.py at 8 x 1,024
  lists         the `mixed` layout of tests/search_lists_grid.py (empty lists, padding, a row of padding only), with a bias and
                without, masks; every list of a covering layout probed against the call over the whole store
  range         count + fill as CSR: the whole store (probes == NULL) and list by list with a list named twice, a bias, a mask;
                thresholds that list nothing, about ten, a hundredth, everything
  orders        hand-made per-candidate arrays over 20,000 candidates at 8 x 1,024, k = 1,024
  high bits     a store OR-ed with 0xFC00 (K = 1,024) or 0xFE00 (K = 512) gives the bits of the clean store's results (rule 32)
  cross-check   at K <= 256 the new entries on codes.to(int16) against the shipped one-byte entries on the uint8 store
  routing       a quantizer of 256 entries names the entries it named, one of 1,024 the new ones
  end to end    the reference's fixtures k1024_d40_n8 and k512_d16_n16: encode, pack_codes, search and range_search within the
                derived bounds of the float64 values of decode; decode of the int16 store"""
import numpy as np
import pytest
import torch

import search_bias_grid as bg
import search_code16_grid as cg
import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg
import search_range_lists_grid as rl
import search_tables_grid as tg
import search_wide_grid as wg
import test_gpu_search as base
from golden import fixtures

pytestmark = pytest.mark.gpu
SEED = cg.SEED
_CACHE = {}


def _i32(t):
    return t.view(torch.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _padded_centers(q):
    """the fp32 rows of `prepared` that the tables and the norms read, (N, K, Dp)"""
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    Dp = sg.padded(D)
    blob = q._prepared(any_flavour=True)
    torch.cuda.synchronize()
    return blob[:N * K * Dp * 4].view(torch.float32).reshape(N, K, Dp).cpu().numpy()


def _setup(x):
    """the quantizer, the digits, the int16 store, the queries and what the device made of them, once per case"""
    if _CACHE.get("name") != x.name:
        _CACHE.clear()
        from quantization_amd import synthetic as gen
        q = base._quantizer(x.case())
        d = cg.digits(x.N, x.K, x.B)
        store = q.pack_codes(_dev(d))
        assert store.dtype == (torch.int16 if x.K > 256 else torch.uint8) and tuple(store.shape) == (x.B, x.N)
        xq = _dev(gen.make_gaussian(77 + x.Q, x.Q, x.D))
        if x.K > 256:
            tables, norms, rnorms = q.search_tables(xq), q.code_norms(store), q.code_rnorms(store)
        else:
            tables = norms = rnorms = None
        _CACHE.update(name=x.name, v=(q, d, store, xq, tables, norms, rnorms))
    return _CACHE["v"]


def _w(metric, norms, rnorms):
    return None if metric == "ip" else (norms if metric == "l2" else rnorms)


def _same_topk(got, want, what):
    (gs, gi), (want_s, want_i) = got, want
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gs.shape == gi.shape == want_i.shape, what
    assert np.array_equal(gi, want_i), f"{what}: positions differ in rows {np.flatnonzero((gi != want_i).any(1))[:8]}"
    assert np.array_equal(_bits(gs), _bits(want_s)), f"{what}: scores differ"


def _same_range(got, want, what):
    (lims, s, i), (want_lims, want_i, want_s) = got, want
    assert np.array_equal(lims.cpu().numpy(), want_lims), f"{what}: lims differ"
    assert np.array_equal(i.cpu().numpy(), want_i), f"{what}: positions differ"
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(want_s)), f"{what}: scores differ"


def _equal(a, b):
    return all(torch.equal(x, y) if x.dtype != torch.float32 else torch.equal(_i32(x), _i32(y)) for x, y in zip(a, b))


# ------------------------------------------------------------------ the digit stream
@pytest.mark.parametrize("x", cg.CASES, ids=lambda c: c.name)
def test_digit_stream(x):
    q, d, store, xq, tables, norms, rnorms = _setup(x)
    Cp = _padded_centers(q)
    T = tables.cpu().numpy()
    assert tuple(T.shape) == (x.Q, x.N, x.K)
    assert np.array_equal(_bits(T.reshape(x.Q, -1)), _bits(tg.restate_tables(xq.cpu().numpy(), Cp))), "tables: rule 1"
    t, r = norms.cpu().numpy(), rnorms.cpu().numpy()
    assert t.shape == r.shape == (x.B,)
    if x.B:
        assert np.array_equal(_bits(t), _bits(tg.restate_norms(Cp, d))), "norms: rule 2"
        assert np.array_equal(_bits(r), _bits(mg.restate_rnorms(t))), "reciprocal roots: rule 6"
        assert torch.equal(_i32(q.rnorms_from_norms(norms)), _i32(rnorms))
    for metric in cg.METRICS:
        w = _w(metric, norms, rnorms)
        s = mg.restate_metric_scores(T, None if w is None else w.cpu().numpy(), d, metric) if x.B else np.zeros((x.Q, 0), np.float32)
        for pattern in cg.MASKS if x.B else (None,):
            keep = None if pattern is None else kg.keep_for(pattern, x.B, SEED, x.k)
            scan = q._search_scan if x.k <= 64 else q._search_wide_scan
            got = scan(tables, store, w, x.k, metric=metric, mask=None if keep is None else _dev(keep))
            _same_topk(got, wg.restate_topk_valid(s, x.k, keep), f"{x.name} {metric} {pattern}")
    # the public calls: shapes, values in the reported domain, int64 digits narrowed per call
    dist, idx = q.search(xq, store, k=x.k)
    assert tuple(dist.shape) == tuple(idx.shape) == (x.Q, x.k)
    assert _equal((dist, idx), q.search_wide(xq, _dev(d), x.k)), "int64 digits and the int16 store differ"
    assert int((idx >= 0).sum()) == x.Q * min(x.k, x.B)


@pytest.mark.parametrize("metric", cg.METRICS)
def test_masks(metric):
    x = cg.MASK_CASE
    q, d, store, xq, tables, norms, rnorms = _setup(x)
    w = _w(metric, norms, rnorms)
    s = mg.restate_metric_scores(tables.cpu().numpy(), None if w is None else w.cpu().numpy(), d, metric)
    for pattern in cg.MASK_PATTERNS:
        keep, words = kg.words_for(pattern, x.B, SEED, x.k)
        for k in (10, x.k):
            want = wg.restate_topk_valid(s, k, keep)
            _same_topk(q._search_scan(tables, store, w, k, metric=metric, mask=_dev(keep)), want, f"{metric} {pattern} k={k}")
            _same_topk(q._search_scan(tables, store, w, k, metric=metric, mask=_dev(words)), want, f"{metric} {pattern} k={k} packed")
        thr = rg.thresholds_for(s[:, keep] if keep.any() else s)
        _same_range(q._search_range(tables, store, w, _dev(thr), metric=metric, mask=_dev(keep)),
                    kg.restate_range_masked(s, keep, thr), f"range {metric} {pattern}")


# ------------------------------------------------------------------ the lists
LISTS = lg.Case("code16_n8_k1024_mixed_p7", 8, 1024, 24, 17, 6000, 10, 7, "mixed", state="decode_only", codes="random")
COVER = lg.Case("code16_n8_k1024_cover_p40", 8, 1024, 24, 5, 5000, 10, 40, "cover", L=40, state="decode_only", codes="random")


def _lists_setup(case):
    x = cg.Case(case.N, case.K, case.B, case.Q, case.D, case.k)
    q, d, store, xq, tables, norms, rnorms = _setup(x)
    off, probes = lg.layout(case)
    return q, d, store, tables, norms, rnorms, off, probes


@pytest.mark.parametrize("metric", cg.METRICS)
def test_lists(metric):
    q, d, store, tables, norms, rnorms, off, probes = _lists_setup(LISTS)
    assert (np.diff(off) == 0).any() and (probes == -1).any() and (probes[0] == -1).all()
    off_d, probes_d = _dev(off), _dev(probes)
    w = _w(metric, norms, rnorms)
    wh = None if w is None else w.cpu().numpy()
    T = tables.cpu().numpy()
    s, S = mg.restate_metric_scores(T, wh, d, metric), mg.restate_sums(T, d)
    bias = bg.bias_for(S, off, probes, SEED)
    sb = bg.biased_scores(S, off, probes, bias, wh, metric)
    for pattern in (None, "half"):
        keep = None if pattern is None else kg.keep_for(pattern, LISTS.B, SEED, 10)
        keep_d = None if keep is None else _dev(keep)
        for k in (10, 300):
            scan = q._search_scan if k <= 64 else q._search_wide_scan
            _same_topk(scan(tables, store, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d)),
                       lg.restate_lists(s, off, probes, k, keep), f"lists {metric} {pattern} k={k}")
            _same_topk(scan(tables, store, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d), bias=_dev(bias)),
                       lg.restate_lists(sb, off, probes, k, keep), f"lists {metric} {pattern} k={k} bias")
    dist, idx = q.search_lists(q.decode(store[:17]), store, off_d, probes_d, k=10, metric=metric)
    assert tuple(idx.shape) == (17, 10) and (idx[0] == -1).all()


@pytest.mark.parametrize("metric", cg.METRICS)
def test_every_list_probed_is_the_whole_store(metric):
    q, d, store, tables, norms, rnorms, off, _ = _lists_setup(COVER)
    assert off[0] == 0 and off[-1] == COVER.B
    L = len(off) - 1
    every = lg.all_probes(COVER, L)
    w = _w(metric, norms, rnorms)
    for k in (10, 300):
        whole = q._search_wide_scan(tables, store, w, k, metric=metric)
        assert _equal(whole, q._search_wide_scan(tables, store, w, k, metric=metric, lists=(_dev(off), _dev(every)))), (metric, k)
    s = mg.restate_metric_scores(tables.cpu().numpy(), None if w is None else w.cpu().numpy(), d, metric)
    thr = _dev(rg.thresholds_for(s))
    whole = q._search_range(tables, store, w, thr, metric=metric)
    ascending = _dev(np.sort(every, axis=1))
    assert _equal(whole, q._search_range(tables, store, w, thr, metric=metric, lists=(_dev(off), ascending))), metric


# ------------------------------------------------------------------ the range search
@pytest.mark.parametrize("metric", cg.METRICS)
def test_range_whole_store(metric):
    x = cg.MASK_CASE
    q, d, store, xq, tables, norms, rnorms = _setup(x)
    w = _w(metric, norms, rnorms)
    thr, lims, pos, val = rg.restate(tables.cpu().numpy(), None if w is None else w.cpu().numpy(), d, metric)
    counts = np.diff(lims)
    assert counts[1] == 0 and counts[2] == x.B and counts[0] >= 10 and counts[3] >= 1     # nothing, everything, ten, a hundredth
    _same_range(q._search_range(tables, store, w, _dev(thr), metric=metric), (lims, pos, val), f"range {metric}")
    got = q.range_search(xq, store, 1e30 if metric == "l2" else -1e30, metric=metric)
    assert int(got[0][-1]) == x.Q * x.B and got[2].reshape(x.Q, x.B)[3].tolist() == list(range(x.B))


@pytest.mark.parametrize("metric", cg.METRICS)
def test_range_lists(metric):
    q, d, store, tables, norms, rnorms, off, probes = _lists_setup(LISTS)
    probes = probes.copy()
    probes[3] = [9, 6, 5, 6, 3, 2, 1]                                   # a list named twice is listed twice (rule 18)
    off_d, probes_d = _dev(off), _dev(probes)
    w = _w(metric, norms, rnorms)
    wh = None if w is None else w.cpu().numpy()
    T = tables.cpu().numpy()
    s, S = mg.restate_metric_scores(T, wh, d, metric), mg.restate_sums(T, d)
    bias = bg.bias_for(S, off, probes, SEED)
    sb = bg.biased_scores(S, off, probes, bias, wh, metric)
    for pattern in (None, "half"):
        keep = None if pattern is None else kg.keep_for(pattern, LISTS.B, SEED, 10)
        keep_d = None if keep is None else _dev(keep)
        thr = rl.thresholds_for(s, off, probes, keep)
        want = rl.restate_range_lists(s, off, probes, thr, keep)
        assert want[0][-1] > 0 and (np.diff(want[0]) == 0).any()
        _same_range(q._search_range(tables, store, w, _dev(thr), metric=metric, mask=keep_d, lists=(off_d, probes_d)), want,
                    f"range lists {metric} {pattern}")
        thr = rl.thresholds_for(sb, off, probes, keep)
        _same_range(q._search_range(tables, store, w, _dev(thr), metric=metric, mask=keep_d, lists=(off_d, probes_d), bias=_dev(bias)),
                    bg.restate_range_lists_bias(S, off, probes, bias, wh, metric, thr, keep), f"range lists {metric} {pattern} bias")
    twice = rl.restate_range_lists(s, off, probes[3:4], np.array([np.inf], np.float32))
    assert len(twice[1]) == len(set(twice[1].tolist())) + (off[7] - off[6])


# ------------------------------------------------------------------ hand-made orders
@pytest.mark.parametrize("order", cg.ORDERS)
def test_hand_made_order(order):
    x = cg.Case(cg.ORDER_N, cg.ORDER_K, wg.ORDER_B, wg.ORDER_Q, 24, 1024)
    q = base._quantizer(x.case())
    Q, B, k = x.Q, x.B, x.k
    T = np.full((Q, x.N, x.K), -0.0, dtype=np.float32)                  # a zero query: every table entry is -0.0
    d = cg.digits(x.N, x.K, B)
    w = wg.order_w(order)
    metric = "ip" if order == "all_equal" else "l2"
    s = mg.restate_metric_scores(T[:1], w, d, metric)
    if metric == "l2":
        assert np.array_equal(_bits(s[0]), _bits(w))                    # the score IS w[b], bit for bit
    want_s, want_i = wg.restate_topk_valid(s, k)
    got = q._search_wide_scan(_dev(T), _dev(cg.store(d)), None if metric == "ip" else _dev(w), k, metric=metric)
    _same_topk(got, (np.repeat(want_s, Q, axis=0), np.repeat(want_i, Q, axis=0)), order)
    if order in ("all_equal", "zeros"):
        assert want_i[0].tolist() == list(range(k))
    if order == "descending":
        assert want_i[0].tolist() == list(range(B - 1, B - 1 - k, -1))


# ------------------------------------------------------------------ rule 32: the bits above the digit
@pytest.mark.parametrize("x,bits", cg.HIGH_BITS, ids=lambda v: getattr(v, "name", hex(v) if isinstance(v, int) else None))
def test_high_bits_are_ignored(x, bits):
    q, d, store, xq, tables, norms, rnorms = _setup(x)
    dirty = _dev(cg.with_high_bits(d, bits))
    assert dirty.dtype == torch.int16 and bool((dirty < 0).all()) and not torch.equal(dirty, store)
    assert torch.equal(_i32(q.code_norms(dirty)), _i32(norms)) and torch.equal(_i32(q.code_rnorms(dirty)), _i32(rnorms))
    off = _dev(np.array([0, 100, 100, x.B], dtype=np.int64))
    probes = _dev(np.tile(np.array([[2, 0]], dtype=np.int32), (x.Q, 1)))
    for metric in cg.METRICS:
        w = _w(metric, norms, rnorms)
        for k in (10, 300):
            for kw in (dict(), dict(lists=(off, probes))):
                assert _equal(q._search_wide_scan(tables, dirty, w, k, metric=metric, **kw),
                              q._search_wide_scan(tables, store, w, k, metric=metric, **kw)), (metric, k, sorted(kw))
        assert _equal(q.range_search(xq, dirty, 0.5, metric=metric), q.range_search(xq, store, 0.5, metric=metric))
    assert torch.equal(q.decode(dirty), q.decode(store))


# ------------------------------------------------------------------ against the shipped one-byte kernels
@pytest.mark.parametrize("N,K", cg.CROSS)
def test_cross_check_against_one_byte_entries(N, K):
    from quantization_amd import search
    x = cg.Case(N, K, cg.CROSS_B, cg.CROSS_Q, cg.CROSS_D, 300)
    q, d, store, xq, _, _, _ = _setup(x)
    assert store.dtype == torch.uint8
    wide = store.to(torch.int16)
    Q, B, D = x.Q, x.B, x.D
    st = torch.cuda.current_stream().cuda_stream
    blob = q._prepared(any_flavour=True)
    # tables
    tables = q.search_tables(xq)
    t16 = torch.empty_like(tables)
    search._call("mcq_search_tables_u16", xq.data_ptr(), 0, Q, blob.data_ptr(), N, K, D, t16.data_ptr(), st)
    assert torch.equal(_i32(t16), _i32(tables))
    # norms and reciprocal roots, plain and with a base
    rs = np.random.RandomState(N + K)
    centroids = _dev(rs.standard_normal((7, D)).astype(np.float32))
    assign = _dev(rs.randint(-1, 8, size=B).astype(np.int32))
    for rnorm, old in ((0, q.code_norms), (1, q.code_rnorms)):
        for bs, asg in ((None, None), (centroids, assign)):
            out = torch.empty(B, dtype=torch.float32, device="cuda")
            search._call("mcq_code_norms_u16", wide.data_ptr(), B, blob.data_ptr(), N, K, D, rnorm, None if bs is None else bs.data_ptr(),
                         7, None if asg is None else asg.data_ptr(), out.data_ptr(), st)
            assert torch.equal(_i32(out), _i32(old(store, bs, asg))), (rnorm, bs is not None)
    norms = q.code_norms(store)
    rnorms = q.rnorms_from_norms(norms)
    case = lg.Case("cross", N, K, D, Q, B, 10, 40, "cover", L=40)
    off, probes = lg.layout(case)
    off_d, probes_d = _dev(off), _dev(probes)
    S = mg.restate_sums(tables.cpu().numpy(), d)
    bias_d = _dev(bg.bias_for(S, off, probes, SEED))
    keep_d = _dev(kg.keep_for("half", B, SEED, 10))
    for metric in cg.METRICS:
        w = _w(metric, norms, rnorms)
        for k in (10, 64, 300):
            narrow = k <= 64
            for kw in (dict(), dict(mask=keep_d), dict(lists=(off_d, probes_d), bias=bias_d), dict(lists=(off_d, probes_d), bias=bias_d, mask=keep_d)):
                old = (q._search_scan if narrow else q._search_wide_scan)(tables, store, w, k, metric=metric, **kw)
                assert _equal(q._search_wide_scan(tables, wide, w, k, metric=metric, **kw), old), (metric, k, sorted(kw))
        s = mg.restate_metric_scores(tables.cpu().numpy(), None if w is None else w.cpu().numpy(), d, metric)
        thr = _dev(rg.thresholds_for(s))
        for kw in (dict(), dict(mask=keep_d), dict(lists=(off_d, probes_d)), dict(lists=(off_d, probes_d), bias=bias_d, mask=keep_d)):
            new, old = q._search_range(tables, wide, w, thr, metric=metric, **kw), q._search_range(tables, store, w, thr, metric=metric, **kw)
            assert _equal(new, old) and int(old[0][-1]) > 0, (metric, sorted(kw))


# ------------------------------------------------------------------ which entries a call names
def test_routing(monkeypatch):
    from quantization_amd import Quantizer, _lib, search
    named = []
    real = search._entry
    monkeypatch.setattr(search, "_entry", lambda name: (named.append(name), real(name))[1])
    neutral = {"mcq_search_pack_mask", "mcq_rnorms_from_norms"}           # they never see a code
    before = set(_lib.SYMBOLS) | set(_lib.RESIDUAL_SYMBOLS) | set(_lib.WIDE_SYMBOLS)

    def calls(q, store):
        B = store.shape[0]
        x = torch.randn(3, 24, device="cuda")
        off = _dev(np.array([0, 100, B], dtype=np.int64))
        probes = _dev(np.array([[0, 1], [1, -1], [0, -1]], dtype=np.int32))
        keep = torch.rand(B, device="cuda") < 0.5
        bias = torch.randn(3, 2, device="cuda")
        norms = q.code_norms(store)
        q.code_rnorms(store)
        q.code_norms(store, base=torch.randn(2, 24, device="cuda"), assign=torch.zeros(B, dtype=torch.int64, device="cuda"))
        q.search_tables(x)
        for metric in cg.METRICS:
            q.search(x, store, k=10, metric=metric, norms=norms)
            q.search(x, store, k=10, metric=metric, mask=keep)
            q.search_lists(x, store, off, probes, k=10, metric=metric, probe_bias=bias)
            q.search_wide(x, store, 300, metric=metric)
            q.search_lists_wide(x, store, off, probes, 300, metric=metric, mask=keep)
            q.range_search(x, store, 0.0, metric=metric)
            q.range_search_lists(x, store, off, probes, 0.0, metric=metric, probe_bias=bias)

    small = Quantizer(24, 256, 4).to("cuda:0").requires_grad_(False)
    calls(small, torch.randint(0, 256, (300, 4), dtype=torch.uint8, device="cuda"))
    assert named and set(named) <= before and not set(named) & set(_lib.CODE16_SYMBOLS)
    with pytest.raises(_lib.McqError, match="uint8 codes"):
        small.search(torch.randn(3, 24, device="cuda"), torch.zeros(300, 4, dtype=torch.int16, device="cuda"))
    del named[:]
    big = Quantizer(24, 1024, 4).to("cuda:0").requires_grad_(False)
    calls(big, big.pack_codes(torch.randint(0, 1024, (300, 4), device="cuda")))
    assert set(named) - neutral == set(_lib.CODE16_SYMBOLS), sorted(set(named) ^ set(_lib.CODE16_SYMBOLS))


# ------------------------------------------------------------------ end to end on the reference's fixtures
@pytest.mark.parametrize("name", cg.FIXTURES)
def test_end_to_end_on_a_reference_fixture(name):
    import test_gpu_parity as parity
    fx = fixtures.load(name)
    N, K, D, B = fx["N"], fx["K"], fx["D"], fx["B"]
    q = parity.load_quantizer(fx["state"], D, K, N).requires_grad_(False)
    it = fx["iters"][-1]
    x = torch.from_numpy(fx["x"]).cuda()
    digits = q.encode(x, it, as_bytes=False)
    fixtures.check_codes(fx, it, digits.cpu().numpy(), f"{name} iters={it}")
    store = q.pack_codes(digits)
    assert store.dtype == torch.int16 and store.element_size() * store.numel() * 4 == digits.element_size() * digits.numel()
    d = digits.cpu().numpy()
    assert d.max() > 255
    assert torch.equal(q.decode(store), q.decode(digits))               # bit for bit: the int16 store is widened
    Q, k = 64, 10
    rs = np.random.RandomState(3)
    xq = (fx["x"][:Q] + 0.01 * rs.standard_normal((Q, D))).astype(np.float32)
    xq_d = _dev(xq)
    Cp = _padded_centers(q)
    C = np.ascontiguousarray(Cp[:, :, :D])
    rows = np.arange(Q)[:, None]
    # L2: the derived bound of tests/test_gpu_search.py -- the N table bounds, the norm bound, and the rounding of |q|^2
    _, tb = tg.tables_bound(xq, Cp, D)
    tb = tb.reshape(Q, N, K)
    _, nb = tg.norms_bound(Cp, d, D)
    dec = np.zeros((B, D))
    for n in range(N):
        dec += C[n].astype(np.float64)[d[:, n]]
    qq = (xq.astype(np.float64) ** 2).sum(1)
    exact_l2 = qq[:, None] - 2.0 * xq.astype(np.float64) @ dec.T + (dec ** 2).sum(1)[None, :]
    bound_l2 = nb[None, :] + D * tg.EPS * qq[:, None]
    for n in range(N):
        bound_l2 = bound_l2 + tb[:, n, :][:, d[:, n]]
    dist, idx = q.search(xq_d, store, k=k)
    dist, idx = dist.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert ((idx >= 0) & (idx < B)).all()
    err = np.abs(dist - np.maximum(exact_l2[rows, idx], 0.0))
    print(f"[code16] {name} l2: largest |distance - float64| / bound = {float((err / bound_l2[rows, idx]).max()):.4f}")
    assert (err <= bound_l2[rows, idx]).all()
    radius = float(np.sort(exact_l2, axis=1)[:, 9].mean())
    lims, val, pos = q.range_search(xq_d, store, radius)
    lims, val, pos = lims.cpu().numpy(), val.cpu().numpy().astype(np.float64), pos.cpu().numpy()
    qrow = np.repeat(np.arange(Q), np.diff(lims))
    assert len(pos) > 0 and (np.abs(val - np.maximum(exact_l2[qrow, pos], 0.0)) <= bound_l2[qrow, pos]).all()
    for metric in mg.METRICS:
        exact, bound = mg.similarity_bound(xq, C, d, metric)
        sim, idx = q.search(xq_d, store, k=k, metric=metric)
        sim, idx = sim.cpu().numpy().astype(np.float64), idx.cpu().numpy()
        err = np.abs(sim - exact[rows, idx])
        print(f"[code16] {name} {metric}: largest |similarity - float64| / bound = {float((err / bound[rows, idx]).max()):.4f}")
        assert ((idx >= 0) & (idx < B)).all() and (err <= bound[rows, idx]).all()
        radius = float(np.sort(exact, axis=1)[:, -10].mean())
        lims, val, pos = q.range_search(xq_d, store, radius, metric=metric)
        lims, val, pos = lims.cpu().numpy(), val.cpu().numpy().astype(np.float64), pos.cpu().numpy()
        qrow = np.repeat(np.arange(Q), np.diff(lims))
        assert len(pos) > 0 and (np.abs(val - exact[qrow, pos]) <= bound[qrow, pos]).all()
