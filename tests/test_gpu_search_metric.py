"""The inner-product and cosine metrics of the search over stored codes on the GPU, BIT FOR BIT against rules 3', 4 and 6 of
include/mcq.h restated in numpy (tests/search_metric_grid.py), and the behaviour of Quantizer.search(metric=...) around them.

Per case of the L2 table (tests/search_grid.py: query tiles, slices, partial last steps, strided waves, short stores, B = 1,
packed codes, fp16 queries, the decode-only state, duplicated codes) and per metric:
  * code_rnorms(codes) and rnorms_from_norms(code_norms(codes)) EQUAL float32(1) / sqrt(t) with 0 where t == 0, formed in numpy
    from the t the device returned;
  * the scores and indexes of the scan EQUAL the restatement formed from the device's tables and reciprocal roots: every row,
    no tolerance -- the contract makes the result a function of tables, w and codes;
  * search(metric=...) returns those indexes and the similarities -0.5 * score (and / |q| for the cosine);
  * a second call returns identical bits.
That the tables and sums MEAN the inner product and the cosine (sign, factor) is tests/test_gpu_search_metric_definition.py."""
import numpy as np
import pytest
import torch

import search_grid as sg
import search_metric_grid as mg
import test_gpu_search as base

pytestmark = pytest.mark.gpu

_CACHE = {}


def _prepared(case):
    """the store, the queries and what the device made of them, shared by the metrics of one case"""
    if _CACHE.get("name") != case.name:
        _CACHE.clear()
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, rows = base._queries(case, q, kept)
        tables, norms = q.search_tables(xq), q.code_norms(kept)
        _CACHE.update(name=case.name, v=(q, kept, flat, xq, tables, norms))
    return _CACHE["v"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("metric", mg.METRICS)
@pytest.mark.parametrize("case", mg.CASES, ids=lambda c: c.name)
def test_metric_case(case, metric):
    q, kept, flat, xq, tables, norms = _prepared(case)
    Q, B, k, N, K = case.Q, case.B, case.k, case.N, case.K
    T, t = tables.cpu().numpy(), norms.cpu().numpy()

    # rule 6: the reciprocal roots, both ways
    r_want = mg.restate_rnorms(t)
    rn = q.code_rnorms(kept)
    rn2 = q.rnorms_from_norms(norms)
    assert rn.dtype == torch.float32 and tuple(rn.shape) == (B,)
    assert np.array_equal(_bits(rn.cpu().numpy()), _bits(r_want)), "code_rnorms differs from 1 / sqrt(t)"
    assert torch.equal(rn.view(torch.int32), rn2.view(torch.int32)), "rnorms_from_norms differs from code_rnorms"
    assert np.isfinite(r_want).all()

    # rules 3' and 4: the scan
    flat_d = torch.from_numpy(flat).cuda()
    w = None if metric == "ip" else rn
    s1, i1 = q._search_scan(tables, flat_d, w, k, metric=metric)
    assert s1.dtype == torch.float32 and i1.dtype == torch.int64 and tuple(s1.shape) == tuple(i1.shape) == (Q, k)
    want_s, want_i = mg.restate_metric(T, r_want, flat, k, metric)
    got_s, got_i = s1.cpu().numpy(), i1.cpu().numpy()
    assert np.array_equal(got_i, want_i), f"indexes differ in rows {np.flatnonzero((got_i != want_i).any(1))[:8]}"
    assert torch.equal(s1.view(torch.int32), torch.from_numpy(want_s).view(torch.int32).cuda()), "scores differ from rule 3'"
    if metric == "ip":                                  # w is ignored: any array gives the same lists
        s0, i0 = q._search_scan(tables, flat_d, norms, k, metric=metric)
        assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)) and torch.equal(i0, i1)

    # the public call: the same lists, as similarities
    sim, idx = q.search(xq, kept, k=k, metric=metric)
    assert sim.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(sim.shape) == tuple(idx.shape) == (Q, k)
    assert np.array_equal(idx.cpu().numpy(), want_i)
    half = s1 * -0.5
    if metric == "ip":
        assert torch.equal(sim.view(torch.int32), half.view(torch.int32))
    else:
        xf = xq.float()
        qn = (xf * xf).sum(1, keepdim=True).sqrt()
        assert bool((qn > 0).all())
        assert torch.equal(sim.view(torch.int32), (half / qn).view(torch.int32))
        simf = sim.cpu().numpy()[want_i >= 0]
        assert (np.abs(simf) <= 1.0 + 1e-3).all()
    m = min(k, B)
    simh = sim.cpu().numpy()
    assert np.isfinite(simh[:, :m]).all() and (np.diff(simh[:, :m], axis=1) <= 0).all()       # largest first
    if case.short:
        assert (want_i[:, B:] == -1).all() and (simh[:, B:] == -np.inf).all() and (got_s[:, B:] == np.inf).all()

    # determinism
    s2, i2 = q._search_scan(tables, flat_d, w, k, metric=metric)
    sim2, idx2 = q.search(xq, kept, k=k, metric=metric)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(i1, i2)
    assert torch.equal(sim.view(torch.int32), sim2.view(torch.int32)) and torch.equal(idx, idx2)


# ------------------------------------------------------------------ behaviour
def _small(N=8, K=256, D=24, name="behaviour"):
    return base._quantizer(sg.Case(name, N, K, D, 3, 100, 10))


def test_l2_is_the_default_and_unchanged():
    q = _small()
    x = torch.randn(2, 3, 24, device="cuda")
    codes = torch.randint(0, 256, (1000, 8), dtype=torch.uint8, device="cuda")
    d0, i0 = q.search(x, codes, k=7)
    d1, i1 = q.search(x, codes, k=7, metric="l2")
    d2, i2 = q.search(x, codes, 7, q.code_norms(codes), "l2")
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(i0, i1)
    assert torch.equal(d0.view(torch.int32), d2.view(torch.int32)) and torch.equal(i0, i2)
    # mcq_search_scan_metric(MCQ_SEARCH_L2) is mcq_search_scan
    from quantization_amd import _lib
    L = _lib.lib()
    tables, norms = q.search_tables(x), q.code_norms(codes)
    s_a, i_a = q._search_scan(tables, codes, norms, 7)
    s_b, i_b = torch.empty_like(s_a), torch.empty_like(i_a)
    ws = torch.empty(L.mcq_search_workspace_bytes(6, 1000, 8, 256, 7), dtype=torch.uint8, device="cuda")
    rc = L.mcq_search_scan_metric(tables.data_ptr(), 6, codes.data_ptr(), norms.data_ptr(), 1000, 8, 256, 7, _lib.MCQ_SEARCH_L2,
                                  s_b.data_ptr(), i_b.data_ptr(), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(s_a.view(torch.int32), s_b.view(torch.int32)) and torch.equal(i_a, i_b)


@pytest.mark.parametrize("metric", mg.METRICS)
def test_metric_interface(metric):
    from quantization_amd._lib import McqError
    q = _small()
    x = torch.randn(2, 3, 24, device="cuda")
    codes = torch.randint(0, 256, (100, 8), dtype=torch.uint8, device="cuda")
    s, i = q.search(x, codes, k=5, metric=metric)
    assert tuple(s.shape) == tuple(i.shape) == (2, 3, 5) and not s.requires_grad
    with pytest.raises(ValueError):
        q.search(x, codes, k=5, metric="nonsense")
    with pytest.raises(McqError):
        q.search(x.cpu(), codes, metric=metric)
    with pytest.raises(McqError):
        q.search(x, codes.cpu(), metric=metric)
    with pytest.raises(McqError):
        q.search(x, codes, k=65, metric=metric)
    # an empty store, a short one and no queries: the mirror of rule 4's fill
    s, i = q.search(x, codes[:0], k=4, metric=metric)
    assert bool((s == float("-inf")).all()) and bool((i == -1).all())
    s, i = q.search(x, codes[:3], k=5, metric=metric)
    assert bool((s[..., 3:] == float("-inf")).all()) and bool((i[..., 3:] == -1).all())
    assert bool(torch.isfinite(s[..., :3]).all()) and bool((i[..., :3] >= 0).all())
    s, i = q.search(x[:0], codes, k=4, metric=metric)
    assert tuple(s.shape) == (0, 3, 4)
    # a non-finite query neither faults nor hangs (its row is unspecified); the other rows are those of a clean run
    xb = x.clone().reshape(6, 24)
    xb[1, 3] = float("nan")
    xb[2, 0] = float("inf")
    s, i = q.search(xb, codes, k=4, metric=metric)
    torch.cuda.synchronize()
    s2, i2 = q.search(x.reshape(6, 24), codes, k=4, metric=metric)
    keep = [0, 3, 4, 5]
    assert torch.equal(i[keep], i2[keep]) and torch.equal(s[keep].view(torch.int32), s2[keep].view(torch.int32))


def test_zero_query_under_cosine():
    q = _small()
    x = torch.randn(4, 24, device="cuda")
    x[2] = 0
    codes = torch.randint(0, 256, (500, 8), dtype=torch.uint8, device="cuda")
    s, i = q.search(x, codes, k=6, metric="cosine")
    assert bool(torch.isfinite(s).all()) and bool((s[2] == 0).all())
    assert i[2].tolist() == list(range(6))                   # every score equal: position decides
    s_ip, i_ip = q.search(x, codes, k=6, metric="ip")
    assert bool((s_ip[2] == 0).all()) and i_ip[2].tolist() == list(range(6))
    clean = q.search(x[[0, 1, 3]], codes, k=6, metric="cosine")
    assert torch.equal(s[[0, 1, 3]].view(torch.int32), clean[0].view(torch.int32)) and torch.equal(i[[0, 1, 3]], clean[1])


def test_all_zero_reconstruction_scores_zero():
    """a decode-only state in which two codes decode to exactly 0: centers that cancel, and centers that are zero"""
    from quantization_amd import Quantizer
    from quantization_amd import synthetic as gen
    N, K, D = 2, 16, 24
    sd = gen.synthetic_state(5, D, K, N)
    c = np.array(sd["centers"], dtype=np.float32).reshape(N, K, D)
    c[1, 0] = -c[0, 0]                                       # code (0, 0): the rows cancel
    c[0, 1] = 0
    c[1, 1] = 0                                              # code (1, 1): zero rows
    sd["centers"] = c.reshape(np.asarray(sd["centers"]).shape)
    q = Quantizer(D, K, N)
    st = q.state_dict()
    for k_, v in sd.items():
        st[k_] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(st)
    q = q.to("cuda:0").requires_grad_(False)
    rs = np.random.RandomState(2)
    flat = rs.randint(2, K, size=(300, N)).astype(np.uint8)
    flat[7] = (0, 0)
    flat[130] = (1, 1)
    codes = torch.from_numpy(flat).cuda()
    dec = q.decode(codes)
    assert q._prep.flavour == "decode"
    assert not bool(dec[[7, 130]].any()) and bool(dec[0].any())
    t, r = q.code_norms(codes), q.code_rnorms(codes)
    assert t[7] == 0 and t[130] == 0 and r[7] == 0 and r[130] == 0
    assert bool(torch.isfinite(r).all()) and int((r == 0).sum()) == 2
    assert torch.equal(r, q.rnorms_from_norms(t))
    x = torch.randn(5, D, device="cuda")
    tables = q.search_tables(x)
    s, i = q._search_scan(tables, codes, r, 64, metric="cosine")      # k = 64 of 300: deep enough for a score of 0 to be listed
    sim, idx = q.search(x, codes, k=64, metric="cosine")
    assert bool(torch.isfinite(s).all()) and bool(torch.isfinite(sim).all()) and torch.equal(i, idx)
    full_s, full_i = [], []
    for a in range(0, 300, 60):                                       # every stored vector's similarity, 60 at a time
        ss, ii = q.search(x, codes[a:a + 60], k=60, metric="cosine")
        full_s.append(ss)
        full_i.append(ii + a)
    full_s, full_i = torch.cat(full_s, 1), torch.cat(full_i, 1)
    assert bool(torch.isfinite(full_s).all())
    for b in (7, 130):
        assert bool((full_s[full_i == b] == 0).all()) and int((full_i == b).sum()) == 5
    assert int((full_s == 0).sum()) == 10


def test_ip_forms_no_norms_and_cosine_takes_either():
    q = _small()
    x = torch.randn(9, 24, device="cuda")
    codes = torch.randint(0, 256, (5000, 8), dtype=torch.uint8, device="cuda")
    norms, rnorms = q.code_norms(codes), q.code_rnorms(codes)
    calls = {"norms": 0, "rnorms": 0, "conv": 0}
    real = (q.code_norms, q.code_rnorms, q.rnorms_from_norms)

    def counted(name, fn):
        def f(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return f
    q.code_norms, q.code_rnorms, q.rnorms_from_norms = (counted(n, f) for n, f in zip(("norms", "rnorms", "conv"), real))
    try:
        q.search(x, codes, k=10, metric="ip")
        q.search(x, codes, k=10, metric="ip", norms=norms)
        assert calls == {"norms": 0, "rnorms": 0, "conv": 0}
        a = q.search(x, codes, k=10, metric="cosine")
        assert calls == {"norms": 0, "rnorms": 1, "conv": 0}
        b = q.search(x, codes, k=10, metric="cosine", norms=norms)
        assert calls == {"norms": 0, "rnorms": 1, "conv": 1}
        c = q.search(x, codes, k=10, metric="cosine", rnorms=rnorms)
        d = q.search(x, codes, k=10, metric="cosine", norms=norms, rnorms=rnorms)
        assert calls == {"norms": 0, "rnorms": 1, "conv": 1}
    finally:
        del q.code_norms, q.code_rnorms, q.rnorms_from_norms
    for other in (b, c, d):
        assert torch.equal(a[0].view(torch.int32), other[0].view(torch.int32)) and torch.equal(a[1], other[1])
