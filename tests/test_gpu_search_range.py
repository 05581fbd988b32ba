"""The range search over stored codes on the GPU (Quantizer._search_range / range_search; include/mcq.h rules 7-9), BIT FOR BIT
against the numpy restatement of tests/search_range_grid.py.

Per case of its table (query tiles, slices, waves of several steps, idle waves, partial last steps, empty and complete results,
thresholds that are scores, duplicated codes, packed codes, fp16 queries, the decode-only state, 1,048,593 stored vectors) and
per metric:
  * lims, positions and scores of _search_range EQUAL the restatement formed from the tables and the per-candidate array the
    device returned: torch.equal, no tolerance, nothing left out;
  * with thr[q] = the k-th score _search_scan returned, the listed set is the top-k positions plus every position tied with
    that score: the two kernels agree on one arithmetic;
  * range_search reports search's values for the positions both report;
  * a second call returns identical bytes.
Then the interface of range_search."""
import numpy as np
import pytest
import torch

import search_grid as sg
import search_metric_grid as mg
import search_range_grid as rg
import test_gpu_search as base

pytestmark = pytest.mark.gpu

_CACHE = {}


def _prepared(case):
    """the store, the queries and what the device made of them, shared by the metrics of one case"""
    if _CACHE.get("name") != case.name:
        _CACHE.clear()
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, _ = base._queries(case, q, kept)
        tables, norms = q.search_tables(xq), q.code_norms(kept)
        _CACHE.update(name=case.name, v=(q, kept, flat, xq, tables, norms, q.rnorms_from_norms(norms)))
    return _CACHE["v"]


def _i32(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("metric", rg.METRICS)
@pytest.mark.parametrize("case", rg.CASES, ids=lambda c: c.name)
def test_range_case(case, metric):
    q, kept, flat, xq, tables, norms, rnorms = _prepared(case)
    Q, B, N, K = case.Q, case.B, case.N, case.K
    T = tables.cpu().numpy()
    w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
    w_h = None if w is None else w.cpu().numpy()
    flat_d = torch.from_numpy(flat).cuda()

    # rules 7 and 8 against the restatement
    thr, want_lims, want_pos, want_val = rg.restate(T, w_h, flat, metric)
    thr_d = torch.from_numpy(thr).cuda()
    lims, val, pos = q._search_range(tables, flat_d, w, thr_d, metric)
    assert lims.dtype == torch.int64 and pos.dtype == torch.int64 and val.dtype == torch.float32
    assert tuple(lims.shape) == (Q + 1,) and tuple(pos.shape) == tuple(val.shape) == (int(want_lims[-1]),)
    n_got, n_want = (lims[1:] - lims[:-1]).cpu().numpy(), np.diff(want_lims)
    print(f"[range] {case.name} {metric}: {int(want_lims[-1])} entries, per query min {n_want.min()} max {n_want.max()}")
    assert torch.equal(lims, torch.from_numpy(want_lims).cuda()), f"counts differ for queries {np.flatnonzero(n_got != n_want)[:8]}"
    assert torch.equal(pos, torch.from_numpy(want_pos).cuda()), "positions differ from rule 8"
    assert torch.equal(_i32(val), _i32(torch.from_numpy(want_val).cuda())), "scores differ from rule 3'"
    if case.empty:
        assert (n_want == 0).any()
    if case.full:
        assert (n_want == B).any()

    # determinism: a second call gives the same bytes
    lims2, val2, pos2 = q._search_range(tables, flat_d, w, thr_d, metric)
    assert torch.equal(lims, lims2) and torch.equal(pos, pos2) and torch.equal(_i32(val), _i32(val2))

    # the top-k scan and the range sweep agree on one arithmetic
    k = case.k
    m = min(k, B)
    s_k, i_k = q._search_scan(tables, flat_d, w, k, metric=metric)
    kth = s_k[:, m - 1].contiguous()
    lims3, val3, pos3 = q._search_range(tables, flat_d, w, kth, metric)
    l3, v3, p3 = lims3.cpu().numpy(), val3.cpu().numpy(), pos3.cpu().numpy()
    s_h, i_h, kth_h = s_k.cpu().numpy(), i_k.cpu().numpy(), kth.cpu().numpy()
    for qi in range(Q):
        listed, scores = p3[l3[qi]:l3[qi + 1]], v3[l3[qi]:l3[qi + 1]]
        top = i_h[qi, :m]
        assert (np.diff(listed) > 0).all()
        assert np.isin(top, listed).all(), (qi, "a top-k position is not listed")
        extra = ~np.isin(listed, top)
        assert (scores[extra] == kth_h[qi]).all(), (qi, "a listed position outside the top k does not tie the k-th score")
        assert int((scores < kth_h[qi]).sum()) == int((s_h[qi, :m] < kth_h[qi]).sum())
        order = np.argsort(top)
        assert np.array_equal(scores[np.isin(listed, top)].view(np.uint32), s_h[qi, :m][order].view(np.uint32))

    # the public call: search's values at the positions both report (a radius a little past the k-th value lists the top k)
    a_val, a_idx = q.search(xq, kept, k=k, norms=norms, metric=metric, rnorms=rnorms)
    edge = a_val[:, m - 1]
    radius = edge * (1 + 1e-3) + 1e-3 if metric == "l2" else edge - edge.abs() * 1e-3 - 1e-3
    r_lims, r_val, r_idx = q.range_search(xq, kept, radius, norms=norms, metric=metric, rnorms=rnorms)
    assert r_lims.dtype == torch.int64 and r_val.dtype == torch.float32 and r_idx.dtype == torch.int64
    rl, rv, ri = r_lims.cpu().numpy(), r_val.cpu().numpy(), r_idx.cpu().numpy()
    av, ai = a_val.cpu().numpy(), a_idx.cpu().numpy()
    for qi in range(Q):
        listed, values = ri[rl[qi]:rl[qi + 1]], rv[rl[qi]:rl[qi + 1]]
        top = ai[qi, :m]
        assert np.isin(top, listed).all(), (qi, "range_search misses a position search reports")
        order = np.argsort(top)
        assert np.array_equal(values[np.isin(listed, top)].view(np.uint32), av[qi, :m][order].view(np.uint32)), qi
        if metric == "l2":
            assert (values >= 0).all()
    r2 = q.range_search(xq, kept, radius, norms=norms, metric=metric, rnorms=rnorms)
    assert torch.equal(r_lims, r2[0]) and torch.equal(_i32(r_val), _i32(r2[1])) and torch.equal(r_idx, r2[2])


# ------------------------------------------------------------------ behaviour
def _small(N=8, K=256, D=24):
    return base._quantizer(sg.Case("behaviour", N, K, D, 3, 100, 10))


@pytest.mark.parametrize("metric", rg.METRICS)
def test_range_interface(metric):
    from quantization_amd._lib import McqError
    q = _small()
    x = torch.randn(2, 3, 24, device="cuda")
    codes = torch.randint(0, 256, (1000, 8), dtype=torch.uint8, device="cuda")
    val, idx = q.search(x, codes, k=20, metric=metric)
    val = val.reshape(6, 20)
    radius = float(val[:, 10].max() if metric == "l2" else val[:, 10].min())
    lims, v, i = q.range_search(x, codes, radius, metric=metric)
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and i.dtype == torch.int64
    assert tuple(lims.shape) == (7,) and v.ndim == i.ndim == 1 and v.numel() == i.numel() == int(lims[-1]) > 0
    assert int(lims[0]) == 0 and bool((lims[1:] >= lims[:-1]).all()) and not v.requires_grad
    assert bool((v <= radius * (1 + 1e-5) + 1e-5).all()) if metric == "l2" else bool((v >= radius - 1e-5).all())
    for qi in range(6):
        a = i[int(lims[qi]):int(lims[qi + 1])]
        assert bool((a[1:] > a[:-1]).all()) and bool((a >= 0).all()) and bool((a < 1000).all())
    # a tensor of radii: one per query, any shape of Q values; the scalar is the same as a constant tensor
    t_lims, t_v, t_i = q.range_search(x, codes, torch.full((2, 3), radius, device="cuda"), metric=metric)
    assert torch.equal(lims, t_lims) and torch.equal(_i32(v), _i32(t_v)) and torch.equal(i, t_i)
    per = val[:, 5].clone()
    p_lims, p_v, p_i = q.range_search(x, codes, per, metric=metric)
    assert bool(((p_lims[1:] - p_lims[:-1]) >= 5).all())
    with pytest.raises((ValueError, McqError)):
        q.range_search(x, codes, torch.zeros(5, device="cuda"), metric=metric)
    with pytest.raises(ValueError):
        q.range_search(x, codes, radius, metric="nonsense")
    with pytest.raises(McqError):
        q.range_search(x.cpu(), codes, radius, metric=metric)
    with pytest.raises(McqError):
        q.range_search(x, codes.cpu(), radius, metric=metric)
    # more results than the caller allows: an error that names the count, before anything is allocated for them
    total = int(lims[-1])
    with pytest.raises(McqError, match=str(total)):
        q.range_search(x, codes, radius, metric=metric, max_results=total - 1)
    ok = q.range_search(x, codes, radius, metric=metric, max_results=total)
    assert torch.equal(ok[2], i)
    # no queries, an empty store: lims is all zeros and the lists are empty (rule 9)
    e_lims, e_v, e_i = q.range_search(x[:0], codes, radius, metric=metric)
    assert e_lims.tolist() == [0] and e_v.numel() == e_i.numel() == 0
    e_lims, e_v, e_i = q.range_search(x, codes[:0], radius, metric=metric)
    assert e_lims.tolist() == [0] * 7 and e_v.numel() == e_i.numel() == 0
    # a query with a NaN neither faults nor hangs and lists nothing (rule 7); the other rows are those of a clean run
    xb = x.clone().reshape(6, 24)
    xb[1, 3] = float("nan")
    b_lims, b_v, b_i = q.range_search(xb, codes, radius, metric=metric)
    torch.cuda.synchronize()
    assert int(b_lims[2] - b_lims[1]) == 0
    for qi in (0, 2, 3, 4, 5):
        a, b = slice(int(lims[qi]), int(lims[qi + 1])), slice(int(b_lims[qi]), int(b_lims[qi + 1]))
        assert torch.equal(i[a], b_i[b]) and torch.equal(_i32(v[a]), _i32(b_v[b]))
    # ... and so does a NaN threshold
    nan_r = torch.full((6,), radius, device="cuda")
    nan_r[4] = float("nan")
    n_lims = q.range_search(x, codes, nan_r, metric=metric)[0]
    assert int(n_lims[5] - n_lims[4]) == 0 and int(n_lims[4]) == int(lims[4]) and int(n_lims[-1]) == total - int(lims[5] - lims[4])


def test_wide_codebooks_are_refused():
    from quantization_amd import Quantizer
    from quantization_amd._lib import McqError
    q = Quantizer(24, 512, 4).to("cuda:0").requires_grad_(False)
    x = torch.randn(3, 24, device="cuda")
    with pytest.raises(McqError):
        q.range_search(x, torch.zeros((10, 4), dtype=torch.uint8, device="cuda"), 1.0)


def test_zero_query_under_cosine():
    q = _small()
    x = torch.randn(4, 24, device="cuda")
    x[2] = 0
    codes = torch.randint(0, 256, (500, 8), dtype=torch.uint8, device="cuda")
    for radius, want in ((0.5, 0), (1e-30, 0), (0.0, 500), (-0.5, 500)):
        lims, v, i = q.range_search(x, codes, radius, metric="cosine")
        assert int(lims[3] - lims[2]) == want, radius
        if want:
            a = slice(int(lims[2]), int(lims[3]))
            assert i[a].tolist() == list(range(500)) and bool((v[a] == 0).all())
        clean = q.range_search(x[[0, 1, 3]], codes, radius, metric="cosine")
        keep = torch.cat([torch.arange(int(lims[0]), int(lims[2])), torch.arange(int(lims[3]), int(lims[4]))]).cuda()
        assert torch.equal(i[keep], clean[2]) and torch.equal(_i32(v[keep]), _i32(clean[1]))
    assert bool(torch.isfinite(v).all())


def test_fill_respects_capacity():
    """the raw C call: a fill with less room than lims[Q] stores the entries whose slot is below the capacity and nothing else"""
    from quantization_amd import _lib
    L = _lib.lib()
    q = _small()
    Q, B, N, K = 5, 3000, 8, 256
    x = torch.randn(Q, 24, device="cuda")
    codes = torch.randint(0, 256, (B, N), dtype=torch.uint8, device="cuda")
    tables, norms = q.search_tables(x), q.code_norms(codes)
    thr = torch.full((Q,), float("inf"), device="cuda")
    lims, val, pos = q._search_range(tables, codes, norms, thr, "l2")
    assert int(lims[-1]) == Q * B
    cap = 2 * B + 77
    guard = 1000
    out_s = torch.full((cap + guard,), -7.0, device="cuda")
    out_i = torch.full((cap + guard,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.mcq_search_range_workspace_bytes(Q, B, N, K), dtype=torch.uint8, device="cuda")
    lims2 = torch.empty(Q + 1, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = (tables.data_ptr(), Q, codes.data_ptr(), norms.data_ptr(), B, N, K, _lib.MCQ_SEARCH_L2, thr.data_ptr(), lims2.data_ptr())
    assert L.mcq_search_range_count(*args, ws.data_ptr(), ws.numel(), st) == 0
    assert L.mcq_search_range_fill(*args, out_s.data_ptr(), out_i.data_ptr(), cap, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(lims2, lims)
    assert torch.equal(out_i[:cap], pos[:cap]) and torch.equal(_i32(out_s[:cap]), _i32(val[:cap]))
    assert bool((out_i[cap:] == -7).all()) and bool((out_s[cap:] == -7.0).all())
