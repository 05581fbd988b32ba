"""The exact re-ranking of a shortlist on the GPU (mcq_rerank through ctypes, quantization_amd.rerank; include/mcq_rerank.h
rules 28-31), BIT FOR BIT -- scores as int32 views, and positions -- against the numpy restatement of tests/rerank_grid.py.
No tolerance appears before the last test, whose bound is rerank_grid.error_bound (derived there).

  cases         the table of tests/rerank_grid.py: D = 1 .. 16,384, the four dtype pairings, S on both sides of k and of the
                group, Q = 1, 17, 300 and one Q whose plan has a single part; shortlists with -1 in the middle and at the
                end, a row of -1 only, the values B, 2**40 and -7, duplicates; row_of as a permutation with entries outside
                [0, B); views one element into their storage.  The workspace and both outputs are pre-filled with 0xA5 bytes.
  orders        S = 3,000 at k = 1,024 and 100 in ONE part: descending true distance (every candidate enters: the flush runs
                throughout), ascending, all rows equal (position decides), rows giving +inf and NaN; the k = 100 result is
                the prefix of the k = 1,024 result
  cosine zeros  a zero row and a zero query
  launch        a query alone and among 300; a shortlist row and its reversal; row_of = arange and row_of = None
  selection     every cell of launch_rerank once
  public call   leading dimensions, int32 shortlists, shortlists straight from search_wide / search_lists_wide, the errors
  end to end    the residual recipe of tests/test_gpu_search_residual.py: search_lists_wide(k = 300), then rerank(k = 10)"""
import numpy as np
import pytest
import torch

import rerank_grid as rg

pytestmark = pytest.mark.gpu


def _lib():
    from quantization_amd import _lib
    return _lib


def _dev(a, view=False):
    """numpy -> device tensor; view: one element into its storage (the base pointer is aligned to the element alone)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not view:
        return t.cuda()
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    out = store[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def _abi(q_d, x_d, short_d, k, metric, row_of_d=None):
    """mcq_rerank with the workspace and both outputs pre-filled with 0xA5 bytes -> (scores, positions) on the device"""
    m = _lib()
    L = m.lib()
    (Q, D), B, S = q_d.shape, x_d.shape[0], short_d.shape[1]
    need = L.mcq_rerank_workspace_bytes(Q, S, D, k)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    scores = torch.full((Q, k), 0xA5, dtype=torch.uint8, device="cuda").repeat(1, 4).view(torch.float32)
    pos = torch.full((Q, k), 0xA5, dtype=torch.uint8, device="cuda").repeat(1, 8).view(torch.int64)
    assert scores.shape == pos.shape == (Q, k)
    rc = L.mcq_rerank(q_d.data_ptr(), int(q_d.dtype == torch.float16), Q, x_d.data_ptr(), int(x_d.dtype == torch.float16), B, D,
                      short_d.data_ptr(), S, None if row_of_d is None else row_of_d.data_ptr(),
                      0 if row_of_d is None else row_of_d.numel(), k, rg.CODE[metric], scores.data_ptr(), pos.data_ptr(),
                      ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return scores, pos


def _same(got, want, what):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    want_s, want_i = want
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gs.shape == gi.shape == want_i.shape, what
    assert np.array_equal(gi, want_i), f"{what}: positions differ from rule 30 in rows {np.flatnonzero((gi != want_i).any(1))[:8]}"
    assert np.array_equal(gs.view(np.uint32), want_s.view(np.uint32)), f"{what}: scores differ from rule 29"
    tail = want_i == -1
    assert (gi[tail] == -1).all() and np.isposinf(gs[tail]).all(), f"{what}: the tail is not (+inf, -1)"
    return int(tail.sum())


def _equal(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize("x", rg.CASES, ids=lambda c: c.name)
def test_case(x):
    q, X, short, row_of = rg.make(x)
    want_s, want_i, _ = rg.restate(q, X, short, x.k, x.metric, row_of)
    q_d, x_d, short_d = _dev(q, x.view), _dev(X, x.view), _dev(short)
    row_d = None if row_of is None else _dev(row_of)
    got = _abi(q_d, x_d, short_d, x.k, x.metric, row_d)
    tail = _same(got, (want_s, want_i), x.name)
    pos, _ = rg.candidates(short, x.B, row_of)
    assert tail == int(np.maximum(x.k - (pos >= 0).sum(1), 0).sum()) if x.S else tail == x.Q * x.k
    assert _equal(got, _abi(q_d, x_d, short_d, x.k, x.metric, row_d)), "a second call differs"
    if x.view:                                                # the vector loads give the same bits as the element-wise ones
        assert _equal(got, _abi(_dev(q), _dev(X), short_d, x.k, x.metric, row_d))


# ------------------------------------------------------------------ hand-made orders
ORDER_Q, ORDER_S, ORDER_D, ORDER_B = 600, 3000, 64, 3200
ORDERS = ("descending", "ascending", "all_equal", "inf_nan")


def _order_inputs(order):
    rs = np.random.RandomState(7)
    X = rs.standard_normal((ORDER_B, ORDER_D)).astype(np.float32)
    q = rs.standard_normal(ORDER_D).astype(np.float32)
    if order == "all_equal":
        X[:] = X[0]
    if order == "inf_nan":
        X[rs.rand(ORDER_B) < 0.3, 5] = 3e38                   # the square overflows: +inf, listed behind every finite score
        X[rs.rand(ORDER_B) < 0.7, 9] = np.nan                 # never listed: about 630 finite scores and 270 +inf remain
        X[7, 3] = np.inf
    s = rg.restate_scores(q, X, "l2")
    by = np.argsort(s, kind="stable")
    by = by[~np.isnan(s[by])] if order != "inf_nan" else rs.permutation(ORDER_B)
    short = by[:ORDER_S][::-1] if order == "descending" else (by[:ORDER_S] if order == "ascending" else rs.permutation(ORDER_B)[:ORDER_S])
    return q, X, np.ascontiguousarray(short.astype(np.int64)), s


@pytest.mark.parametrize("order", ORDERS)
def test_orders_in_one_part(order):
    assert rg.rerank_plan(ORDER_Q, ORDER_S, ORDER_D, 1024).parts == 1
    q, X, short, s = _order_inputs(order)
    if order == "descending":
        d = np.diff(s[short])                                 # every candidate beats the bound when it arrives:
        assert (d <= 0).all() and (np.diff(short)[d == 0] < 0).all()       # a lower score, or the score at a lower position
    if order == "inf_nan":
        ok = s[short]
        assert np.isnan(ok).sum() > 1000 and np.isposinf(ok).sum() > 200 and 100 < np.isfinite(ok).sum() < 1024
    want = {k: rg.restate(q[None, :], X, short[None, :], k, "l2")[:2] for k in (1024, 100)}
    q_d = _dev(np.repeat(q[None, :], ORDER_Q, 0))
    x_d, short_d = _dev(X), _dev(np.repeat(short[None, :], ORDER_Q, 0))
    got = {k: _abi(q_d, x_d, short_d, k, "l2") for k in (1024, 100)}
    for k in (1024, 100):
        _same(got[k], (np.repeat(want[k][0], ORDER_Q, 0), np.repeat(want[k][1], ORDER_Q, 0)), f"{order} k={k}")
    assert _equal((got[1024][0][:, :100], got[1024][1][:, :100]), got[100]), "k = 100 is not the prefix of k = 1,024"
    if order == "all_equal":
        assert np.array_equal(want[1024][1][0], np.sort(short)[:1024])
    if order == "inf_nan":
        assert (want[1024][1][0] == -1).any() and np.isposinf(want[1024][0][0][want[1024][1][0] >= 0]).any()


def test_cosine_zero_row_and_zero_query():
    rs = np.random.RandomState(8)
    X = rs.standard_normal((40, 30)).astype(np.float32)
    X[3] = 0
    q = rs.standard_normal((2, 30)).astype(np.float32)
    q[1] = 0
    short = np.tile(np.arange(40, dtype=np.int64), (2, 1))
    want_s, want_i, _ = rg.restate(q, X, short, 40, "cosine")
    got = _abi(_dev(q), _dev(X), _dev(short), 40, "cosine")
    _same(got, (want_s, want_i), "cosine zeros")
    assert (want_s[1] == 0).all() and np.array_equal(want_i[1], np.arange(40)) and want_s[0][list(want_i[0]).index(3)] == 0
    from quantization_amd import rerank
    val, idx = rerank(_dev(q), _dev(X), _dev(short), 40, metric="cosine")
    val, idx = val.cpu().numpy(), idx.cpu().numpy()
    assert (val[1] == 0).all() and val[0][list(idx[0]).index(3)] == 0 and np.isfinite(val).all()
    x64, q64 = X.astype(np.float64), q.astype(np.float64)
    cos = (x64[idx[0]] @ q64[0]) / np.maximum(np.sqrt((x64[idx[0]] ** 2).sum(1)), 1e-300) / np.sqrt((q64[0] ** 2).sum())
    assert np.abs(val[0] - cos).max() < 1e-5 and (np.diff(val[0]) <= 0).all()


# ------------------------------------------------------------------ launch independence
def test_result_does_not_depend_on_the_launch():
    x = next(c for c in rg.CASES if c.name == "d64_q300_s3000_k1")
    q, X, short, row_of = rg.make(x)
    q_d, x_d, short_d = _dev(q), _dev(X), _dev(short)
    for k in (10, 1024):
        among = _abi(q_d, x_d, short_d, k, "l2")
        assert _equal(among, _abi(q_d, x_d, short_d, k, "l2", _dev(row_of))), "row_of = arange differs from row_of = None"
        for j in (0, 299):                                    # alone: another number of parts
            alone = _abi(q_d[j:j + 1].contiguous(), x_d, short_d[j:j + 1].contiguous(), k, "l2")
            assert _equal(alone, (among[0][j:j + 1], among[1][j:j + 1])), "a query alone differs from the same query among 300"
        assert _equal(among, _abi(q_d, x_d, short_d.flip(1).contiguous(), k, "l2")), "a reversed shortlist row gives another result"
    assert rg.rerank_plan(1, x.S, x.D, 10).parts != rg.rerank_plan(300, x.S, x.D, 10).parts


# ------------------------------------------------------------------ selection
def test_every_cell_of_the_launcher_runs_once():
    rs = np.random.RandomState(9)
    B, D, Q, S, k = 70, 30, 3, 40, 10
    short = rs.randint(-2, B + 2, size=(Q, S)).astype(np.int64)
    cells = 0
    for metric in rg.METRICS:
        for qhalf in (False, True):
            for xhalf in (False, True):
                q = rs.standard_normal((Q, D)).astype(np.float16 if qhalf else np.float32)
                X = rs.standard_normal((B, D)).astype(np.float16 if xhalf else np.float32)
                _same(_abi(_dev(q), _dev(X), _dev(short), k, metric), rg.restate(q, X, short, k, metric)[:2], (metric, qhalf, xhalf))
                cells += 1
    assert cells == 12


# ------------------------------------------------------------------ the public call
def test_public_call():
    from quantization_amd import rerank
    m = _lib()
    rs = np.random.RandomState(10)
    B, D = 300, 20
    X = rs.standard_normal((B, D)).astype(np.float32)
    q = rs.standard_normal((2, 3, D)).astype(np.float16)
    short = rs.randint(-1, B, size=(2, 3, 50)).astype(np.int32)
    short[1, 2] = -1                                          # a row without a candidate
    row_of = rs.permutation(B).astype(np.int64)
    x_d, q_d, s_d, r_d = _dev(X), _dev(q), _dev(short), _dev(row_of)
    for metric in rg.METRICS:
        for ro, ro_d in ((None, None), (row_of, r_d)):
            val, idx = rerank(q_d, x_d, s_d, 60, metric=metric, row_of=ro_d)
            assert tuple(val.shape) == tuple(idx.shape) == (2, 3, 60) and val.dtype == torch.float32 and idx.dtype == torch.int64
            ws, wi, _ = rg.restate(q.reshape(6, D), X, short.reshape(6, 50), 60, metric, ro)
            assert np.array_equal(idx.cpu().numpy().reshape(6, 60), wi)
            v = val.cpu().numpy().reshape(6, 60)
            if metric == "l2":
                assert np.array_equal(v.view(np.uint32), ws.view(np.uint32))
            elif metric == "ip":
                assert np.array_equal(v.view(np.uint32), (-ws).view(np.uint32)) and np.isneginf(v[5]).all()
            else:
                qn = np.sqrt((q.reshape(6, D).astype(np.float32) ** 2).sum(1, keepdims=True))
                # |q| is torch's sum of 20 squares in an order of its own: (20 / 2 + 2) roundings of 2^-24 at most
                assert np.allclose(v[:5], (-ws / qn)[:5], rtol=12 * 2.0 ** -24, atol=0) and np.isneginf(v[5]).all()
            assert (wi[5] == -1).all() and (wi[:5, 50:] == -1).all()
    with pytest.raises(m.McqError):
        rerank(q_d.cpu(), x_d, s_d, 10)
    with pytest.raises(ValueError):
        rerank(q_d, x_d, s_d, 1025)
    with pytest.raises(ValueError):
        rerank(q_d, x_d, s_d, 10, metric="dot")
    # shortlists straight from search_wide, with their -1 tails
    import search_grid as sg
    import test_gpu_search as base
    case = sg.Case("rerank_public", 4, 256, 24, 5, 90, 10)
    quant = base._quantizer(case)
    xs = torch.from_numpy(rs.standard_normal((90, 24)).astype(np.float32)).cuda()
    xq = xs[:5] + 0.01
    with torch.no_grad():
        codes = quant.encode(xs, refine_indexes_iters=2)
    _, wide = quant.search_wide(xq, codes, 100)
    assert tuple(wide.shape) == (5, 100) and bool((wide[:, 90:] == -1).all())
    val, idx = rerank(xq, xs, wide, 10)
    exact = ((xs.cpu().numpy().astype(np.float64)[None] - xq.cpu().numpy().astype(np.float64)[:, None]) ** 2).sum(2)
    assert np.array_equal(idx.cpu().numpy(), np.argsort(exact, axis=1, kind="stable")[:, :10])     # all 90 are in the shortlist
    assert np.array_equal(idx[:, 0].cpu().numpy(), np.arange(5))


# ------------------------------------------------------------------ end to end
def test_end_to_end_after_search_lists_wide():
    """search_lists_wide(k = 300) over the residual store of tests/test_gpu_search_residual.py, then rerank(k = 10, row_of =
    order) against the raw vectors: equal to the restatement, every value within rerank_grid.error_bound of the float64
    distance at its index, and the ten indexes those of the float64 top ten over the shortlist -- the data (that recipe's
    seed, 21) leave a float64 gap between the 10th and the 11th candidate of every query that exceeds twice the bound, which
    is asserted.  recall@10 against the float64 top ten over the whole store is printed, not asserted."""
    import test_gpu_search_residual as res
    from quantization_amd import build_lists, rerank
    quant, xq_d, codes, off, probes, bias, norms, rnorms, exact, bound, cand = res._setup()
    rs = np.random.RandomState(21)                            # the raw vectors of that recipe, drawn again
    cen = (rs.standard_normal((res.NL, res.D)) * 2.0).astype(np.float32)
    member = rs.randint(0, res.NL, size=res.B)
    x = (cen[member] + 0.5 * rs.standard_normal((res.B, res.D))).astype(np.float32)
    xq = (cen[rs.randint(0, res.NL, size=res.Q)] + 0.5 * rs.standard_normal((res.Q, res.D))).astype(np.float32)
    assert np.array_equal(xq, xq_d.cpu().numpy())
    x64, q64, cen64 = x.astype(np.float64), xq.astype(np.float64), cen.astype(np.float64)
    assign = ((x64[:, None, :] - cen64[None]) ** 2).sum(2).argmin(1)
    x_d = torch.from_numpy(x).cuda()
    order, off2 = build_lists(torch.from_numpy(assign).cuda(), res.NL)
    assert torch.equal(off2, off)
    _, short = quant.search_lists_wide(xq_d, codes, off, probes, 300, norms=norms, probe_bias=bias)
    val, idx = rerank(xq_d, x_d, short, 10, row_of=order)
    short_h, order_h = short.cpu().numpy(), order.cpu().numpy()
    want_s, want_i, _ = rg.restate(xq, x, short_h, 10, "l2", order_h)
    _same((val, idx), (want_s, want_i), "end to end")
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    truth = ((q64[:, None, :] - x64[None]) ** 2).sum(2)       # (Q, B) over original rows
    top = np.argsort(truth, axis=1, kind="stable")[:, :10]
    coarse = quant.search_lists_wide(xq_d, codes, off, probes, 10, norms=norms, probe_bias=bias)[1].cpu().numpy()
    hits_before = hits_after = 0
    for j in range(res.Q):
        p = short_h[j][short_h[j] >= 0]
        assert len(p) >= 50 and len(set(p.tolist())) == len(p)
        rows = order_h[p]
        d = truth[j, rows]
        bd = rg.error_bound(xq[j], x[rows], "l2")
        by = np.argsort(d, kind="stable")
        assert d[by[10]] - d[by[9]] > 2 * bd.max(), (j, d[by[10]] - d[by[9]], bd.max())
        assert np.array_equal(np.sort(idx[j]), np.sort(p[by[:10]]))
        at = order_h[idx[j]]
        assert (np.abs(val[j] - truth[j, at]) <= rg.error_bound(xq[j], x[at], "l2")).all()
        hits_before += len(set(order_h[coarse[j][coarse[j] >= 0]].tolist()) & set(top[j].tolist()))
        hits_after += len(set(at.tolist()) & set(top[j].tolist()))
    print(f"[rerank] recall@10 against the float64 top ten over the whole store: {hits_before / (10 * res.Q):.3f} from the codes, "
          f"{hits_after / (10 * res.Q):.3f} after re-ranking a shortlist of 300")
