"""An inverted file over RESIDUAL codes, end to end on the GPU (quantization_amd.ivf's recipe; include/mcq_residual.h rules 21-23):
vector b of list l is kept as the code of x_b - c_l, searched with probe_bias = -2 <q, c_l> and the norms of c_l + decode(code).

Setup: dim 24, 16 coarse centroids drawn once, 4,000 clustered vectors, Quantizer(24, 256, 4) in the synthetic state of the
search tests; the residuals are encoded and ordered with build_lists; 17 queries, 4 probes each, k = 10, three metrics.

Expectations, with no tolerance list: x^_b = c_l + decode(code_b) in float64 from the fp32 centroids and centers; the exact
distance / inner product / cosine of a query to every candidate of its probed lists; and a DERIVED bound per (query,
candidate), first-order fp32 rounding of every chain with absolute values (the form of search_metric_grid.similarity_bound,
extended by the bias and the base).  With eps = 2^-24, A_r = sum_n sum_d |q_d| |C[n][code_n][d]|, A_c = sum_d |q_d| |c_l[d]|,
M = sum_d (|c_l[d]| + sum_n |C[n][code_n][d]|)^2 and t = |x^|^2:
    the table sum S          2 (D + N + 2) eps A_r      similarity_bound's: D products and D additions per entry, N - 1 sums
    the bias                 2 (D + 1) eps A_c          D rounded products, D - 1 additions in any order (a matmul)
    S + bias                 eps 2 (A_r + A_c)          one addition
  E_sb = 2 eps ((D + N + 3) A_r + (D + 2) A_c)          on -2 <q, x^>;    inner product: E_ip = E_sb / 2 (halving is exact)
    the norm t               E_t = 4 L eps M,  L = max(N, the lane chain of search_grid.norms_chains): test_gpu_search's form,
                             the row chain one longer for the base
    l2: (S + bias) + t, then + |q|^2:   E_l2 = E_sb + E_t + 2 eps (2 (A_r + A_c) + M) + (D + 2) eps |q|^2 + eps |q|^2
    cosine: sqrt and division of rule 6 (2 eps, and half the relative error of t), one product, then / |q| (its sum of D
            squares, a root, a division):   E_cos = E_ip / (|q| |x^|) + |cos| (E_t / (2 t) + ((D + 1) / 2 + 5) eps)
Every returned value lies within the bound of the exact value AT ITS RETURNED INDEX, and that exact value within twice the
query's largest bound of the true j-th best (order statistics of two sequences that differ by at most E differ by at most E).
The range search runs at a radius between the 5th and 6th exact neighbour of the query whose gap is widest in units of its
bound -- wider than twice the bound is asserted -- and must return exactly those five."""
import numpy as np
import pytest
import torch

import search_grid as sg
import test_gpu_search as base

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
D, NL, B, Q, NPROBE, KTOP = 24, 16, 4000, 17, 4, 10
N, K = 4, 256
_STATE = {}


def _setup():
    if _STATE:
        return _STATE["v"]
    from quantization_amd import build_lists, list_assign, probe_bias, probe_lists
    case = sg.Case("residual_4x256_d24", N, K, D, Q, B, KTOP)
    q = base._quantizer(case)
    rs = np.random.RandomState(21)
    cen = (rs.standard_normal((NL, D)) * 2.0).astype(np.float32)
    member = rs.randint(0, NL, size=B)
    x = (cen[member] + 0.5 * rs.standard_normal((B, D))).astype(np.float32)
    xq = (cen[rs.randint(0, NL, size=Q)] + 0.5 * rs.standard_normal((Q, D))).astype(np.float32)
    d2 = ((x.astype(np.float64)[:, None, :] - cen.astype(np.float64)[None]) ** 2).sum(2)
    assign = d2.argmin(1)                                               # the nearest centroid: the coarse cell of a vector
    cen_d, x_d, xq_d = torch.from_numpy(cen).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(xq).cuda()
    assign_d = torch.from_numpy(assign).cuda()
    with torch.no_grad():
        codes = q.encode(x_d - cen_d[assign_d], refine_indexes_iters=2)
    order, off = build_lists(assign_d, NL)
    codes = codes[order].contiguous()
    of = list_assign(off, B)
    assert torch.equal(of.long(), assign_d[order])
    norms = q.code_norms(codes, base=cen_d, assign=of)
    rnorms = q.code_rnorms(codes, base=cen_d, assign=of)
    probes = probe_lists(xq_d, cen_d, NPROBE)
    bias = probe_bias(xq_d, cen_d, probes)
    # float64: x^ = c_l + decode(code), from the fp32 centroids and the fp32 centers that decode sums
    C = base._centers(q)
    flat = codes.cpu().numpy()
    l_of = of.cpu().numpy().astype(np.int64)
    q64, C64, cen64 = xq.astype(np.float64), C.astype(np.float64), cen.astype(np.float64)
    xhat = cen64[l_of] + base._decode64(C, flat)
    mag = np.abs(cen64)[l_of]
    A_r = np.zeros((Q, B))
    for n in range(N):
        mag = mag + np.abs(C64[n])[flat[:, n]]
        A_r += (np.abs(q64) @ np.abs(C64[n]).T)[:, flat[:, n]]
    A_c = (np.abs(q64) @ np.abs(cen64).T)[:, l_of]
    M = (mag ** 2).sum(1)[None, :]
    t = (xhat ** 2).sum(1)[None, :]
    qq = (q64 ** 2).sum(1)[:, None]
    chain = max(N, sg.norms_chains(N, D)[1])
    E_sb = 2 * EPS * ((D + N + 3) * A_r + (D + 2) * A_c)
    E_t = 4 * chain * EPS * M
    ip = q64 @ xhat.T
    cos = ip / np.sqrt(qq * t)
    exact = {"l2": ((q64[:, None, :] - xhat[None]) ** 2).sum(2), "ip": ip, "cosine": cos}
    bound = {"l2": E_sb + E_t + 2 * EPS * (2 * (A_r + A_c) + M) + (D + 3) * EPS * qq,
             "ip": E_sb / 2,
             "cosine": E_sb / 2 / np.sqrt(qq * t) + np.abs(cos) * (E_t / (2 * t) + ((D + 1) / 2 + 5) * EPS)}
    off_h, probes_h = off.cpu().numpy(), probes.cpu().numpy()
    cand = [np.concatenate([np.arange(off_h[l], off_h[l + 1]) for l in row]) for row in probes_h]
    assert all(len(c) > 50 for c in cand) and (t > 0).all()
    _STATE["v"] = (q, xq_d, codes, off, probes, bias, norms, rnorms, exact, bound, cand)
    return _STATE["v"]


@pytest.mark.parametrize("metric", ("l2", "ip", "cosine"))
def test_residual_search_against_float64(metric):
    q, xq_d, codes, off, probes, bias, norms, rnorms, exact, bound, cand = _setup()
    val, idx = q.search_lists(xq_d, codes, off, probes, k=KTOP, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias)
    assert tuple(val.shape) == tuple(idx.shape) == (Q, KTOP) and bool((idx >= 0).all())
    val, idx = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    ex, bd = exact[metric], bound[metric]
    sign = 1.0 if metric == "l2" else -1.0                               # similarities: largest first
    worst = worst_rank = 0.0
    for j in range(Q):
        c = cand[j]
        assert np.isin(idx[j], c).all(), (j, "a position outside the probed lists")
        assert len(set(idx[j].tolist())) == KTOP
        err = np.abs(val[j] - ex[j, idx[j]])
        assert (err <= bd[j, idx[j]]).all(), (j, err.max(), bd[j, idx[j]].min())
        worst = max(worst, float((err / bd[j, idx[j]]).max()))
        best = sign * np.sort(sign * ex[j, c])[:KTOP]                    # the true j-th best among the candidates, float64
        E = float(bd[j, c].max())
        off_rank = np.abs(ex[j, idx[j]] - best)
        assert (off_rank <= 2 * E).all(), (j, off_rank.max(), E)
        worst_rank = max(worst_rank, float(off_rank.max() / (2 * E)))
    print(f"[residual] {metric}: largest error / bound {worst:.4f}, largest rank displacement / (2 x bound) {worst_rank:.4f}")
    # the bias and the based norms are what makes it so: without them the values are those of the residuals alone
    p_val, p_idx = q.search_lists(xq_d, codes, off, probes, k=KTOP, metric=metric)
    p_val, p_idx = p_val.cpu().numpy().astype(np.float64), p_idx.cpu().numpy()
    rows = np.arange(Q)[:, None]
    assert (np.abs(p_val - ex[rows, p_idx]) > bd[rows, p_idx]).any()


@pytest.mark.parametrize("metric", ("l2", "ip", "cosine"))
def test_residual_range_search_returns_exactly_the_five_nearest(metric):
    q, xq_d, codes, off, probes, bias, norms, rnorms, exact, bound, cand = _setup()
    ex, bd = exact[metric], bound[metric]
    sign = 1.0 if metric == "l2" else -1.0
    pick = None
    for j in range(Q):                                                   # the query whose 5th and 6th neighbours lie widest apart
        c = cand[j]
        by = c[np.argsort(sign * ex[j, c], kind="stable")]
        gap = abs(ex[j, by[5]] - ex[j, by[4]])
        E = float(bd[j, c].max())
        if pick is None or gap / E > pick[0]:
            pick = (gap / E, j, by[:5], 0.5 * (ex[j, by[4]] + ex[j, by[5]]))
    ratio, j, five, radius = pick
    assert ratio > 2, "no query has its 5th and 6th neighbours more than twice the bound apart"
    lims, val, idx = q.range_search_lists(xq_d[j:j + 1], codes, off, probes[j:j + 1], float(radius), norms=norms, metric=metric,
                                          rnorms=rnorms, probe_bias=bias[j:j + 1])
    assert lims.tolist() == [0, 5]
    assert sorted(idx.tolist()) == sorted(five.tolist())
    got = val.cpu().numpy().astype(np.float64)
    assert (np.abs(got - ex[j, idx.cpu().numpy()]) <= bd[j, idx.cpu().numpy()]).all()
    print(f"[residual] {metric}: range search of query {j}, gap / bound {ratio:.1f}")
