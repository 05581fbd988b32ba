"""Inner-product and cosine search against their DEFINITION, in float64 on the host.

The bit-exact tests (tests/test_gpu_search_metric.py) restate the scan from the tables the device formed, so a wrong sign or
a wrong factor in what those tables and sums are taken to MEAN would pass them.  Here the store is decoded and
<q, x^_b> and cos(q, x^_b) = <q, x^_b> / (|q| |x^_b|) are formed in float64 from the fp32 centers that decode sums.

The bound (derived, not measured; eps = 2^-24, the unit round-off of fp32):
  * a table entry T[n][k] = -2 * chain over the D features: D rounded products and D additions in one chain, so its error is at
    most (D + 1) * eps * 2 * sum_d |q_d| |C[n][k][d]| to first order (the pad columns of the chain add exact zeros; * -2 is exact);
  * the score adds N such entries in N - 1 further fp32 additions (+ 1 multiplication for the cosine), each of which at most
    multiplies the magnitude accumulated so far by (1 + eps); * -0.5 is exact.  Together
        |sim_ip - <q, x^_b>|  <=  (D + N + 2) * eps * A_b,      A_b = sum_n sum_d |q_d| |C[n][c_n][d]|;
  * the cosine divides by |q| (fp32, Quantizer.search) and multiplies by r_b = 1 / sqrt(t_b) (two correctly rounded operations):
        |sim_cos - cos|  <=  (D + N + 2) * eps * A_b / (|q| |x^_b|)  +  3 * eps * |cos|.
    The second term is for the roundings of the two norms' last operations; the fp32 chains that FORM t_b and |q|^2 (rule 2: at
    most 2 * (N - 1) + 4 * ceil(D / 256) + 7 roundings, all terms positive, so a relative error of that many eps, halved by the
    root) are not itemised: they scale |cos| <= A_b / (|q| |x^_b|), and the first term bounds the chain of D + N + 1 operations
    by its worst case where a chain of positive and negative terms uses a small fraction of it.
  (a) every returned similarity is within the bound of the float64 value at the returned index;
  (b) the k-th returned float64 value >= the true k-th largest float64 value minus twice the bound (the largest over the
      vectors concerned: the returned ones and the true k best -- a true member the scan left out lost to the k-th returned one
      in fp32, and each of the two is within its own bound of its float64 value);
  (c) signs, with no bound on ranks: a query that IS a decoded stored vector has cosine 1 with itself, and finds its own position
      first or tied with the first; q and -q have tables and sums that are exact negations, so their inner-product lists over a
      whole store of 32 vectors (k = B) are each other's reverse wherever neighbouring scores differ;
  (d) metric="l2" and the call without a metric return identical tensors.
The largest error / bound ratios are printed (run with -s)."""
import numpy as np
import pytest
import torch

import search_grid as sg
import search_metric_grid as mg
import test_gpu_search as base

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24

DEFINITION_CASES = [
    sg.Case("def_trained_8x256_d512", 8, 256, 512, 64, 65536, 10, state="trained"),
    sg.Case("def_packed_16x16_d512", 16, 16, 512, 64, 20_000, 10, packed=True),
]


def _setup(case):
    q = base._quantizer(case)
    kept, flat = base._store(case, q)
    assert kept.shape[0] >= case.B and (kept.shape[1] != case.N) == case.packed
    xq, _ = base._queries(case, q, kept)
    return q, kept, flat, xq, base._centers(q)


@pytest.mark.parametrize("metric", mg.METRICS)
@pytest.mark.parametrize("case", DEFINITION_CASES, ids=lambda c: c.name)
def test_similarities_against_float64(case, metric):
    q, kept, flat, xq, C = _setup(case)
    k, Q, B = case.k, case.Q, case.B
    sim, idx = q.search(xq, kept, k=k, metric=metric)
    sim, idx = sim.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    assert ((idx >= 0) & (idx < B)).all() and all(len(set(row)) == k for row in idx.tolist())
    exact, bound = mg.similarity_bound(xq.float().cpu().numpy(), C, flat, metric, EPS)
    rows = np.arange(Q)[:, None]
    # (a)
    err = np.abs(sim - exact[rows, idx])
    ba = bound[rows, idx]
    ratio_a = float((err / ba).max())
    print(f"[search-metric] {case.name} {metric}: largest |sim - float64| / bound = {ratio_a:.4f} (largest error {err.max():.3e})")
    assert (err <= ba).all(), (metric, float(err.max()), float(ba.min()))
    # (b)
    true_top = np.argsort(-exact, axis=1, kind="stable")[:, :k]
    kth_true = exact[rows, true_top][:, k - 1]
    kth_got = exact[rows, idx][:, k - 1]
    b2 = np.maximum(bound[rows, true_top].max(1), ba.max(1))
    short = kth_true - kth_got
    print(f"[search-metric] {case.name} {metric}: largest (true k-th - returned k-th) / (2 * bound) = {float((short / (2 * b2)).max()):.4f}; "
          f"lists equal to the float64 ranking as sets in {int(sum(set(a) == set(b) for a, b in zip(idx.tolist(), true_top.tolist())))} of {Q} rows")
    assert (kth_got >= kth_true - 2 * b2).all()
    # the returned order is the descending order of the float64 values wherever they differ by more than the two bounds
    ex = exact[rows, idx]
    gap = ex[:, :-1] - ex[:, 1:]
    assert (gap >= -(ba[:, :-1] + ba[:, 1:])).all()
    if metric == "cosine":
        assert (np.abs(sim) <= 1 + bound[rows, idx]).all()


@pytest.mark.parametrize("case", DEFINITION_CASES, ids=lambda c: c.name)
def test_a_stored_vector_has_cosine_one_with_itself(case):
    q, kept, flat, _, C = _setup(case)
    own = torch.arange(0, case.B, case.B // case.Q, device="cuda")[:case.Q] + 5
    xq = q.decode(kept[own])
    sim, idx = q.search(xq, kept, k=case.k, metric="cosine")
    rn = q.code_rnorms(kept)
    tables = q.search_tables(xq)
    flat_d = torch.from_numpy(flat).cuda()
    s, i = q._search_scan(tables, flat_d, rn, case.k, metric="cosine")
    assert torch.equal(i, idx)
    own_h = own.cpu().numpy()
    own_s = torch.from_numpy(np.diagonal(mg.restate_metric_scores(tables.cpu().numpy(), rn.cpu().numpy()[own_h], flat[own_h],
                                                                   "cosine")).copy()).cuda()
    first = (idx[:, 0] == own) | (s[:, 0].view(torch.int32) == own_s.view(torch.int32))
    assert bool(first.all()), (idx[:, 0].tolist(), own.tolist())
    exact, bound = mg.similarity_bound(xq.cpu().numpy(), C, flat[idx[:, 0].cpu().numpy()], "cosine", EPS)
    d = np.abs(sim[:, 0].cpu().numpy().astype(np.float64) - 1.0)
    b = np.diagonal(bound) + np.abs(np.diagonal(exact) - 1.0)       # (the float64 cosine of a vector with itself is 1 to 2^-52)
    print(f"[search-metric] {case.name}: largest |cos(own) - 1| / bound = {float((d / b).max()):.4f}")
    assert (d <= b).all() and (sim[:, 0] > 0.99).all()
    # the inner product with itself is |x^|^2 > 0, and the largest of its row is no smaller
    sip, iip = q.search(xq, kept, k=case.k, metric="ip")
    assert bool((sip[:, 0] > 0).all())


def test_negated_query_reverses_the_inner_product_list():
    case = sg.Case("def_negated", 8, 256, 512, 16, 32, 32, state="trained")
    q, kept, flat, xq, C = _setup(case)
    sp, ip = q.search(xq, kept, k=32, metric="ip")
    sn, inn = q.search(-xq, kept, k=32, metric="ip")
    sp, ip, sn, inn = sp.cpu().numpy(), ip.cpu().numpy(), sn.cpu().numpy(), inn.cpu().numpy()
    assert np.array_equal(np.sort(ip, 1), np.tile(np.arange(32), (16, 1))) and np.array_equal(np.sort(inn, 1), np.sort(ip, 1))
    assert np.array_equal(sp, -sn[:, ::-1])                              # exact negations, value for value
    lone = np.ones_like(sp, dtype=bool)                                  # entries whose score differs from both neighbours'
    lone[:, 1:] &= sp[:, 1:] != sp[:, :-1]
    lone[:, :-1] &= sp[:, :-1] != sp[:, 1:]
    assert lone.sum() >= 16 * 24 and np.array_equal(ip[lone], inn[:, ::-1][lone])
    # the sign itself: the first of +q is the float64 arg-max of <q, x^>, that of -q the arg-min, unless the bound says "tie"
    exact, bound = mg.similarity_bound(xq.cpu().numpy(), C, flat, "ip", EPS)
    rows = np.arange(16)
    assert (exact[rows, ip[:, 0]] >= exact.max(1) - 2 * bound.max(1)).all()
    assert (exact[rows, inn[:, 0]] <= exact.min(1) + 2 * bound.max(1)).all()
    assert (exact.max(1) - exact.min(1) > 4 * bound.max(1)).all()        # ... and the two ends are far apart: the check can fail


def test_l2_with_and_without_the_metric_argument():
    case = DEFINITION_CASES[1]
    q, kept, flat, xq, _ = _setup(case)
    d0, i0 = q.search(xq, kept, k=case.k)
    d1, i1 = q.search(xq, kept, k=case.k, metric="l2")
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(i0, i1)
