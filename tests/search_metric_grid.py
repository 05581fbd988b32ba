"""The inner-product and cosine metrics of the search over stored codes: the numpy restatement of rules 3' and 6 of the contract
(include/mcq.h), beside tests/search_grid.py, which keeps rules 3 and 4 for L2.

    S[q][b]  = ((T[q][0][c_0] + T[q][1][c_1]) + ...) + T[q][N-1][c_{N-1}]      float32 additions in this order (rule 3's sum)
    r[b]     = float32(1) / sqrt(t[b]) in float32, 0 where t[b] == 0            (rule 6; numpy's sqrt and division round correctly)
    score    = S (ip),  float32(S * r[b]) (cosine): ONE multiplication
and the lists are rule 4's: restate_topk of search_grid.  restate_scores of search_grid ends in `+ t`; with t = -0.0 that
addition returns its other operand bit for bit (x + (-0) == x for every x, either zero included), which is how S is had
from it unchanged.

The GPU cases of the two metrics are the L2 table itself (search_grid.CASES): tests/test_search_host.py already checks every
claim of that table (query tiles, slices, partial last step, strided waves, short stores) against the launch arithmetic, and
that arithmetic does not depend on the metric."""
import numpy as np

import search_grid as sg

METRICS = ("ip", "cosine")
CODE = {"l2": 0, "ip": 1, "cosine": 2}          # MCQ_SEARCH_L2 / _IP / _COS
CASES = sg.CASES


def restate_rnorms(t):
    """rule 6 in float32"""
    t = np.asarray(t, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float32(1) / np.sqrt(t, dtype=np.float32)
    return np.where(t == 0, np.float32(0), r).astype(np.float32)


def restate_sums(T, codes):
    """S of rule 3, (Q, B) float32"""
    return sg.restate_scores(T, np.full(codes.shape[0], -0.0, dtype=np.float32), codes)


def restate_metric_scores(T, w, codes, metric):
    if metric == "l2":
        return sg.restate_scores(T, w, codes)
    S = restate_sums(T, codes)
    if metric == "ip":
        return S
    assert metric == "cosine"
    with np.errstate(invalid="ignore", over="ignore"):
        return (S * np.asarray(w, dtype=np.float32)[None, :]).astype(np.float32)


def restate_metric(T, w, codes, k, metric, qchunk=8):
    """rules 3' and 4 for all queries, a few at a time; scores ascend (the tail of a short store is (+inf, -1))"""
    Q = T.shape[0]
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    if codes.shape[0] == 0:
        return out_s, out_i
    for a in range(0, Q, qchunk):
        s = restate_metric_scores(T[a:a + qchunk], w, codes, metric)
        out_s[a:a + qchunk], out_i[a:a + qchunk] = sg.restate_topk(s, k)
    return out_s, out_i


def similarity_bound(qh, C, flat, metric, eps=2.0 ** -24):
    """The derived bound of tests/test_gpu_search_metric_definition.py for every (query, stored vector), with the float64
    values it is a bound on: (exact (Q, B), bound (Q, B)).  qh (Q, D) float32 queries, C (N, K, D) the fp32 centers that
    decode sums, flat (B, N) unpacked codes."""
    N, K, D = C.shape
    q64, C64 = qh.astype(np.float64), C.astype(np.float64)
    dec = np.zeros((flat.shape[0], D))
    for n in range(N):
        dec += C64[n][flat[:, n]]
    exact = q64 @ dec.T
    A_tab = (np.abs(q64) @ np.abs(C64).reshape(N * K, D).T).reshape(len(qh), N, K)     # sum_d |q_d| |C[n][k][d]|
    A = np.zeros_like(exact)
    for n in range(N):
        A += A_tab[:, n, :][:, flat[:, n]]
    bound = (D + N + 2) * eps * A
    if metric == "ip":
        return exact, bound
    assert metric == "cosine"
    qn = np.sqrt((q64 ** 2).sum(1))[:, None]
    xn = np.sqrt((dec ** 2).sum(1))[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = np.where((qn == 0) | (xn == 0), 0.0, exact / (qn * xn))
        bound = np.where((qn == 0) | (xn == 0), 0.0, bound / (qn * xn)) + 3 * eps * np.abs(cos)
    return cos, bound
