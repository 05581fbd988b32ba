"""The exact re-ranking of a shortlist (mcq_rerank, quantization_amd.rerank; include/mcq_rerank.h rules 28-31): the numpy
restatement of rule 29 (the score, vectorised over candidates, the trip loop explicit), the restatement of rules 28 and 30 on
top of search_wide_grid.restate_topk_valid, the mirror of the launch arithmetic (rerank_plan of quantization_amd/csrc/mcq_api.hip
and the kRerank* constants of mcq_rerank_kernels.h), and the case table of tests/test_gpu_rerank.py.

Each case CLAIMS what it reaches (tests/test_rerank_host.py checks the claims against the mirror), so that a moved constant
makes a test fail instead of leaving the GPU cases covering nothing.  A helper module: no tests."""
import os
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_metric_grid as mg
import search_wide_grid as wg

RERANK_HDR = os.path.join(sg.ROOT, "quantization_amd", "csrc", "mcq_rerank_kernels.h")
ME = "tests/rerank_grid.py"
NAMES = ("kRerankWaves", "kRerankGroup", "kRerankRows", "kRerankTrips", "kRerankMaxD", "kRerankTargetBlocks")
METRICS = ("l2", "ip", "cosine")
CODE = mg.CODE
NO_ROW = -1


def constants():
    c = dict(wg.constants())
    with open(RERANK_HDR) as f:
        src = f.read()
    for name in NAMES:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9]+);", src)
        assert m, f"{name} moved out of mcq_rerank_kernels.h: update {ME}"
        c[name] = int(m.group(1))
    return c


# ------------------------------------------------------------------ rerank_plan of mcq_api.hip
@dataclass(frozen=True)
class Plan:
    parts: int
    lds: int
    ws_bytes: int
    steps: int


def query_floats(D, c):
    chunk = 256 * c["kRerankTrips"]
    return (D + chunk - 1) // chunk * chunk


def rerank_plan(Q, S, D, k, c=None):
    """rerank_plan of mcq_api.hip: the parts per query -- a function of the call's shape alone"""
    c = c or constants()
    half = wg.wide_half(k, c)
    steps = (S + c["kRerankGroup"] - 1) // c["kRerankGroup"]
    parts = max(1, min(c["kRerankTargetBlocks"] // max(Q, 1), c["kWideMergeEntries"] // half, steps))
    return Plan(parts, query_floats(D, c) * 4 + 2 * half * 8 + 64, 2 * sg.align256(Q * parts * k * 4), steps)


def part_steps(T, parts):
    return [(T * p // parts, T * (p + 1) // parts) for p in range(parts)]


# ------------------------------------------------------------------ rule 29 in numpy
def lane_terms(D):
    """terms a lane adds at most: 4 ceil(D / 256)"""
    return 4 * ((D + 255) // 256)


def restate_scores(q, X, metric):
    """q (D,), X (C, D), float32 or float16 -> float32 (C,): rule 29's score of every row of X against q, in the ascending
    domain.  Element e belongs to lane (e / 4) % 64; a lane adds its terms in ascending e into one accumulator that starts at
    +0.0 -- trip t, then element j of the lane's group, is that order; the lane sums go through the butterfly."""
    q = np.asarray(q).astype(np.float32)
    X = np.asarray(X).astype(np.float32)
    C, D = X.shape
    lanes = np.arange(64)
    acc = np.zeros((C, 64), dtype=np.float32)
    accx = np.zeros((C, 64), dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for t in range((D + 255) // 256):
            for j in range(4):
                e = t * 256 + lanes * 4 + j
                on = lanes[e < D]                             # the lanes that have this element
                if len(on) == 0:
                    continue
                qe, xe = q[e[on]][None, :], X[:, e[on]]
                if metric == "l2":
                    d = qe - xe
                    acc[:, on] = acc[:, on] + d * d
                else:
                    acc[:, on] = acc[:, on] + qe * xe
                    if metric == "cosine":
                        accx[:, on] = accx[:, on] + xe * xe
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[:, lanes ^ m]
            accx = accx + accx[:, lanes ^ m]
        s = acc[:, 0]
        if metric == "ip":
            s = -s
        elif metric == "cosine":
            s = -(s * mg.restate_rnorms(accx[:, 0]))
    return s.astype(np.float32)


def error_bound(q, X, metric):
    """|restate_scores - the float64 value| <= this, float64 (C,).  u = 2^-24.  A lane adds at most n = 4 ceil(D / 256) terms
    and the butterfly 6 more levels, so a term passes through at most n + 5 additions (the first addition, to +0.0, is exact
    but is counted), each a factor (1 + d), |d| <= u.  A term itself carries 1 rounding under ip (the product) and 3 under
    l2 (the difference, squared: two factors, and the product).  So |sum - exact| <= ((1 + u)^(n + 5 + r) - 1) * sum |term|
    with r = 1 or 3, which gamma(n + 8) = (n + 8) u / (1 - (n + 8) u) bounds.  Cosine: dot and xx each as ip, then r = 1 /
    sqrt(xx) with two roundings on a value whose relative error is gamma(n + 8) (the root halves it), and one product: the
    relative factors multiply to at most (1 + gamma(n + 8))^2 (1 + u)^3 on |q||x| >= |dot|, bounded by 2.5 gamma(n + 8) +
    4 u times sum |q_e x_e| / |x| plus the same share of |x| through xx -- taken as (3 gamma(n + 8) + 4 u) * |q|_abs.|x|_abs /
    |x|.  Denormal terms add at most 2^-149 each: D * 2^-149.  Finite inputs without overflow only."""
    q = np.asarray(q).astype(np.float64)
    X = np.asarray(X).astype(np.float64)
    D = X.shape[1]
    u = 2.0 ** -24
    n = lane_terms(D) + 8
    gamma = n * u / (1 - n * u)
    tiny = D * 2.0 ** -149
    if metric == "l2":
        return gamma * ((q[None, :] - X) ** 2).sum(1) + tiny
    mag = (np.abs(q)[None, :] * np.abs(X)).sum(1)
    if metric == "ip":
        return gamma * mag + tiny
    xn = np.sqrt((X ** 2).sum(1))
    return (3 * gamma + 4 * u) * mag / np.where(xn == 0, 1.0, xn) + tiny


def exact_scores(q, X, metric):
    """the float64 value of rule 29's score (ascending domain)"""
    q = np.asarray(q).astype(np.float64)
    X = np.asarray(X).astype(np.float64)
    if metric == "l2":
        return ((q[None, :] - X) ** 2).sum(1)
    dot = X @ q
    if metric == "ip":
        return -dot
    xn = np.sqrt((X ** 2).sum(1))
    return -np.where(xn == 0, 0.0, dot / np.where(xn == 0, 1.0, xn))


# ------------------------------------------------------------------ rules 28 and 30 in numpy
def candidates(short, B, row_of=None):
    """short (Q, S) integer -> (pos (Q, S) int64, row (Q, S) int64): rule 28; NO_ROW where an entry names no candidate"""
    short = np.asarray(short).astype(np.int64)
    Bs = B if row_of is None else len(row_of)
    ok = (short >= 0) & (short < Bs)
    row = np.where(ok, short, 0)
    if row_of is not None and Bs > 0:
        row = np.asarray(row_of, dtype=np.int64)[row]
        ok &= (row >= 0) & (row < B)
    return np.where(ok, short, NO_ROW), np.where(ok, row, NO_ROW)


def restate(queries, vectors, short, k, metric, row_of=None):
    """rules 28-30 -> (scores float32 (Q, k), positions int64 (Q, k)) as mcq_rerank leaves them; also the per-slot scores
    (list of float32 arrays over the candidates of each row, in slot order) for the tests that look at them"""
    Q, S = short.shape
    pos, row = candidates(short, vectors.shape[0], row_of)
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    slots = []
    for q in range(Q):
        at = np.flatnonzero(pos[q] >= 0)
        sc = restate_scores(queries[q], vectors[row[q][at]], metric) if len(at) else np.zeros(0, dtype=np.float32)
        slots.append(sc)
        if len(at) == 0:                                      # no candidate: the fill
            continue
        order = np.argsort(pos[q][at], kind="stable")         # columns in ascending position: restate_topk_valid's tie rule
        ts, ti = wg.restate_topk_valid(np.ascontiguousarray(sc[order][None, :]), k)
        out_s[q] = ts[0]
        out_i[q] = np.where(ti[0] >= 0, pos[q][at][order][np.maximum(ti[0], 0)], -1)
    return out_s, out_i, slots


# ------------------------------------------------------------------ the GPU cases
@dataclass(frozen=True)
class Case:
    name: str
    D: int
    Q: int
    S: int
    k: int
    metric: str = "l2"
    qhalf: bool = False
    xhalf: bool = False
    B: int = 4099
    short: str = "distinct"          # distinct | pad (-1 in the middle and at the end, a row of -1 only) | junk (B, 2**40, -7) | dups
    row_of: str = None               # None | perm | perm_bad (entries outside [0, B)) | arange
    view: bool = False               # queries and vectors are views one element into their storage
    # claims (tests/test_rerank_host.py)
    parts: bool = False              # a query has several parts
    one_part: bool = False
    short_row: bool = False          # some row has fewer than k candidates
    empty_row: bool = False          # some row has no candidate
    all_enter: bool = False          # every row has at least k candidates
    elementwise: bool = False        # the element-wise loads run (D % 4 != 0, or a misaligned base)
    chunks: bool = False             # a row takes more than one chunk of loads
    ragged: bool = False             # the last group of a row is partial


CASES = [
    Case("d1_s0_k1", 1, 1, 0, 1, one_part=True, short_row=True, empty_row=True, elementwise=True),
    Case("d3_s1_k10", 3, 17, 1, 10, "ip", True, False, one_part=True, short_row=True, elementwise=True, ragged=True),
    Case("d4_s63_k64", 4, 17, 63, 64, "cosine", False, True, parts=True, short_row=True, ragged=True),
    Case("d30_s64_k64", 30, 1, 64, 64, "l2", True, True, parts=True, all_enter=True, elementwise=True),
    Case("d64_q300_s65_k64", 64, 300, 65, 64, "l2", row_of="perm", parts=True, all_enter=True, ragged=True),
    Case("d252_s99_k100", 252, 17, 99, 100, "ip", short="pad", parts=True, short_row=True, empty_row=True, ragged=True),
    Case("d256_s100_k100", 256, 17, 100, 100, "cosine", True, True, short="dups", parts=True, all_enter=True, ragged=True),
    Case("d260_s101_k100", 260, 1, 101, 100, "l2", False, True, short="junk", row_of="perm_bad", parts=True, short_row=True,
         ragged=True),
    Case("d512_s1024_k1024", 512, 17, 1024, 1024, "l2", row_of="perm", parts=True, all_enter=True),
    Case("d512_s1025_k1024", 512, 1, 1025, 1024, "ip", True, False, parts=True, all_enter=True, ragged=True),
    Case("d512_s1023_k1024", 512, 1, 1023, 1024, "cosine", parts=True, short_row=True, ragged=True),
    Case("d1000_s3000_k10", 1000, 17, 3000, 10, "l2", short="junk", row_of="perm_bad", parts=True, all_enter=True, chunks=True,
         ragged=True),
    Case("d64_q300_s3000_k1", 64, 300, 3000, 1, "ip", False, True, row_of="arange", parts=True, all_enter=True, ragged=True),
    Case("d16384_s65_k65", 16384, 1, 65, 65, "cosine", True, False, B=100, short="dups", parts=True, all_enter=True, chunks=True,
         ragged=True),
    Case("d512_view_f32", 512, 17, 65, 10, "l2", view=True, parts=True, all_enter=True, elementwise=True, ragged=True),
    Case("d1000_view_f16", 1000, 17, 65, 65, "ip", True, True, view=True, parts=True, all_enter=True, elementwise=True, chunks=True,
         ragged=True),
    Case("d30_q600_s40_k10", 30, 600, 40, 10, "l2", short="pad", one_part=True, short_row=True, empty_row=True, elementwise=True,
         ragged=True),
]


def make(case, seed=3):
    """-> (queries (Q, D), vectors (B, D), short int64 (Q, S), row_of int64 or None): numpy, in the case's dtypes"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal((case.B, case.D)).astype(np.float16 if case.xhalf else np.float32)
    q = rs.standard_normal((case.Q, case.D)).astype(np.float16 if case.qhalf else np.float32)
    row_of = None
    Bs = case.B
    if case.row_of == "arange":
        row_of = np.arange(case.B, dtype=np.int64)
    elif case.row_of in ("perm", "perm_bad"):
        row_of = rs.permutation(case.B).astype(np.int64)
        if case.row_of == "perm_bad":                         # one in sixteen positions names no row
            bad = rs.rand(case.B) < 1 / 16
            row_of[bad] = rs.choice(np.array([-1, case.B, 2 ** 40, -(2 ** 33)], dtype=np.int64), size=int(bad.sum()))
    short = np.empty((case.Q, case.S), dtype=np.int64)
    for r in range(case.Q):
        if case.S <= Bs:
            short[r] = rs.permutation(Bs)[:case.S]
        else:
            short[r] = rs.randint(Bs, size=case.S)
    if case.short == "dups" and case.S > 1:
        short[:, 1::3] = short[:, 0:-1:3][:, :short[:, 1::3].shape[1]]     # every third entry repeats its neighbour
    if case.short == "pad" and case.S > 0:
        short[:, case.S // 2] = -1                            # in the middle
        short[:, -(case.S // 4 + 1):] = -1                    # and the tail, as the searches pad
        short[case.Q // 2] = -1                               # a row of -1 only
    if case.short == "junk" and case.S > 0:
        junk = rs.rand(case.Q, case.S) < 0.2
        short[junk] = rs.choice(np.array([Bs, 2 ** 40, -7, -1], dtype=np.int64), size=int(junk.sum()))
    return q, x, short, row_of


def reach(case, short, row_of, c=None):
    """what a case meets -> dict of the claims"""
    c = c or constants()
    plan = rerank_plan(case.Q, case.S, case.D, case.k, c)
    pos, _ = candidates(short, case.B, row_of)
    n = (pos >= 0).sum(1) if case.S else np.zeros(case.Q, dtype=np.int64)
    el = 2 if case.xhalf else 4
    return dict(parts=plan.parts > 1, one_part=plan.parts == 1, short_row=bool((n < case.k).any()), empty_row=bool((n == 0).any()),
                all_enter=bool((n >= case.k).all()), elementwise=case.D % 4 != 0 or case.view,
                chunks=query_floats(case.D, c) > 256 * c["kRerankTrips"], ragged=case.S % c["kRerankGroup"] != 0)
