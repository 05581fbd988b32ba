"""The search over a shortlist (mcq_search_shortlist, mcq_search_shortlist_u16, Quantizer.search_shortlist;
include/mcq_shortlist.h rules 36-39): the numpy restatement on top of the existing ones, the mirror of the launch arithmetic
(short_plan of quantization_amd/csrc/mcq_api.hip and the kShort* constants of mcq_shortlist_kernels.h), and the case table of
tests/test_gpu_search_shortlist.py.  Comparison is bit for bit everywhere; no tolerance.

Nothing about a score or the order is restated here: what an entry names is rerank_grid.candidates (rule 28 = rule 36), the
table sums are search_metric_grid.restate_sums (search_grid.restate_scores, rule 3), the bias addition and the finish are
search_bias_grid.finish on float32 (S + bias) (rule 21 = rule 37), and the selection is search_wide_grid.restate_topk_valid
(rule 26 = rule 38) over the candidates in ascending position, so that its stable order is "(score, position) ascending".

Each case CLAIMS what it reaches (tests/test_search_shortlist_host.py checks the claims against the mirror), so that a moved
constant makes a test fail instead of leaving the GPU cases covering nothing.  A helper module: no tests."""
import os
import re
from dataclasses import dataclass

import numpy as np

import rerank_grid as rg
import search_bias_grid as bg
import search_grid as sg
import search_metric_grid as mg
import search_wide_grid as wg

SHORT_HDR = os.path.join(sg.ROOT, "quantization_amd", "csrc", "mcq_shortlist_kernels.h")
ME = "tests/search_shortlist_grid.py"
NAMES = ("kShortStep", "kShortTargetBlocks")
METRICS = ("l2", "ip", "cosine")
CODE = mg.CODE
ONE_BYTE = ((1, 256), (2, 256), (4, 16), (8, 256), (16, 16), (16, 256), (64, 256))      # every chunk width; 1, 2 and 8 chunks a row
TWO_BYTE = ((1, 1024), (8, 1024), (16, 1024), (32, 512))
CROSS = ((8, 256), (16, 16), (64, 256))                     # (N, K) at which the two-byte entry is held against the one-byte one
NS = (1, 2, 4, 8, 16, 32, 64)                               # launch_short's N values: those of k_search_wide


def constants():
    c = dict(wg.constants())
    with open(SHORT_HDR) as f:
        src = f.read()
    for name in NAMES:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9]+);", src)
        assert m, f"{name} moved out of mcq_shortlist_kernels.h: update {ME}"
        c[name] = int(m.group(1))
    return c


# ------------------------------------------------------------------ short_plan of mcq_api.hip
@dataclass(frozen=True)
class Plan:
    parts: int
    lds: int
    ws_bytes: int
    steps: int


def short_plan(Q, S, N, K, k, c=None):
    """short_plan of mcq_api.hip: the parts per query -- a function of the call's shape alone"""
    c = c or constants()
    half = wg.wide_half(k, c)
    steps = (S + c["kShortStep"] - 1) // c["kShortStep"]
    parts = max(1, min(c["kShortTargetBlocks"] // max(Q, 1), c["kWideMergeEntries"] // half, steps))
    return Plan(parts, ((N * K * 4 + 15) & ~15) + 2 * half * 8 + 64, 2 * sg.align256(Q * parts * k * 4), steps)


def part_steps(T, parts):
    return [(T * p // parts, T * (p + 1) // parts) for p in range(parts)]


# ------------------------------------------------------------------ rules 36-38 in numpy
def slot_scores(Tq, w, codes, rows, bias_at, metric):
    """the scores of one query's candidates: Tq (N, K), rows int64 (C,) into codes and w, bias_at float32 (C,) or None"""
    if len(rows) == 0:
        return np.zeros(0, dtype=np.float32)
    S = mg.restate_sums(Tq[None], codes[rows])[0]
    if bias_at is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            S = (S + np.asarray(bias_at, dtype=np.float32)).astype(np.float32)
    return bg.finish(S, None if w is None else np.asarray(w, dtype=np.float32)[rows], metric)


def restate(T, w, codes, short, k, metric, row_of=None, bias=None):
    """-> (scores float32 (Q, k), positions int64 (Q, k)) as the entries leave them, and the per-slot scores of each row's
    candidates in slot order"""
    Q = T.shape[0]
    pos, row = rg.candidates(short, codes.shape[0], row_of)
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    slots = []
    for q in range(Q):
        at = np.flatnonzero(pos[q] >= 0)
        sc = slot_scores(T[q], w, codes, row[q][at], None if bias is None else bias[q][at], metric)
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
    N: int
    K: int
    Q: int
    S: int
    k: int
    metric: str = "l2"
    B: int = 4099
    short: str = "distinct"          # distinct | pad (-1 in the middle and at the end, a row of -1 only) | junk (B, 2**40, -7, INT64_MIN) | dups
    row_of: str = None               # None | perm | perm_bad (entries outside [0, B), Bs != B) | arange
    bias: str = None                 # None | random (zeros, negatives, one -0.0 among them) | negzero
    # claims (tests/test_search_shortlist_host.py)
    parts: bool = False              # a query has several parts
    one_part: bool = False
    rounds: bool = False             # some part has more steps than the workgroup has waves: more than one round
    short_row: bool = False          # some row has fewer than k candidates
    empty_row: bool = False          # some row has no candidate
    all_enter: bool = False          # every row has at least k candidates
    ragged: bool = False             # the last step of a row is partial

    @property
    def two(self):
        return self.K > 256


CASES = [
    Case("n1_k256_s0_k1", 1, 256, 1, 0, 1, one_part=True, short_row=True, empty_row=True),
    Case("n2_k256_s1_k10", 2, 256, 5, 1, 10, "ip", one_part=True, short_row=True, ragged=True),
    Case("n4_k16_s63_k64", 4, 16, 5, 63, 64, "cosine", short="pad", one_part=True, short_row=True, empty_row=True, ragged=True),
    Case("n8_k256_s64_k64", 8, 256, 1, 64, 64, one_part=True, all_enter=True),
    Case("n16_k16_q70_s65_k65", 16, 16, 70, 65, 65, "ip", row_of="perm", parts=True, all_enter=True, ragged=True),
    Case("n16_k256_s255_k300", 16, 256, 5, 255, 300, "cosine", short="junk", parts=True, short_row=True, ragged=True),
    Case("n64_k256_s256_k10", 64, 256, 1, 256, 10, short="dups", bias="random", parts=True, all_enter=True),
    Case("n8_k256_s257_k1024", 8, 256, 5, 257, 1024, short="junk", row_of="perm_bad", bias="random", parts=True, short_row=True,
         ragged=True),
    Case("n8_k256_q70_s1000_k300", 8, 256, 70, 1000, 300, "ip", bias="random", parts=True, all_enter=True, ragged=True),
    Case("n64_k256_s1000_k1024", 64, 256, 5, 1000, 1024, "cosine", parts=True, short_row=True, ragged=True),
    Case("n8_k256_q600_s1000_k10", 8, 256, 600, 1000, 10, short="pad", one_part=True, rounds=True, short_row=True, empty_row=True,
         ragged=True),
    Case("n2_k256_s1000_k1", 2, 256, 1, 1000, 1, "l2", row_of="arange", bias="negzero", parts=True, all_enter=True, ragged=True),
    Case("n16_k256_q300_s1000_k64", 16, 256, 300, 1000, 64, "l2", row_of="perm", parts=True, rounds=True, all_enter=True, ragged=True),
    Case("w_n1_k1024_s65_k10", 1, 1024, 5, 65, 10, parts=True, all_enter=True, ragged=True),
    Case("w_n8_k1024_s1000_k300", 8, 1024, 1, 1000, 300, "cosine", row_of="perm", bias="random", parts=True, all_enter=True,
         ragged=True),
    Case("w_n16_k1024_s257_k64", 16, 1024, 5, 257, 64, "ip", short="junk", parts=True, all_enter=True, ragged=True),
    Case("w_n32_k512_q70_s256_k65", 32, 512, 70, 256, 65, short="dups", parts=True, all_enter=True),
]


def make(case, seed=3):
    """-> (T float32 (Q, N, K), w float32 (B,), codes uint8 or uint16 (B, N), short int64 (Q, S), row_of int64 or None,
    bias float32 (Q, S) or None): numpy"""
    rs = np.random.RandomState(seed)
    T = rs.standard_normal((case.Q, case.N, case.K)).astype(np.float32)
    codes = rs.randint(0, case.K, size=(case.B, case.N)).astype(np.uint16 if case.two else np.uint8)
    w = (rs.rand(case.B) * 4).astype(np.float32)
    row_of = None
    Bs = case.B
    if case.row_of == "arange":
        row_of = np.arange(case.B, dtype=np.int64)
    elif case.row_of == "perm":
        row_of = rs.permutation(case.B).astype(np.int64)
    elif case.row_of == "perm_bad":                           # Bs != B, and one in sixteen positions names no row
        Bs = case.B + 101
        row_of = rs.randint(0, case.B, size=Bs).astype(np.int64)
        row_of[:case.B] = rs.permutation(case.B)
        bad = rs.rand(Bs) < 1 / 16
        row_of[bad] = rs.choice(np.array([-1, case.B, 2 ** 40, -(2 ** 33)], dtype=np.int64), size=int(bad.sum()))
    short = np.empty((case.Q, case.S), dtype=np.int64)
    for r in range(case.Q):
        short[r] = rs.permutation(Bs)[:case.S] if case.S <= Bs else rs.randint(Bs, size=case.S)
    if case.short == "dups" and case.S > 1:
        short[:, 1::3] = short[:, 0:-1:3][:, :short[:, 1::3].shape[1]]     # every third entry repeats its neighbour
    if case.short == "pad" and case.S > 0:
        short[:, case.S // 2] = -1                            # in the middle
        short[:, -(case.S // 4 + 1):] = -1                    # and the tail, as the searches pad
        short[case.Q // 2] = -1                               # a row of -1 only
    if case.short == "junk" and case.S > 0:
        junk = rs.rand(case.Q, case.S) < 0.2
        junk[0, :4] = True
        vals = np.array([Bs, 2 ** 40, -7, np.iinfo(np.int64).min], dtype=np.int64)
        short[junk] = rs.choice(vals, size=int(junk.sum()))
        short[0, :4] = vals
    bias = None
    if case.bias == "negzero":
        bias = np.full((case.Q, case.S), -0.0, dtype=np.float32)
    elif case.bias == "random" and case.S > 0:
        bias = rs.standard_normal((case.Q, case.S)).astype(np.float32)
        bias[rs.rand(case.Q, case.S) < 0.2] = 0.0
        bias[0, 0] = -0.0
    return T, w, codes, short, row_of, bias


def reach(case, short, row_of, c=None):
    """what a case meets -> dict of the claims"""
    c = c or constants()
    plan = short_plan(case.Q, case.S, case.N, case.K, case.k, c)
    pos, _ = rg.candidates(short, case.B, row_of)
    n = (pos >= 0).sum(1) if case.S else np.zeros(case.Q, dtype=np.int64)
    longest = max(hi - lo for lo, hi in part_steps(plan.steps, plan.parts))
    return dict(parts=plan.parts > 1, one_part=plan.parts == 1, rounds=longest > c["kWideWaves"], short_row=bool((n < case.k).any()),
                empty_row=bool((n == 0).any()), all_enter=bool((n >= case.k).all()), ragged=case.S % c["kShortStep"] != 0)
