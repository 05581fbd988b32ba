"""The top-k search past 64 neighbours (mcq_search_wide, mcq_search_wide_lists, Quantizer.search_wide / search_lists_wide;
include/mcq_wide.h rules 24-27): the mirror of its launch arithmetic (wide_plan of quantization_amd/csrc/mcq_api.hip, the
kWide* constants and wide_half / wide_lds_bytes of mcq_wide_kernels.h), the restatement of rule 26 on top of the existing ones,
the case table of tests/test_gpu_search_wide.py and its hand-made orders.

Nothing about a score is restated here: scores are search_metric_grid.restate_metric_scores (rules 3 and 3') and
search_bias_grid.biased_scores (rule 21), the selection is search_grid.restate_topk (rule 4) through
search_mask_grid.restate_topk_masked and search_lists_grid.restate_lists.  The one addition is restate_topk_valid, which drops
NaN scores (rule 26: never listed) before the selection, as restate_topk itself has no answer for them.

Each case CLAIMS what it reaches in the kernels (tests/test_search_wide_host.py checks the claims against the mirror), so that
a moved constant makes a test fail instead of leaving the GPU cases covering nothing."""
import os
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_selection_grid as sel

WIDE_HDR = os.path.join(sg.ROOT, "quantization_amd", "csrc", "mcq_wide_kernels.h")
ME = "tests/search_wide_grid.py"
NAMES = ("kWideWaves", "kWideMaxK", "kWideMergeEntries")
METRICS = lg.METRICS
KS = (1, 10, 64, 65, 128, 129, 256, 257, 1000, 1024)      # both sides of the old cap and of every size of the list
MASKS = (None, "half", "sparse", "none", "one_last")      # patterns of tests/search_mask_grid.py
SEED = 1


def constants():
    c = dict(lg.constants())
    with open(WIDE_HDR) as f:
        src = f.read()
    for name in NAMES:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9]+);", src)
        assert m, f"{name} moved out of mcq_wide_kernels.h: update {ME}"
        c[name] = int(m.group(1))
    m = re.search(r"wide_half\(int k\)\s*\{\s*return k <= ([0-9]+) \? ([0-9]+) : ([0-9]+);", src)
    assert m and m.group(1) == m.group(2), f"wide_half of mcq_wide_kernels.h changed: update {ME}"
    c["half_small"], c["half_large"] = int(m.group(2)), int(m.group(3))
    return c


def wide_half(k, c):
    return c["half_small"] if k <= c["half_small"] else c["half_large"]


@dataclass(frozen=True)
class Plan:
    parts: int
    lds: int
    ws_bytes: int
    half: int


def wide_plan(Q, P, N, K, k, c=None):
    """wide_plan of mcq_api.hip: the parts per query (those of lists_plan, capped by what the merge streams) -- a function of
    the call's shape alone; P is 1 for a call over the whole store"""
    c = c or constants()
    half = wide_half(k, c)
    parts = min(lg.lists_plan(Q, P, N, K, k, c).parts, c["kWideMergeEntries"] // half)
    lds = ((lg.lists_plan(Q, P, N, K, k, c).lds + 15) & ~15) + 2 * half * 8 + 64
    return Plan(parts, lds, 2 * sg.align256(Q * parts * k * 4), half)


def wide_pick_lists(path=sel.API):
    """the value lists of launch_wide, read as search_selection_grid.pick_lists reads its launchers': (metrics, N); one flag"""
    with open(path) as f:
        src = f.read()
    m = re.search(r"^int\s+launch_wide\s*\(", src, re.M)
    assert m, f"launch_wide moved out of mcq_api.hip or was renamed: update {ME}"
    body = src[m.end():src.find("\n}\n", m.end())]
    lists = re.findall(r"\bpick<([^<>]*)>\s*\(", body)
    assert len(lists) == 2 and len(re.findall(r"\bpick_bool\s*\(", body)) == 1, f"launch_wide no longer selects (metric, N) and one flag: update {ME}"
    assert [t.strip() for t in lists[0].split(",")] == ["kMetricL2", "kMetricIP", "kMetricCos"]
    return tuple(int(t) for t in lists[1].split(","))


# ------------------------------------------------------------------ rule 26 in numpy
def restate_topk_valid(s, k, keep=None):
    """s (Q, B) float32 -> (scores (Q, k), positions (Q, k)): rule 4 over the positions whose score is no NaN (and, with
    keep bool (B,), that the mask keeps); the tail is (+inf, -1)"""
    Q = s.shape[0]
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        ok = ~np.isnan(s[q])
        if keep is not None:
            ok &= keep
        pos = np.flatnonzero(ok)
        ts, ti = sg.restate_topk(np.ascontiguousarray(s[q:q + 1, pos]), k)
        out_s[q], out_i[q] = ts[0], kg.map_back(ti, pos)[0]
    return out_s, out_i


# ------------------------------------------------------------------ what a call reaches
def reach(B, plan, k, c, keep=None):
    """what a call over the whole store of B vectors meets -> dict: `parts` -- a query has several parts with a step;
    `empty_part` -- a part without a step beside one with a step; `partial` -- the last step has fewer than 64 candidates;
    `short` -- fewer than k candidates; `flush` -- some part offers more candidates than the 2 half - k pending entries take
    (so a hostile order flushes inside the loop); `merge_flush` -- the merge streams more entries than its pending ones take"""
    T = (B + 63) // 64
    steps = [hi - lo for lo, hi in lg.part_steps(T, plan.parts)]
    n = B if keep is None else int(keep.sum())
    return dict(parts=sum(1 for x in steps if x) > 1, empty_part=T > 0 and any(x == 0 for x in steps), partial=B % 64 != 0,
                short=n < k, flush=max(steps) * 64 > 2 * plan.half - k, merge_flush=plan.parts * k > 2 * plan.half - k)


# ------------------------------------------------------------------ the GPU cases over the whole store
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    K: int
    Q: int
    B: int
    k: int
    D: int = 24
    # claims (tests/test_search_wide_host.py)
    parts: bool = False
    empty_part: bool = False
    partial: bool = False
    short: bool = False
    flush: bool = False
    merge_flush: bool = False
    one_part: bool = False           # the plan gives a single part (a large Q)

    def case(self):
        """the case of tests/search_grid.py whose machinery makes the inputs: a decode-only state and random codes"""
        return sg.Case(self.name, self.N, self.K, self.D, self.Q, self.B, self.k, state="decode_only", codes="random")


CASES = [
    Case("n1_k16_b0_k1", 1, 16, 1, 0, 1, short=True),
    Case("n2_k256_b9_k10", 2, 256, 17, 9, 10, partial=True, short=True, empty_part=True),                    # B = k - 1
    Case("n8_k256_q200_b4099_k64", 8, 256, 200, 4099, 64, parts=True, partial=True),
    Case("n8_k256_b100003_k65", 8, 256, 17, 100_003, 65, parts=True, partial=True, flush=True, merge_flush=True),
    Case("n64_k16_b128_k128", 64, 16, 1, 128, 128, parts=True, empty_part=True, merge_flush=True),            # B = k
    Case("n64_k256_b130_k129", 64, 256, 17, 130, 129, parts=True, partial=True, empty_part=True, merge_flush=True),   # B = k + 1
    Case("n16_k16_b63_k256", 16, 16, 1, 63, 256, partial=True, short=True, empty_part=True, merge_flush=True),
    Case("n2_k256_b64_k257", 2, 256, 17, 64, 257, short=True, empty_part=True, merge_flush=True),
    Case("n8_k256_q1_b100003_k1000", 8, 256, 1, 100_003, 1000, parts=True, partial=True, flush=True, merge_flush=True),
    Case("n8_k256_b4099_k1024", 8, 256, 17, 4099, 1024, parts=True, partial=True, merge_flush=True),
    Case("n8_k256_q600_b300_k100", 8, 256, 600, 300, 100, partial=True, one_part=True),
    Case("n64_k256_q1_b4099_k1024", 64, 256, 1, 4099, 1024, parts=True, partial=True, merge_flush=True),
    Case("n1_k16_q200_b1025_k1024", 1, 16, 200, 1025, 1024, parts=True, partial=True, merge_flush=True),      # B = k + 1
]


# ------------------------------------------------------------------ hand-made orders
# One codebook of 16 entries, every table entry -0.0 and the metric L2: the score of position b is (-0.0 + -0.0) + w[b], the
# bits of w[b] for every w[b], either zero included.  Q queries so that the plan gives few parts of many candidates.
ORDER_N, ORDER_K, ORDER_B, ORDER_Q = 1, 16, 20_000, 300
ORDER_KS = (1024, 100)
ORDERS = ("descending", "ascending", "all_equal", "zeros", "inf", "nan", "nan_short")


def order_w(order, B=ORDER_B):
    """the per-candidate array of a hand-made order, float32 (B,)"""
    rs = np.random.RandomState(5)
    if order == "descending":                               # every candidate enters: the flush runs throughout
        return np.arange(B, 0, -1).astype(np.float32)
    if order == "ascending":
        return np.arange(B).astype(np.float32)
    if order == "all_equal":                                # positions 0 .. k - 1
        return np.full(B, -0.0, dtype=np.float32)
    if order == "zeros":                                    # -0.0 and +0.0 are ONE score: positions 0 .. k - 1, bits kept
        return np.where(rs.rand(B) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    w = rs.standard_normal(B).astype(np.float32)
    if order == "inf":                                      # +inf behind every finite score, -inf before
        w[rs.rand(B) < 0.97] = np.inf
        w[rs.randint(B, size=5)] = -np.inf
        return w
    if order == "nan":                                      # never listed
        w[rs.rand(B) < 0.5] = np.nan
        return w
    assert order == "nan_short"                             # 500 scores remain: a short tail at k = 1,024, none at k = 100
    w[:] = np.nan
    at = rs.permutation(B)[:500]
    w[at] = rs.standard_normal(500).astype(np.float32)
    return w


def dup16_case():
    return sg.Case("wide_dup16", 8, 256, 24, 17, ORDER_B, 1024, state="decode_only", codes="dup16")


# ------------------------------------------------------------------ the lists
LISTS_KS = (300, 1024)
BIG = lg.Case("n64_k256_ones_p4096_k1024", 64, 256, 24, 1, 6144, 1024, 4096, "ones", state="decode_only", codes="random",
              covering=True)
