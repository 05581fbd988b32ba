"""The range search over stored codes: the numpy restatement of rules 7 and 8 of the contract (include/mcq.h), built on the
scores of tests/search_grid.py (rule 3) and tests/search_metric_grid.py (rule 3'); a host mirror of the launch arithmetic of
the two sweeps (range_plan in quantization_amd/csrc/mcq_api.hip, the constants of mcq_range_kernels.h and of
mcq_search_kernels.h); and the case table of tests/test_gpu_search_range.py.

    listed(q, b)  iff  score[q][b] <= thr[q]          one float32 comparison, inclusive; a NaN on either side lists nothing
    lims[0] = 0,  lims[q+1] - lims[q] = #listed(q),   entries of q in ascending b as (score float32, position int64)

The constants are read from the source, and each case CLAIMS what it reaches; tests/test_search_range_host.py checks the claims
on the CPU -- against the mirror for the launch shape, against the restatement on grid-valued tables for the shape of the
result -- so that a moved constant makes a test fail instead of leaving the GPU cases covering nothing.

The thresholds of a case are a function of its scores (thresholds_for): query q takes, by q mod 4,
    0  the score of rank min(B, 10) exactly                (inclusivity: a threshold equal to a score that occurs, ties included)
    1  -inf                                                (an empty result)
    2  +inf                                                (every stored vector listed)
    3  halfway between the scores of rank r and r + 1, r = max(1, B // 100)        (about 1 % listed)."""
import os
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_metric_grid as mg

RANGE_HDR = os.path.join(sg.ROOT, "quantization_amd", "csrc", "mcq_range_kernels.h")
METRICS = ("l2", "ip", "cosine")


def constants():
    """the constants of the top-k scan the sweeps share, and kRangeWaves of mcq_range_kernels.h"""
    c = dict(sg.constants())
    with open(RANGE_HDR) as f:
        m = re.search(r"constexpr\s+int\s+kRangeWaves\s*=\s*([0-9]+);", f.read())
    assert m, "kRangeWaves moved out of mcq_range_kernels.h: update tests/search_range_grid.py"
    c["kRangeWaves"] = int(m.group(1))
    return c


@dataclass(frozen=True)
class Plan:
    qt: int
    qtiles: int
    slices: int
    per_slice: int
    waves: int
    lds: int
    ws_bytes: int

    def slice_len(self, B, s):
        return min(B, (s + 1) * self.per_slice) - s * self.per_slice

    def run(self, B, s):
        """steps of 64 candidates a wave of slice s owns (its last wave may own fewer, later ones none)"""
        steps = (self.slice_len(B, s) + 63) // 64
        return (steps + self.waves - 1) // self.waves

    def multi_step(self, B):
        return any(self.run(B, s) > 1 for s in range(self.slices))

    def last_step_partial(self, B):
        return any(self.slice_len(B, s) % 64 != 0 for s in range(self.slices))

    def idle_waves(self, B):
        """some wave owns no step at all"""
        return any(self.run(B, s) * (self.waves - 1) >= (self.slice_len(B, s) + 63) // 64 for s in range(self.slices))


def range_plan(Q, B, N, K, c=None):
    c = c or constants()
    W = c["kRangeWaves"]
    qt, qtiles, slices, per = sg.tile_plan(Q, B, N, K, W, c)
    return Plan(qt, qtiles, slices, per, W, qt * N * K * 4 + W * qt * 8, sg.align256(Q * slices * W * 8))


# ------------------------------------------------------------------ rules 7 and 8 in numpy
def restate_range(s, thr):
    """s (Q, B) float32 scores, thr (Q,) float32 -> (counts int64 (Q,), positions int64 (total,), scores float32 (total,)),
    the entries of query q after those of q - 1, in ascending position"""
    s = np.asarray(s, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        hit = s <= thr[:, None]                                 # a NaN compares false
    counts = hit.sum(axis=1).astype(np.int64)
    qs, pos = np.nonzero(hit)                                   # row-major: q ascending, then b ascending
    return counts, pos.astype(np.int64), s[qs, pos]


def thresholds_for(s, q_first=0):
    """the thresholds of the module docstring for the rows of s, which are queries q_first, q_first + 1, ..."""
    s = np.asarray(s, dtype=np.float32)
    Qc, B = s.shape
    thr = np.empty(Qc, dtype=np.float32)
    for i in range(Qc):
        mode = (q_first + i) % 4
        if mode == 1:
            thr[i] = -np.inf
        elif mode == 2:
            thr[i] = np.inf
        elif mode == 0:
            r = min(B, 10)
            thr[i] = np.partition(s[i], r - 1)[r - 1]
        else:
            r = max(1, B // 100)
            if r >= B:
                thr[i] = np.partition(s[i], B - 1)[B - 1]
            else:
                lo, hi = np.partition(s[i], (r - 1, r))[r - 1:r + 1]
                thr[i] = np.float32((np.float64(lo) + np.float64(hi)) / 2)
    return thr


def restate(T, w, codes, metric, thr=None, qchunk=8):
    """rules 3', 7 and 8 for all queries, a few at a time (the score matrix of a large store is not held whole).
    thr None: the thresholds of thresholds_for.  -> (thr (Q,), lims int64 (Q + 1,), positions, scores)"""
    Q = T.shape[0]
    out_thr = np.empty(Q, dtype=np.float32)
    lims = np.zeros(Q + 1, dtype=np.int64)
    pos, val = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for a in range(0, Q, qchunk):
        s = mg.restate_metric_scores(T[a:a + qchunk], w, codes, metric)
        out_thr[a:a + qchunk] = thresholds_for(s, a) if thr is None else thr[a:a + qchunk]
        n, p, v = restate_range(s, out_thr[a:a + qchunk])
        lims[a + 1:a + 1 + len(n)] = n
        pos.append(p)
        val.append(v)
    return out_thr, np.cumsum(lims), np.concatenate(pos), np.concatenate(val)


# ------------------------------------------------------------------ the GPU cases
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    K: int
    D: int
    Q: int
    B: int
    k: int = 10                     # the k of the top-k scan the range search is compared with
    state: str = "synthetic"        # as tests/search_grid.py: "synthetic" | "trained" | "decode_only"
    codes: str = "encode"           # "encode" | "random" | "dup16" (16 distinct codes: many equal scores at a threshold)
    queries: str = "gaussian"       # "gaussian" | "fp16"
    packed: bool = False            # the store keeps encode's packed 16-entry codes
    tiles: bool = False             # claims: more than one query tile,
    sliced: bool = False            # more than one slice,
    multi: bool = False             # a wave that takes more than one step of its slice (its steps are contiguous),
    partial: bool = False           # a last step of fewer than 64 candidates,
    idle: bool = False              # a wave that owns no step,
    empty: bool = False             # some query lists nothing,
    full: bool = False              # some query lists every stored vector,
    ties: bool = False              # at least 8 stored vectors score exactly the threshold of some query


BIG = 1_048_576 + 17
CASES = [
    Case("trained_8x256_d512", 8, 256, 512, 200, 100_003, state="trained", tiles=True, sliced=True, multi=True, partial=True,
         idle=True, empty=True, full=True),
    Case("big_8x256_d24", 8, 256, 24, 17, BIG, k=64, tiles=True, sliced=True, multi=True, partial=True, idle=True, empty=True,
         full=True),
    Case("n1_k16_one", 1, 16, 24, 1, 1, k=1, partial=True, idle=True, full=True),
    Case("n2_k64_b63", 2, 64, 24, 17, 63, tiles=True, partial=True, idle=True, empty=True, full=True),
    Case("n16_k16_packed_b65", 16, 16, 512, 17, 65, k=64, packed=True, tiles=True, partial=True, idle=True, empty=True, full=True),
    Case("n64_k256_decode_only", 64, 256, 24, 17, 100_003, state="decode_only", codes="random", tiles=True, sliced=True,
         multi=True, partial=True, idle=True, empty=True, full=True),
    Case("n64_k16_b1024", 64, 16, 24, 3, 1024, k=1, packed=True, full=True, empty=True),
    Case("n1_k256_b64", 1, 256, 512, 17, 64, k=1, tiles=True, idle=True, empty=True, full=True),
    Case("dup16_k64", 8, 256, 24, 17, 4096, k=64, codes="dup16", tiles=True, sliced=True, empty=True, full=True, ties=True),
    Case("dup16_multi", 8, 256, 24, 200, 40_000, k=64, codes="dup16", tiles=True, sliced=True, multi=True, idle=True,
         empty=True, full=True, ties=True),
    Case("fp16_queries", 8, 64, 24, 17, 4099, queries="fp16", tiles=True, sliced=True, partial=True, idle=True, empty=True,
         full=True),
    Case("decode_only_8x256", 8, 256, 512, 17, 4099, state="decode_only", codes="random", tiles=True, sliced=True, partial=True,
         idle=True, empty=True, full=True),
    Case("n8_k256_q1", 8, 256, 512, 1, 100_003, k=1, sliced=True, partial=True, idle=True),
]


def host_codes(case, rs):
    """codes of the case's shape for the CPU check of its claims (the GPU test encodes where the case says so)"""
    if case.codes == "dup16":
        return rs.randint(0, case.K, size=(16, case.N)).astype(np.uint8)[rs.randint(0, 16, size=case.B)]
    return rs.randint(0, case.K, size=(case.B, case.N)).astype(np.uint8)
