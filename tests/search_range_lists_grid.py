"""The range search list by list (mcq_search_range_lists_count / _fill, Quantizer.range_search_lists): the mirror of its launch
arithmetic (range_lists_plan of quantization_amd/csrc/mcq_api.hip; kRangeListWaves of mcq_range_kernels.h, the kList* constants
of mcq_search_kernels.h), the numpy restatement of rules 17 and 18 of the contract (include/mcq.h) on top of the scores of
tests/search_metric_grid.py (rules 3 and 3'), and the case table of tests/test_gpu_search_range_lists.py.

    listed(q, b)  iff  b lies in a list that row q of `probes` names, its bit is set under a mask, and score[q][b] <= thr[q]
    entries of q  in the order of its probe row: slot 0's list first, ascending position within a list; a list named twice
                  is listed twice

The restatement walks, per query, the slots of its row in order and appends the positions of the named list that pass; it
removes no duplicate and sorts nothing.

The thresholds of a case are a function of its scores (thresholds_for): query q takes, by q mod 6, over the scores of ITS
candidates (under the mask of the call)
    0  -inf                                   nothing listed
    1  the smallest score itself              exactly one hit unless tied: the comparison is inclusive
    2  the score of rank max(1, n // 100)     about 1 % listed
    3  the score of rank n // 2 + 1           about half
    4  +inf                                   every candidate listed
    5  NaN                                    nothing listed
and a query without a candidate takes +inf (it lists nothing whatever the threshold).  The GPU test runs the cases of ONE
query a second time with the thresholds shifted by 4 (query 0 takes +inf): their only query would otherwise list nothing.

Each case CLAIMS what its lists, probes and hits reach in the kernel (tests/test_search_range_lists_host.py checks the claims
against this mirror and against the restatement on host-made scores), so that a moved constant makes a test fail instead of
leaving the GPU cases covering nothing."""
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg

METRICS = lg.METRICS
PATTERNS = lg.PATTERNS


def constants():
    c = dict(lg.constants())
    with open(rg.RANGE_HDR) as f:
        m = re.search(r"constexpr\s+int\s+kRangeListWaves\s*=\s*([0-9]+);", f.read())
    assert m, "kRangeListWaves moved out of mcq_range_kernels.h: update tests/search_range_lists_grid.py"
    c["kRangeListWaves"] = int(m.group(1))
    return c


@dataclass(frozen=True)
class Plan:
    parts: int
    waves: int
    lds: int
    ws_bytes: int


def range_lists_plan(Q, P, N, K, c=None):
    """range_lists_plan of mcq_api.hip: the parts of lists_plan, the LDS of k_search_lists, 8 bytes per (query, part, wave)"""
    c = c or constants()
    W = c["kRangeListWaves"]
    parts = min(max(c["kListTargetBlocks"] // max(Q, 1), 1), c["kScanMaxSlices"])
    head = (max(N * K * 4, c["kListWaves"] * 64 * 8) + 15) & ~15
    return Plan(parts, W, head + (P + 1) * 8 + P * 8, sg.align256(Q * parts * W * 8))


# ------------------------------------------------------------------ rules 17 and 18 in numpy
def row_positions(list_offsets, row):
    """the candidate positions of one query IN THE ORDER OF ITS ROW, a list named twice twice (no mask)"""
    L = len(list_offsets) - 1
    out = [np.zeros(0, dtype=np.int64)]
    for l in row:
        if 0 <= int(l) < L:
            out.append(np.arange(list_offsets[int(l)], list_offsets[int(l) + 1], dtype=np.int64))
    return np.concatenate(out)


def restate_range_lists(s, list_offsets, probes, thr, keep=None):
    """s (Q, B) float32 scores of the WHOLE store, thr (Q,) float32 -> (lims int64 (Q + 1,), positions int64, scores float32)"""
    s = np.asarray(s, dtype=np.float32)
    thr = np.asarray(thr, dtype=np.float32)
    lims = np.zeros(len(probes) + 1, dtype=np.int64)
    pos, val = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for q, row in enumerate(probes):
        p = row_positions(list_offsets, row)
        if keep is not None:
            p = p[keep[p]]
        with np.errstate(invalid="ignore"):
            p = p[s[q, p] <= thr[q]]                              # a NaN compares false
        lims[q + 1] = lims[q] + len(p)
        pos.append(p)
        val.append(s[q, p])
    return lims, np.concatenate(pos), np.concatenate(val)


def thresholds_for(s, list_offsets, probes, keep=None, shift=0):
    """the thresholds of the module docstring; shift: query q takes the threshold of q + shift (a case of one query would
    otherwise only ever list nothing)"""
    thr = np.empty(len(probes), dtype=np.float32)
    for q, row in enumerate(probes):
        p = row_positions(list_offsets, row)
        if keep is not None:
            p = p[keep[p]]
        v = np.sort(s[q, p])
        n, mode = len(v), (q + shift) % 6
        if mode == 0:
            thr[q] = -np.inf
        elif mode == 5:
            thr[q] = np.nan
        elif mode == 4 or n == 0:
            thr[q] = np.inf
        elif mode == 1:
            thr[q] = v[0]
        elif mode == 2:
            thr[q] = v[max(1, n // 100) - 1]
        else:
            thr[q] = v[n // 2]
    return thr


def sorted_rows(probes, L):
    """the rows as Quantizer.range_search_lists hands them on: entries that name no list become -1, then each row ascends"""
    p = np.where((probes >= 0) & (probes < L), probes, -1).astype(np.int32)
    return np.sort(p, axis=1)


def distinct(list_offsets, row):
    L = len(list_offsets) - 1
    named = [int(l) for l in row if 0 <= int(l) < L]
    return len(named) == len(set(named))


# ------------------------------------------------------------------ what the lists and the hits do to parts and waves
def wave_runs(T, parts, waves):
    """per part the steps [a, b) of each of its waves: contiguous runs of ceil((hi - lo) / waves), as k_range_lists cuts them"""
    out = []
    for lo, hi in lg.part_steps(T, parts):
        run = -(-(hi - lo) // waves)
        out.append([(min(lo + v * run, hi), min(lo + (v + 1) * run, hi)) for v in range(waves)])
    return out


def step_hits(s_row, thr, list_offsets, row, B, keep=None):
    """bool (T, 64): lane l of flattened step i of this query holds a hit; and the prefix sums of the steps per probe"""
    rng, pre = lg.step_space(list_offsets, row, B)
    T = int(pre[-1])
    hit = np.zeros((T, 64), dtype=bool)
    for (a, z, n), first in zip(rng, pre[:-1]):
        if n == 0:
            continue
        p = np.arange(a, z, dtype=np.int64)
        with np.errstate(invalid="ignore"):
            h = s_row[p] <= thr
        if keep is not None:
            h &= keep[p]
        flat = np.zeros(n * 64, dtype=bool)
        flat[:len(p)] = h
        hit[first:first + n] = flat.reshape(n, 64)
    return hit, pre


def reach(s, thr, list_offsets, probes, B, parts, waves):
    """-> dict of what some (query, part, wave) of the call meets:
    boundary     a wave's run of steps crosses from one list into another
    idle         a part that has steps leaves a wave without one (idle waves beside busy ones)
    empty_part   a part without a step beside a part with one
    spread       a query's hits lie in at least 2 parts AND in at least 2 waves of one part
    later_lanes  a step has hits in several lanes after earlier hits of the same wave (the slot is base + cnt + rank)
    zero_between a query without a hit between two queries that have hits"""
    got = dict(boundary=False, idle=False, empty_part=False, spread=False, later_lanes=False, zero_between=False)
    totals = []
    for q, row in enumerate(probes):
        hit, pre = step_hits(s[q], thr[q], list_offsets, row, B)
        T = int(pre[-1])
        per_step = hit.sum(axis=1)
        totals.append(int(per_step.sum()))
        parts_hit, two_waves = 0, False
        for runs in wave_runs(T, parts, waves):
            lo, hi = runs[0][0], runs[-1][1]
            got["empty_part"] |= lo == hi and T > 0
            got["idle"] |= hi > lo and any(a == b for a, b in runs)
            waves_hit = 0
            for a, b in runs:
                if a == b:
                    continue
                got["boundary"] |= lg.probe_of(pre, a) != lg.probe_of(pre, b - 1)
                c = per_step[a:b]
                before = np.concatenate([[0], np.cumsum(c)[:-1]])
                got["later_lanes"] |= bool(((c >= 2) & (before > 0)).any())
                waves_hit += bool(c.sum() > 0)
            parts_hit += waves_hit > 0
            two_waves |= waves_hit >= 2
        got["spread"] |= parts_hit >= 2 and two_waves
    some = [i for i, n in enumerate(totals) if n > 0]
    got["zero_between"] = any(totals[i] == 0 for i in range(some[0], some[-1])) if some else False
    return got


# ------------------------------------------------------------------ the GPU cases
CLAIMS = ("boundary", "idle", "empty_part", "spread", "later_lanes", "zero_between")


@dataclass(frozen=True)
class Case:
    base: lg.Case                   # shape, state, codes and queries as the search list by list has them
    boundary: bool = False          # the claims: reach() above
    idle: bool = False
    empty_part: bool = False
    spread: bool = False
    later_lanes: bool = False
    zero_between: bool = False
    twice: bool = False             # some row names a list twice

    def __getattr__(self, name):    # N, K, D, Q, B, k, P, name, state, codes, queries, packed, covering: the base's
        return getattr(object.__getattribute__(self, "base"), name)


# N = 4 so that chunks of 4 codebooks are launched: the "mixed" lengths of search_lists_grid with its two long lists cut to
# 300 and 50 vectors, so that the ten lists fit a store of 700 (they end at 685: the last 15 vectors belong to none)
N4 = lg.Case("n4_k16_mixed_p3", 4, 16, 24, 5, 700, 10, 3, "mixed", packed=True)     # (encode packs 16-entry codes)
N4_LENS = (0, 1, 63, 64, 65, 130, 300, 7, 0, 50)
N4_PROBES = [[6, 5, 2],             # q 0  (-inf)   nothing listed
             [9, 6, 1],             # q 1  (min)    a row that does not ascend
             [0, 8, -1],            # q 2           empty lists and padding: no candidate between two queries that have hits
             [2, 3, 4],             # q 3  (about half)
             [6, 6, 7]]             # q 4  (+inf)   a list named twice: listed twice

_BY = {c.name: c for c in lg.CASES}
CASES = [
    Case(_BY["n1_k16_single_p1"], idle=True, empty_part=True),
    Case(_BY["n2_k64_mixed_p7"], idle=True, empty_part=True, spread=True, zero_between=True),
    Case(_BY["n8_k256_long_p2"], boundary=True, idle=True, empty_part=True, spread=True, later_lanes=True, zero_between=True),
    Case(_BY["n16_k256_cover_p64"], idle=True, empty_part=True),
    Case(_BY["n64_k256_cover_p130"], idle=True, empty_part=True),
    Case(_BY["n8_k256_ones_p4096"], boundary=True),
    Case(_BY["dup16_cover_p7"], idle=True, empty_part=True, zero_between=True),
    Case(N4, idle=True, empty_part=True, zero_between=True, twice=True),
]


def layout(case):
    """(list_offsets int64 (L + 1,), probes int32 (Q, P)) of a case, a function of the case alone"""
    if case.name != N4.name:
        return lg.layout(case.base)
    off = lg.MIXED_START + np.concatenate([[0], np.cumsum(N4_LENS)]).astype(np.int64)
    assert off[-1] <= case.B
    return off, np.array(N4_PROBES, dtype=np.int32)


def all_ascending(case, L):
    """every list once per row, ascending"""
    return np.tile(np.arange(L, dtype=np.int32), (case.Q, 1))


def host_scores(case):
    """(scores of the whole store under L2, float32 (Q, B)) from host-made tables for the CPU check of the claims"""
    T, codes, t = kg.host_data(case, queries=case.Q)
    return mg.restate_metric_scores(T, t, codes, "l2")
