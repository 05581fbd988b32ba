"""The search over stored codes under a mask: the numpy restatement of rules 10 and 11 of the contract (include/mcq.h) on top of
the scores of tests/search_metric_grid.py (rules 3 and 3'), the mask patterns, and the case table of
tests/test_gpu_search_mask.py.

    candidate(b)  iff  bit b & 63 of word b >> 6 is set                 numpy.packbits(keep, bitorder="little") read as uint64
    top-k / range search: rules 4, 7 and 8 over the candidates, positions staying those of the whole store

The restatement drops the scores of the positions a mask leaves out and hands the rest to restate_topk (search_grid) or
restate_range (search_range_grid); what they return as positions among the kept is mapped back through nonzero(keep).

Each case CLAIMS what its patterns reach in the kernels (tests/test_search_mask_host.py checks the claims against the mirrors
of the launch arithmetic, search_grid.scan_plan and search_range_grid.range_plan, and against the restatement), so that a
moved constant makes a test fail instead of leaving the GPU cases covering nothing.  kMaskWindow is read from the source."""
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_metric_grid as mg
import search_range_grid as rg

METRICS = rg.METRICS
PATTERNS = ("all", "none", "one_last", "one_first", "half", "sparse", "blocks", "run", "tail_off", "few", "garbage_tail")


def constants():
    """the constants of the scan and of the sweeps, and kMaskWindow of mcq_search_kernels.h"""
    c = dict(rg.constants())
    with open(sg.HDR) as f:
        m = re.search(r"constexpr\s+int\s+kMaskWindow\s*=\s*([0-9]+);", f.read())
    assert m, "kMaskWindow moved out of mcq_search_kernels.h: update tests/search_mask_grid.py"
    c["kMaskWindow"] = int(m.group(1))
    return c


# ------------------------------------------------------------------ rule 10 in numpy, and the patterns
def words_of(B):
    return (B + 63) // 64


def pack(keep):
    """rule 10: bool (B,) -> int64 (ceil(B / 64),), bit b & 63 of word b >> 6; the bits past B are zero"""
    keep = np.asarray(keep, dtype=bool)
    raw = np.packbits(keep, bitorder="little")
    out = np.zeros(words_of(len(keep)) * 8, dtype=np.uint8)
    out[:len(raw)] = raw
    return out.view("<u8").astype(np.uint64).view(np.int64)


def unpack(words, B):
    """the candidates a packed mask names among B stored vectors (bits at positions >= B are ignored)"""
    bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")
    return bits[:B].astype(bool)


def keep_for(pattern, B, seed, k):
    """the candidates of a pattern over a store of B vectors, a function of (pattern, B, seed, k)"""
    rs = np.random.RandomState(seed * 7919 + B % 1009)
    keep = np.zeros(B, dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "none":
        pass
    elif pattern == "one_last":
        keep[B - 1] = True
    elif pattern == "one_first":
        keep[0] = True
    elif pattern in ("half", "garbage_tail"):
        keep = rs.rand(B) < 0.5
    elif pattern == "sparse":                                   # 1 %; a store below 64 vectors keeps exactly one
        if B >= 64:
            keep = rs.rand(B) < 0.01
        if not keep.any():
            keep[rs.randint(B)] = True
    elif pattern == "blocks":                                   # whole steps of 64, every other one cleared
        keep = (np.arange(B) >> 6) % 2 == 0
    elif pattern == "run":                                      # one contiguous run of 1 %
        n = max(1, B // 100)
        a = rs.randint(B - n + 1)
        keep[a:a + n] = True
    elif pattern == "tail_off":                                 # the last step (the partial one, where there is one) cleared
        keep[:(B - 1) // 64 * 64] = True
    elif pattern == "few":                                      # k - 1 candidates spread over the store
        n = min(k - 1, B)
        keep[np.unique(np.linspace(0, B - 1, n).astype(np.int64)) if n else []] = True
    else:
        raise ValueError(pattern)
    return keep


def words_for(pattern, B, seed, k):
    """(keep, packed words) of a pattern.  garbage_tail sets the bits of the last word at positions >= B: the candidates are
    those of `half`, and only a hand-packed mask can say so."""
    keep = keep_for(pattern, B, seed, k)
    words = pack(keep)
    if pattern == "garbage_tail" and B % 64:
        words = words.copy()
        words[-1] = (words.view(np.uint64)[-1] | (np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(B % 64))).view(np.int64)
    return keep, words


# ------------------------------------------------------------------ rule 11 in numpy
def map_back(out_i, pos):
    """positions among the kept -> positions of the whole store; -1 (no candidate) stays -1"""
    return np.concatenate([pos, [-1]]).astype(np.int64)[out_i]


def restate_topk_masked(s, keep, k):
    """s (Q, B) float32 scores of the WHOLE store, keep bool (B,) -> (scores (Q, k), positions (Q, k)) over the candidates"""
    pos = np.flatnonzero(keep)
    out_s, out_i = sg.restate_topk(np.ascontiguousarray(s[:, pos]), k)
    return out_s, map_back(out_i, pos)


def restate_range_masked(s, keep, thr):
    """-> (lims int64 (Q + 1,), positions int64, scores float32): rules 7 and 8 over the candidates, original positions"""
    pos = np.flatnonzero(keep)
    n, p, v = rg.restate_range(np.ascontiguousarray(s[:, pos]), thr)
    return np.concatenate([[0], np.cumsum(n)]).astype(np.int64), pos[p].astype(np.int64), v


def compact_topk(T, w, codes, k, metric, keep):
    """rule 11's equivalence: the unmasked restatement over codes[keep], w[keep], positions mapped through nonzero(keep)"""
    pos = np.flatnonzero(keep)
    out_s, out_i = mg.restate_metric(T, None if w is None else w[pos], codes[pos], k, metric)
    return out_s, map_back(out_i, pos)


def compact_range(T, w, codes, metric, keep, thr):
    pos = np.flatnonzero(keep)
    if len(pos) == 0:
        return np.zeros(T.shape[0] + 1, dtype=np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    _, lims, p, v = rg.restate(T, None if w is None else w[pos], codes[pos], metric, thr=thr)
    return lims, pos[p].astype(np.int64), v


# ------------------------------------------------------------------ what a mask does to the waves of the two kernels
def wave_steps(plan, B, waves, strided):
    """per slice and wave the steps of 64 candidates it owns, as (slice, list of step indexes within the slice): the scan's
    waves take v, v + waves, ... (strided), a sweep's a contiguous run"""
    out = []
    for s in range(plan.slices):
        steps = (min(B, (s + 1) * plan.per_slice) - s * plan.per_slice + 63) // 64
        run = (steps + waves - 1) // waves
        for v in range(waves):
            own = range(v, steps, waves) if strided else range(min(v * run, steps), min((v + 1) * run, steps))
            out.append((s, list(own)))
    return out


def live_steps(keep, plan, B):
    """per slice, which of its steps of 64 candidates hold one"""
    out = []
    for s in range(plan.slices):
        part = keep[s * plan.per_slice:min(B, (s + 1) * plan.per_slice)]
        pad = np.zeros((len(part) + 63) // 64 * 64, dtype=bool)
        pad[:len(part)] = part
        out.append(pad.reshape(-1, 64).any(axis=1))
    return out


def reach(keep, plan, B, waves, strided):
    """-> (a wave skips an empty step between two live ones, a wave that owns steps has no live one, a slice has no candidate)"""
    skips = dead_wave = False
    live_of = live_steps(keep, plan, B)
    for s, own in wave_steps(plan, B, waves, strided):
        if not own:
            continue
        at = np.flatnonzero(live_of[s][own])
        dead_wave |= len(at) == 0
        skips |= len(at) >= 2 and at[-1] - at[0] + 1 > len(at)
    return skips, dead_wave, any(not l.any() for l in live_of)


def refills_on_empty(keep, plan, B, waves, strided, window):
    """some wave owns more than `window` steps and the first `window` of them are all empty: it refills with nothing found"""
    live_of = live_steps(keep, plan, B)
    return any(len(own) > window and not live_of[s][own[:window]].any() for s, own in wave_steps(plan, B, waves, strided))


def longest_run(plan, B, waves, strided):
    return max(len(own) for _, own in wave_steps(plan, B, waves, strided))


# ------------------------------------------------------------------ the GPU cases
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    K: int
    D: int
    Q: int
    B: int
    k: int = 10
    state: str = "synthetic"        # as tests/search_grid.py: "synthetic" | "decode_only"
    codes: str = "encode"           # "encode" | "random" | "dup16"
    queries: str = "gaussian"       # "gaussian" | "fp16"
    packed: bool = False
    restate: bool = True            # the GPU test compares with the numpy restatement (else with the compacted store alone)
    # claims -- over the patterns that keep at least one candidate, in the scan AND in the sweeps:
    skips: bool = False             # some wave skips an empty step between two live ones,
    dead_wave: bool = False         # some wave that owns steps has no live one,
    dead_slice: bool = False        # some slice has no candidate;
    short: bool = False             # over all patterns: some has candidates, but fewer than k,
    best_cleared: bool = False      # some query's best position of the whole store has its bit cleared (candidates exist),
    tie_at_k: bool = False          # some query's k-th kept score is also the score of a cleared position;
    long_run: bool = False          # a wave of the scan and a wave of the sweeps own more than kMaskWindow steps


CASES = [
    Case("n1_k16_one", 1, 16, 24, 1, 1, k=1),
    Case("n2_k64_b63", 2, 64, 24, 17, 63, short=True, best_cleared=True),
    Case("n8_k256_b64", 8, 256, 24, 17, 64, short=True, best_cleared=True),
    Case("n16_k16_packed_b65", 16, 16, 512, 17, 65, packed=True, dead_wave=True, short=True, best_cleared=True),
    Case("n8_k256_b4099", 8, 256, 24, 17, 4099, dead_wave=True, dead_slice=True, short=True, best_cleared=True),
    Case("dup16_b40000", 8, 256, 24, 200, 40_000, codes="dup16", skips=True, dead_wave=True, dead_slice=True, short=True,
         best_cleared=True, tie_at_k=True),
    Case("n64_k256_decode_only", 64, 256, 24, 17, 100_003, state="decode_only", codes="random", skips=True, dead_wave=True,
         dead_slice=True, short=True, best_cleared=True),
    Case("n8_k256_q1_k1", 8, 256, 24, 1, 100_003, k=1, dead_wave=True, dead_slice=True, best_cleared=True),
    Case("fp16_queries", 8, 64, 24, 17, 4099, queries="fp16", dead_wave=True, dead_slice=True, short=True, best_cleared=True),
    Case("long_run", 64, 256, 24, 258, 70_000, state="decode_only", codes="random", restate=False, skips=True, dead_wave=True,
         short=True, best_cleared=True, long_run=True),
]


def host_data(case, queries=8):
    """tables, codes of the case's kind and the per-candidate arrays for the CPU check of its claims.  The tables are not
    grid-valued and t is a function of the code, as norms are: equal scores come from equal codes alone."""
    rs = np.random.RandomState(case.B % 1009 + case.N)
    Q = min(case.Q, queries)
    T = rs.randn(Q, case.N, case.K).astype(np.float32)
    codes = rg.host_codes(case, rs)
    U = (rs.randint(1, 64, size=(case.N, case.K)) / 4.0).astype(np.float32)
    t = np.zeros(case.B, dtype=np.float32)
    for n in range(case.N):
        t = (t + U[n][codes[:, n]]).astype(np.float32)
    return T, codes, t
