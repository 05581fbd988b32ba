"""The search list by list (mcq_search_scan_lists, Quantizer.search_lists): the mirror of its launch arithmetic (lists_plan of
quantization_amd/csrc/mcq_api.hip, the kList* constants of mcq_search_kernels.h), the numpy restatement of rules 13-15 of the
contract (include/mcq.h) on top of the scores of tests/search_metric_grid.py (rules 3 and 3'), and the case table of
tests/test_gpu_search_lists.py.

    list l       = the positions [list_offsets[l], list_offsets[l + 1])
    candidate(q, b)  iff  b lies in a list that row q of `probes` names (an entry outside [0, L) names none) and, under a
                          mask, bit b of the mask is set
    top-k: rule 4 over the candidates of each query, positions staying those of the store

The restatement takes, per query, the candidate positions in ascending order, hands those columns of the score matrix to
restate_topk (search_grid) and maps what it returns back through them (an increasing map: the order carries over).

Each case CLAIMS what its lists and probes reach (tests/test_search_lists_host.py checks the claims against this mirror and
against the restatement), so that a moved constant makes a test fail instead of leaving the GPU cases covering nothing."""
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_mask_grid as kg

METRICS = ("l2", "ip", "cosine")
PATTERNS = (None, "half", "sparse")             # the masks of the GPU cases: none, and two patterns of search_mask_grid
NAMES = ("kListWaves", "kListTargetBlocks", "kListMaxProbes")


def constants():
    c = dict(sg.constants())
    with open(sg.HDR) as f:
        src = f.read()
    for name in NAMES:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9]+);", src)
        assert m, f"{name} moved out of mcq_search_kernels.h: update tests/search_lists_grid.py"
        c[name] = int(m.group(1))
    return c


@dataclass(frozen=True)
class Plan:
    parts: int
    lds: int
    ws_bytes: int


def lists_plan(Q, P, N, K, k, c=None):
    """lists_plan of mcq_api.hip: the parts per query, a function of the call's shape alone"""
    c = c or constants()
    parts = min(max(c["kListTargetBlocks"] // max(Q, 1), 1), c["kScanMaxSlices"])
    head = (max(N * K * 4, c["kListWaves"] * 64 * 8) + 15) & ~15
    return Plan(parts, head + (P + 1) * 8 + P * 8, 2 * sg.align256(Q * parts * k * 4))


# ------------------------------------------------------------------ rules 13-15 in numpy
def candidates(list_offsets, row, keep=None):
    """the candidate positions of one query, ascending: the union of the lists its row names, under the mask if there is one"""
    L = len(list_offsets) - 1
    named = [int(l) for l in row if 0 <= int(l) < L]
    if not named:
        return np.zeros(0, dtype=np.int64)
    pos = np.unique(np.concatenate([np.arange(list_offsets[l], list_offsets[l + 1], dtype=np.int64) for l in named]))
    return pos if keep is None else pos[keep[pos]]


def union_mask(list_offsets, row, B, keep=None):
    """bool (B,): the mask under which a scan of the whole store has the candidates of this row (rule 14)"""
    m = np.zeros(B, dtype=bool)
    m[candidates(list_offsets, row, keep)] = True
    return m


def restate_lists(s, list_offsets, probes, k, keep=None):
    """s (Q, B) float32 scores of the WHOLE store -> (scores (Q, k), positions (Q, k)) over each query's own candidates"""
    Q = s.shape[0]
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        pos = candidates(list_offsets, probes[q], keep)
        ts, ti = sg.restate_topk(np.ascontiguousarray(s[q:q + 1, pos]), k)
        out_s[q], out_i[q] = ts[0], kg.map_back(ti, pos)[0]
    return out_s, out_i


# ------------------------------------------------------------------ what the lists do to the parts and waves of the kernel
def step_space(list_offsets, row, B):
    """per probe of a row (begin, end, steps) as the kernel forms them, and the exclusive prefix sums of the steps"""
    L = len(list_offsets) - 1
    rng = []
    for l in row:
        a = z = 0
        if 0 <= int(l) < L:
            a, z = (min(max(int(list_offsets[int(l) + j]), 0), B) for j in (0, 1))
            if a >= z:
                a = z = 0
        rng.append((a, z, (z - a + 63) // 64))
    return rng, np.concatenate([[0], np.cumsum([r[2] for r in rng])]).astype(np.int64)


def part_steps(T, parts):
    """the steps [lo, hi) of every part of a query with T steps"""
    return [(T * s // parts, T * (s + 1) // parts) for s in range(parts)]


def probe_of(pre, step):
    return int(np.searchsorted(pre, step, side="right")) - 1


def reach(list_offsets, probes, B, parts, waves):
    """-> dict of what some (query, part) of the call meets: `cut` -- one list spans more than one part and, in some part,
    gives every wave a step; `two_steps` -- a wave takes more than one step; `boundary` -- the consecutive steps of a wave lie
    in two different lists; `empty_part` -- a part without a step beside a part with one"""
    got = dict(cut=False, two_steps=False, boundary=False, empty_part=False)
    for row in probes:
        rng, pre = step_space(list_offsets, row, B)
        T = int(pre[-1])
        owners = [[] for _ in row]
        for s, (lo, hi) in enumerate(part_steps(T, parts)):
            got["empty_part"] |= lo == hi and T > 0
            got["two_steps"] |= hi - lo > waves
            of = [probe_of(pre, st) for st in range(lo, hi)]
            for v in range(waves):
                mine = of[v::waves]
                got["boundary"] |= any(a != b for a, b in zip(mine, mine[1:]))
            for p in set(of):
                owners[p].append((s, sum(1 for o in of if o == p) >= waves and len(set(of[:waves])) == 1 and of[0] == p))
        got["cut"] |= any(len(o) > 1 and any(full for _, full in o) for o in owners)
    return got


# ------------------------------------------------------------------ the GPU cases
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    K: int
    D: int
    Q: int
    B: int
    k: int
    P: int
    lists: str                      # "mixed" | "cover" | "ones" | "single": layout() below
    L: int = 0                      # the number of lists ("cover"; the other layouts fix their own)
    state: str = "synthetic"        # as tests/search_grid.py
    codes: str = "encode"           # "encode" | "random" | "dup16"
    queries: str = "gaussian"
    packed: bool = False
    # claims (tests/test_search_lists_host.py):
    covering: bool = False          # the lists cover [0, B): with every list probed the call is the scan of the whole store
    empty_list: bool = False        # a probed list is empty
    short: bool = False             # some query has candidates, but fewer than k
    cut: bool = False               # a list is cut across parts and gives all waves of some part a step
    two_steps: bool = False         # some wave takes more than one step
    boundary: bool = False          # some wave's consecutive steps lie in different lists
    empty_part: bool = False        # some part has no step
    tie_across: bool = False        # some query's list of results holds one score at positions of two different lists
    unordered: bool = False         # some probe row is not ascending
    pad_row: bool = False           # a row of -1 only
    mixed_row: bool = False         # a row mixing -1, L and large or negative values with real lists


MIXED_LENS = (0, 1, 63, 64, 65, 130, 3000, 7, 0, 500)          # list lengths of the "mixed" layout, from position 5 on
MIXED_START = 5

CASES = [
    Case("n1_k16_single_p1", 1, 16, 24, 1, 200, 1, 1, "single", empty_part=True),
    Case("n2_k64_mixed_p7", 2, 64, 24, 17, 6000, 10, 7, "mixed", empty_list=True, short=True, unordered=True, pad_row=True,
         mixed_row=True, empty_part=True, tie_across=True),
    Case("n8_k256_long_p2", 8, 256, 24, 17, 20_000, 10, 2, "cover", L=3, covering=True, cut=True, two_steps=True, boundary=True,
         empty_part=True, unordered=True),
    Case("n16_k256_cover_p64", 16, 256, 24, 3, 8000, 64, 64, "cover", L=130, codes="random", covering=True, empty_list=True,
         empty_part=True, unordered=True),
    Case("n64_k256_cover_p130", 64, 256, 24, 3, 5000, 10, 130, "cover", L=130, state="decode_only", codes="random",
         covering=True, empty_list=True, empty_part=True, unordered=True, mixed_row=True),
    Case("n8_k256_ones_p4096", 8, 256, 24, 1, 6144, 10, 4096, "ones", covering=True, boundary=True, two_steps=True,
         unordered=True),
    Case("dup16_cover_p7", 8, 256, 24, 17, 4099, 64, 7, "cover", L=64, codes="dup16", covering=True, tie_across=True,
         unordered=True, empty_part=True),
]


def layout(case):
    """(list_offsets int64 (L + 1,), probes int32 (Q, P)) of a case, a function of the case alone"""
    rs = np.random.RandomState(case.B % 1009 + 31 * case.P)
    B, Q, P = case.B, case.Q, case.P
    if case.lists == "single":                              # one list of 65 vectors from position 3 on
        off = np.array([3, 68], dtype=np.int64)
    elif case.lists == "mixed":
        off = MIXED_START + np.concatenate([[0], np.cumsum(MIXED_LENS)]).astype(np.int64)
    elif case.lists == "ones":                              # 4,096 lists of one or two vectors
        off = np.concatenate([[0], np.cumsum(1 + np.arange(4096) % 2)]).astype(np.int64)
    elif case.lists == "cover":
        if case.L == 3:                                     # one list long enough for every wave of several parts
            off = np.array([0, 70, 70 + 19_000, B], dtype=np.int64)
        else:
            off = np.concatenate([[0], np.sort(rs.randint(0, B + 1, size=case.L - 1)), [B]]).astype(np.int64)
    else:
        raise ValueError(case.lists)
    L = len(off) - 1
    assert 0 <= off[0] and off[-1] <= B and (np.diff(off) >= 0).all()
    probes = np.full((Q, P), -1, dtype=np.int32)
    for q in range(Q):
        n = min(P, L)
        probes[q, rs.permutation(P)[:n]] = rs.permutation(L)[:n]        # distinct lists, scattered among the padding
    if case.lists == "mixed":
        probes[0] = -1
        probes[1] = [-1, L, 2 ** 31 - 1, -5, 6, 1, 0]
        probes[2] = [1, 0, 8, -1, -1, -1, -1]               # 1 candidate
        probes[3] = [9, 6, 5, 4, 3, 2, 1]
        probes[4] = [6, 7, -1, -1, -1, -1, -1]              # the long list, then a short one
    if case.name == "n64_k256_cover_p130":
        probes[1, ::3] = -1
        probes[1, 1] = L
        probes[1, 4] = -2 ** 31
        probes[1, 7] = 2 ** 31 - 1
    return off, probes


def all_probes(case, L):
    """every list once per row, each row scrambled in its own way"""
    rs = np.random.RandomState(case.B % 1009 + 7)
    return np.stack([rs.permutation(L) for _ in range(case.Q)]).astype(np.int32)


def host_data(case):
    """tables, codes of the case's kind and the per-candidate array for the CPU check of its claims (search_mask_grid)"""
    return kg.host_data(case, queries=case.Q)
