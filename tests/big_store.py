"""Stores past 2^26 rows and 4 GiB of codes with an exact reference that costs seconds: the stores, their planted rows and the
reference of tests/test_gpu_big_store.py; tests/test_big_store_host.py pins all of it on the CPU, on a miniature restated in full.

A store is a uniform BACKGROUND -- every digit 0 -- with a few hundred PLANTED rows of random digits in 1 .. K - 1.  The tables are
    T[q][n][0] = 1000          so a background row scores exactly 1000 * N under rule 3's ascending sum (integers below 2^24),
    T[q][n][k] in [-1, 1]      so the table sum of a planted row is below N in magnitude,
and the per-candidate array w is 0 (L2) or 1 (cosine) on the background and random on the planted rows: in [0, 1) under L2 (a
planted row scores below N + 1), in [0.5, 1.5) under the cosine (below 1.5 * N).  Every planted row of every query therefore
precedes every background row, for every N and every seed; `separated` checks it on the reference and the tests assert it
as a condition on their inputs.  The answer of a search over the whole store is then the answer of the existing restatement
over the COMPACT store of planted rows in ascending position, positions mapped back through the planted list as rule 11 has
it, followed -- top-k only -- by a TAIL of background rows: equal scores, so the lowest positions that are not planted.

The planted positions are where a kernel over a large store can go wrong (required()): the ends of the store, of a step of 64
and of the slices of the scan's plan, and both sides of every row at which the byte offset of the codes crosses 2^31 or 2^32.
A load whose offset wrapped at such a crossing reads the row `crossing / N` below (aliases()).  The other planted rows have
no planted row at either alias, so a wrapped load of one lands on background and the row goes missing from the answer.  The
required rows themselves cannot all be free of aliases -- rows 0 and 1 lie 2^32 / N below the rows at the 2^32 crossing, and
the rows at the two crossings lie 2^31 / N apart -- so for such a pair the host test asserts what a wrapped load needs to be
noticed there: the two rows score differently for every query under every metric."""
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg

METRICS = ("l2", "ip", "cosine")
BACKGROUND = 1000.0
Q = 3                                               # a tile of 4 with an idle query
MIN_FREE = 16 * 2 ** 30                             # the device tests skip below this many free bytes


@dataclass(frozen=True)
class Store:
    name: str
    N: int
    K: int
    B: int
    crossings: tuple = (2 ** 31, 2 ** 32)           # byte offsets of the codes whose rows are planted on both sides
    seed: int = 1

    def bg(self):
        """the score of a background row under every metric: 1000 added N times, then + 0 or * 1"""
        return np.float32(BACKGROUND * self.N)


ROWS = Store("rows", 1, 16, 2 ** 26 + 321)          # 64 * B threads pass 2^32
BYTES = Store("bytes", 64, 16, 2 ** 26 + 321)       # 4 GiB + 20 KiB of codes
EDGE = Store("edge", 1, 16, 2 ** 31 - 1, seed=2)    # positions up to 2^31 - 2
STORES = (ROWS, BYTES, EDGE)
MINI = Store("mini", 4, 16, 5000, crossings=(1250 * 4, 2500 * 4), seed=3)      # the "crossings" at rows 1,250 and 2,500


# ------------------------------------------------------------------ the planted rows
def aliases(st):
    """the distances in rows between a row and the row a wrapped load of it would read"""
    return tuple(x // st.N for x in st.crossings)


def crossing_rows(st):
    """the row in which each crossing lies and its two neighbours, where they exist"""
    out = []
    for x in st.crossings:
        r = x // st.N
        out += [r + d for d in (-1, 0, 1) if 0 <= r + d < st.B and r < st.B]
    return out


def slice_rows(st, k=64, queries=Q):
    """the first and last row of the first, a middle and the last slice of the scan's plan"""
    plan = sg.scan_plan(queries, st.B, st.N, st.K, k)
    out = []
    for s in sorted({0, plan.slices // 2, plan.slices - 1}):
        out += [s * plan.per_slice, min(st.B, (s + 1) * plan.per_slice) - 1]
    return out


def required(st, k=64, queries=Q):
    """the positions every planted list of a store holds (given enough rows), ascending"""
    B = st.B
    req = {0, 1, 63, 64, B - 1, B - 2, (B - 1) // 64 * 64}
    req.update(crossing_rows(st))
    req.update(slice_rows(st, k, queries))
    return np.array(sorted(p for p in req if 0 <= p < B), dtype=np.int64)


def planted(st, count=256, last=None, k=64, queries=Q):
    """`count` distinct planted positions, ascending: required(st), then seeded pseudo-random rows none of which has a
    planted row at an alias.  last = (rows, n): exactly n of them lie among the last `rows` rows of the store."""
    rs = np.random.RandomState(st.seed * 1009 + count)
    have = set(int(p) for p in required(st, k, queries))
    assert len(have) <= count, (st.name, len(have), count)
    deltas = aliases(st)

    def free(p):
        return p not in have and all(p + d not in have and p - d not in have for d in deltas)

    lo_tail = st.B - last[0] if last else st.B
    if last:
        assert sum(p >= lo_tail for p in have) <= last[1]
        while sum(p >= lo_tail for p in have) < last[1]:
            p = int(rs.randint(lo_tail, st.B))
            if free(p):
                have.add(p)
    while len(have) < count:
        p = int(rs.randint(0, lo_tail))
        if free(p):
            have.add(p)
    return np.array(sorted(have), dtype=np.int64)


def alias_pairs(st, pos):
    """the pairs (p, p + d) of planted positions a wrapped load would confuse"""
    have = set(int(p) for p in pos)
    return [(p, p + d) for p in sorted(have) for d in aliases(st) if p + d in have]


def digits(st, count):
    """the codes of the planted rows, (count, N) uint8 in 1 .. K - 1"""
    return np.random.RandomState(st.seed * 7919 + count).randint(1, st.K, size=(count, st.N)).astype(np.uint8)


def tables(st, queries=Q):
    T = np.random.RandomState(st.seed * 31 + queries).uniform(-1.0, 1.0, size=(queries, st.N, st.K)).astype(np.float32)
    T[:, :, 0] = BACKGROUND
    return T


def planted_w(st, count, metric):
    """w of the planted rows: None under ip, [0, 1) under l2, [0.5, 1.5) under the cosine"""
    if metric == "ip":
        return None
    u = np.random.RandomState(st.seed * 131 + count).uniform(0.0, 1.0, size=count).astype(np.float32)
    u = np.minimum(u, np.float32(1.0 - 2.0 ** -24))
    return u if metric == "l2" else (u + np.float32(0.5)).astype(np.float32)


def background_w(metric):
    return {"l2": 0.0, "cosine": 1.0}[metric]


# ------------------------------------------------------------------ the builder, shared by numpy and the device
class Numpy:
    """what build() needs of an array library; tests/test_gpu_big_store.py has the torch twin"""

    @staticmethod
    def full(shape, value, dtype):
        return np.full(shape, value, dtype=dtype)

    @staticmethod
    def put(arr, pos, vals):
        arr[pos] = vals


def build_codes(st, pos, xp=Numpy):
    """codes (B, N) uint8 of the store with the planted rows at pos"""
    codes = xp.full((st.B, st.N), 0, "uint8")
    xp.put(codes, pos, digits(st, len(pos)))
    return codes


def build_w(st, pos, metric, xp=Numpy):
    """w (B,) float32 of the store under a metric, None under ip"""
    if metric == "ip":
        return None
    w = xp.full((st.B,), background_w(metric), "float32")
    xp.put(w, pos, planted_w(st, len(pos), metric))
    return w


def build(st, pos, metric, xp=Numpy):
    return build_codes(st, pos, xp), build_w(st, pos, metric, xp)


# ------------------------------------------------------------------ the reference: compact store plus background tail
def compact_scores(st, T, count, metric):
    """(Q, count) float32: the scores of the planted rows in ascending position"""
    return mg.restate_metric_scores(T, planted_w(st, count, metric), digits(st, count), metric)


def separated(st, T, count):
    """every planted row of every query precedes the background under every metric: the condition on the inputs"""
    return all(float(compact_scores(st, T, count, m).max()) < float(st.bg()) for m in METRICS)


def tail_positions(pos, ranges, count, keep_from=0):
    """the `count` lowest positions of the disjoint, ascending `ranges` [(a, z), ...] that are not planted and not below
    keep_from (fewer where the ranges run out)"""
    out = []
    have = set(int(p) for p in pos)
    for a, z in ranges:
        p = max(int(a), keep_from)
        while p < z and len(out) < count:
            if p not in have:
                out.append(p)
            p += 1
    return np.array(out, dtype=np.int64)


def with_tail(st, top_s, top_i, k, tail):
    """planted results (Q, m) padded by restate with (+inf, -1) -> (Q, k): the entries without a candidate become the
    background rows of `tail` (one array for all queries, or one per query), then (+inf, -1)"""
    Qn = top_s.shape[0]
    out_s = np.full((Qn, k), np.inf, dtype=np.float32)
    out_i = np.full((Qn, k), -1, dtype=np.int64)
    for q in range(Qn):
        got = top_i[q] >= 0
        n = int(got.sum())
        assert got[:n].all() and n <= k
        t = (tail[q] if isinstance(tail, list) else tail)[:k - n]
        out_s[q, :n], out_i[q, :n] = top_s[q, :n], top_i[q, :n]
        out_s[q, n:n + len(t)], out_i[q, n:n + len(t)] = st.bg(), t
    return out_s, out_i


def reference_topk(st, T, pos, k, metric, kept=None, keep_from=0, B=None):
    """top-k over the whole store: kept (bool per planted row) is the mask over the planted rows; the background is kept from
    row keep_from on"""
    B = st.B if B is None else B
    n = len(pos)
    kept = np.ones(n, dtype=bool) if kept is None else kept
    top_s, top_i = kg.compact_topk(T, planted_w(st, n, metric), digits(st, n), min(k, n), metric, kept)
    top_i = np.where(top_i >= 0, pos[np.maximum(top_i, 0)], -1)
    return with_tail(st, top_s, top_i, k, tail_positions(pos, [(0, B)], k, keep_from))


def thresholds(st, T, count, metric):
    """search_range_grid.thresholds_for on the planted scores, started at mode 3 so that no query takes +inf: halfway between
    two ranks, the score of rank 10, -inf, ... -- all below the background, which is therefore never listed"""
    thr = rg.thresholds_for(compact_scores(st, T, count, metric), q_first=3)
    assert (thr < st.bg()).all()
    return thr


def reference_range(st, T, pos, metric, thr, kept=None):
    n = len(pos)
    kept = np.ones(n, dtype=bool) if kept is None else kept
    lims, p, v = kg.compact_range(T, planted_w(st, n, metric), digits(st, n), metric, kept, thr)
    return lims, pos[p], v


# ------------------------------------------------------------------ lists over a big store
def list_layout(st):
    """9 lists that cover [0, B) with borders at 2^25 - 1, 2^25 + 1 and 2^26 (scaled with the store: B / 2 and B on the
    miniature), and three probe rows: every list, the two lists around 2^25 in descending order, none"""
    B = st.B
    half = 2 ** 25 if B > 2 ** 26 else B // 4
    off = np.array([0, 70, half - half // 8, half - 1, half + 1, half + half // 2, 2 * half, 2 * half + 64, B - 1, B], dtype=np.int64)
    assert (np.diff(off) > 0).all() and len(off) == 10
    L = 9
    probes = np.full((Q, L), -1, dtype=np.int32)
    probes[0] = np.random.RandomState(st.seed).permutation(L)
    probes[1, :2] = [3, 2]                                           # [half - 1, half + 1) and the list below it, descending
    return off, probes


def compact_offsets(pos, off):
    """the list offsets of the compact store: planted row j lies in list l iff off[l] <= pos[j] < off[l + 1]"""
    return np.searchsorted(pos, off, side="left").astype(np.int64)


def reference_lists(st, T, pos, off, probes, k, metric, bias=None):
    """rules 13-15 (and 21 with a bias (Q, P)) over the whole store.  With a bias the background of slot p scores
    finish(1000 * N + bias[q][p]): the tail is taken from the slots in ascending (score, position)."""
    n = len(pos)
    w = planted_w(st, n, metric)
    off_c = compact_offsets(pos, off)
    S = mg.restate_sums(T, digits(st, n))
    b = np.zeros(probes.shape, dtype=np.float32) if bias is None else bias
    s = np.full(S.shape, np.nan, dtype=np.float32)
    for q, row in enumerate(probes):
        for p, l in enumerate(row):
            if 0 <= int(l) < len(off) - 1:
                at = slice(off_c[int(l)], off_c[int(l) + 1])
                Sb = S[q, at] if bias is None else (S[q, at] + b[q, p]).astype(np.float32)
                s[q, at] = Sb if w is None else ((Sb + w[at]) if metric == "l2" else (Sb * w[at])).astype(np.float32)
    top_s, top_i = lg.restate_lists(s, off_c, probes, min(k, n))
    top_i = np.where(top_i >= 0, pos[np.maximum(top_i, 0)], -1)
    out_s = np.full((len(probes), k), np.inf, dtype=np.float32)
    out_i = np.full((len(probes), k), -1, dtype=np.int64)
    bgw = None if metric == "ip" else np.float32(background_w(metric))
    for q, row in enumerate(probes):
        m = int((top_i[q] >= 0).sum())
        out_s[q, :m], out_i[q, :m] = top_s[q, :m], top_i[q, :m]
        slots = []
        for p, l in enumerate(row):
            if 0 <= int(l) < len(off) - 1:
                sb = st.bg() if bias is None else np.float32(st.bg() + b[q, p])
                sc = sb if bgw is None else (np.float32(sb + bgw) if metric == "l2" else np.float32(sb * bgw))
                assert m == 0 or top_s[q, m - 1] < sc
                slots.append((float(sc), int(off[int(l)]), int(off[int(l) + 1])))
        slots.sort()
        at = m
        for sc, a, z in slots:                                       # the background of the cheapest slot first; slots of equal
            t = tail_positions(pos, [(a, z)], k - at)               # score come by their begin, and the lists are disjoint: a
            out_s[q, at:at + len(t)], out_i[q, at:at + len(t)] = np.float32(sc), t      # slot is used up before the next one, so
            at += len(t)                                             # equal scores are listed in ascending position
    return out_s, out_i


def reference_range_lists(st, T, pos, off, probes, metric, thr):
    """rules 17 and 18: the hits of a row's lists in the order of the row, planted rows only (thr is below the background)"""
    import search_range_lists_grid as rl
    n = len(pos)
    s = compact_scores(st, T, n, metric)
    lims, p, v = rl.restate_range_lists(s, compact_offsets(pos, off), probes, thr)
    return lims, pos[p], v


# ------------------------------------------------------------------ a store whose loads wrap, in numpy
def wrapped(st, codes, wrap_row):
    """the codes a kernel sees whose byte offset b * N wrapped at wrap_row * N: codes[(b * N) % wrap] row by row"""
    flat = codes.reshape(-1)
    at = (np.arange(st.B, dtype=np.int64)[:, None] * st.N) % (wrap_row * st.N) + np.arange(st.N)[None, :]
    return flat[at]
