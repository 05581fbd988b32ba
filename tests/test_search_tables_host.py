"""Host-side checks of tests/search_tables_grid.py (no GPU): the claims of its case tables against the constants of
mcq_search_kernels.h, the two restatements against scalar loops written straight from rules 1 and 2 of include/mcq.h and
against the float64 bounds of tests/test_gpu_search.py, and their SENSITIVITY: a fused multiply-add, a chain split over two
accumulators, a butterfly run the other way and an accumulator started at -0.0 each change bits on the inputs of the cases --
otherwise a bit-for-bit GPU comparison would prove less than it seems to."""
import functools
import time

import numpy as np
import pytest

import search_bias_grid as bg
import search_grid as sg
import search_tables_grid as tg

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _centers(N, K, D):
    return tg.host_centers(N, K, D)


# ------------------------------------------------------------------ the claims
def test_table_cases_reach_what_they_claim():
    c = sg.constants()
    assert tg.TAB_THREADS % c["kTabRows"] == 0 and c["kTabQueries"] % (tg.TAB_THREADS // c["kTabRows"]) == 0
    own = c["kTabQueries"] // (tg.TAB_THREADS // c["kTabRows"])
    for x in tg.TAB_CASES:
        got = tg.tables_paths(x.N, x.K, x.D, x.Q, c)
        assert got == {f: getattr(x, f) for f in tg.TAB_FLAGS}, (x.name, got)
        assert x.N * x.K <= 16384 and x.K in (16, 64, 256) and x.D <= 16384            # the domain of the library
    cases = tg.TAB_CASES
    # every class of the padded dim, with fp32 and with fp16 queries
    for flag in ("small", "half_last", "ragged"):
        assert {x.fp16 for x in cases if getattr(x, flag)} == {False, True}, flag
    assert {x.fp16 for x in cases if x.chunks >= 8} == {False, True}                   # many chunks
    assert {x.fp16 for x in cases if not x.small and not x.half_last and not x.ragged} == {False, True}     # whole chunks only
    assert any(x.small and not x.ragged for x in cases) and any(x.half_last and not x.ragged for x in cases)
    assert {x.D for x in cases} >= {1, 15, 16, 17, 31, 32, 33, 40, 48, 49, 260, 512, 1000, 16384}
    assert max(x.chunks for x in cases) == 16384 // c["kTabChunk"]
    # queries on both sides of a thread's group and of the tile
    assert {x.Q for x in cases} >= {1, own - 1, own, own + 1, c["kTabQueries"] - 1, c["kTabQueries"], c["kTabQueries"] + 1,
                                    2 * c["kTabQueries"] + 1}
    assert {x.qtiles for x in cases} >= {1, 2, 3}
    # rows: fewer than a block, half of one, exactly one, many
    assert {x.N * x.K for x in cases} >= {c["kTabRows"] // 4, c["kTabRows"] // 2, c["kTabRows"], 2048, 16384}
    assert max(x.row_blocks for x in cases) == 16384 // c["kTabRows"]


def test_norm_cases_reach_what_they_claim():
    c = sg.constants()
    for x in tg.NORM_CASES:
        got = tg.norms_paths(x.N, x.K, x.D, x.B, c)
        assert got == {f: getattr(x, f) for f in tg.NORM_FLAGS}, (x.name, got)
        assert x.N * x.K <= 16384 and x.K in (16, 64, 256) and x.D <= 16384
        assert sg.norms_chains(x.N, x.D)[1] == 4 * x.trips + 6
        if x.codes == "bytes":
            assert x.K == 16 and (tg.codes(x) >= 16).any()                             # the mask of rule 2 has something to do
    cases = tg.NORM_CASES
    assert {x.D for x in cases} >= {1, 16, 17, 252, 256, 260, 512, 1000, 16384}
    assert {x.groups for x in cases} >= {4, 64, 68} and {x.data_groups for x in cases} >= {63, 64, 65}
    assert {x.trips for x in cases} >= {1, 2, 64}
    assert {x.N for x in cases} == {1, 2, 8, 64}
    w = c["kNormWaves"]
    assert {x.B for x in cases} >= {1, w - 1, w, w + 1, 300}
    assert any(x.no_row_add for x in cases) and any(x.all_lanes_digits for x in cases) and any(x.codes == "bytes" for x in cases)
    assert {x.lanes_idle for x in cases} == {False, True}
    # the end-to-end cases are the two added to the table of tests/search_grid.py
    shapes = {(s.N, s.K, s.D, s.Q, s.B, s.k) for s in sg.CASES}
    assert set(tg.END_TO_END) <= shapes and {e[2] for e in tg.END_TO_END} == {40, 1000}


# ------------------------------------------------------------------ the restatements against the rules' text
def _tables_by_the_text(q, Cp):
    """rule 1 with np.float32 scalars: three loops"""
    q = q.astype(np.float32)
    N, K, Dp = Cp.shape
    Q, D = q.shape
    C2 = Cp.reshape(N * K, Dp)
    out = np.empty((Q, N * K), dtype=np.float32)
    for a in range(Q):
        for r in range(N * K):
            acc = f32(0.0)
            for d in range(Dp):
                qd = q[a, d] if d < D else f32(0.0)
                acc = f32(acc + f32(qd * C2[r, d]))
            out[a, r] = f32(f32(-2.0) * acc)
    return out


def _norms_by_the_text(Cp, codes):
    """rule 2 with np.float32 scalars: 64 lane accumulators, then the six levels of the butterfly"""
    N, K, Dp = Cp.shape
    out = np.empty(len(codes), dtype=np.float32)
    for b in range(len(codes)):
        lane = [f32(0.0)] * 64
        for g in range(Dp // 4):
            for c in range(4):
                d = 4 * g + c
                v = Cp[0, int(codes[b, 0]) & (K - 1), d]
                for n in range(1, N):
                    v = f32(v + Cp[n, int(codes[b, n]) & (K - 1), d])
                lane[g % 64] = f32(lane[g % 64] + f32(v * v))
        for m in (32, 16, 8, 4, 2, 1):
            lane = [f32(lane[l] + lane[l ^ m]) for l in range(64)]
        assert len({x.tobytes() for x in lane}) == 1                                   # every lane ends with the same bits
        out[b] = lane[0]
    return out


@pytest.mark.parametrize("D", (1, 17, 40))
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
def test_restate_tables_is_rule_1(D, half):
    Cp = _centers(2, 16, D)
    q = np.random.RandomState(D).standard_normal((3, D)).astype(np.float16 if half else np.float32)
    assert tg.bits_differ(tg.restate_tables(q, Cp), _tables_by_the_text(q, Cp)) == 0
    zero = np.zeros((1, D), dtype=q.dtype)
    T = tg.restate_tables(zero, Cp)
    assert (T == 0).all() and np.signbit(T).all()                                      # -2 * (+0): every entry is -0.0


@pytest.mark.parametrize("shape", ((1, 16, 1), (2, 16, 17), (2, 16, 40), (8, 16, 260)), ids=lambda s: "n%d_k%d_d%d" % s)
def test_restate_norms_is_rule_2(shape):
    N, K, D = shape
    Cp = _centers(N, K, D)
    codes = np.random.RandomState(D).randint(0, 256, size=(4, N)).astype(np.uint8)     # any byte: the mask is part of the rule
    want = _norms_by_the_text(Cp, codes)
    assert tg.bits_differ(tg.restate_norms(Cp, codes), want) == 0
    assert tg.bits_differ(bg.restate_norms_based(Cp, codes, None, None, D), want) == 0
    assert tg.bits_differ(tg.restate_norms(Cp, codes & (K - 1)), want) == 0


def test_restatements_lie_within_the_float64_bounds():
    """the derived bounds of tests/test_gpu_search.py (_check_tables, _check_norms), on every case"""
    for x in tg.TAB_CASES:
        Cp, q = _centers(x.N, x.K, x.D), tg.queries(x)
        ref, bound = tg.tables_bound(q, Cp, x.D)
        assert (np.abs(tg.restate_tables(q, Cp).astype(np.float64) - ref) <= bound).all(), x.name
    for x in tg.NORM_CASES:
        Cp, codes = _centers(x.N, x.K, x.D), tg.codes(x)
        ref, bound = tg.norms_bound(Cp, codes, x.D)
        assert (np.abs(tg.restate_norms(Cp, codes).astype(np.float64) - ref) <= bound).all(), x.name


def test_restate_tables_is_quick():
    """33 queries against 16,384 rows of 512 features, the largest table the domain of the library has at that dim, restate in
    a couple of seconds (a GPU case forms its reference once)"""
    rs = np.random.RandomState(0)
    Cp, q = rs.standard_normal((64, 256, 512)).astype(np.float32), rs.standard_normal((33, 512)).astype(np.float32)
    t0 = time.perf_counter()
    T = tg.restate_tables(q, Cp)
    assert time.perf_counter() - t0 < 4.0
    assert T.shape == (33, 16384) and T.dtype == np.float32


# ------------------------------------------------------------------ sensitivity
def test_mutations_change_bits_on_the_case_inputs():
    """Per mutation the entries that change, over all cases: > 0, and > 0 in EVERY table case whose chain has 16 real terms or
    more and in every norm case of 300 vectors (a chain of one term has no order and no second rounding to lose: D = 1 cannot
    tell any of them apart)."""
    seen = {"fma": 0, "two_acc": 0}
    for x in tg.TAB_CASES:
        Cp, q = _centers(x.N, x.K, x.D), tg.queries(x)
        want = tg.restate_tables(q, Cp)
        for how in seen:
            n = tg.bits_differ(tg.mutate_tables(q, Cp, how), want)
            seen[how] += n
            assert n > 0 or x.D < 16, (x.name, how)
    assert all(v > 0 for v in seen.values()), seen
    seen = {"fma": 0, "ascending": 0}
    for x in tg.NORM_CASES:
        Cp, codes = _centers(x.N, x.K, x.D), tg.codes(x)
        want = tg.restate_norms(Cp, codes)
        for how in seen:
            n = tg.bits_differ(tg.mutate_norms(Cp, codes, how), want)
            seen[how] += n
            assert n > 0 or x.B < 300, (x.name, how)                 # (a norm's sum absorbs most changes of one term: of a handful
                                                                     # of vectors none may change, of 300 dozens do)
    assert all(v > 0 for v in seen.values()), seen


def test_a_negative_zero_start_shows_only_where_every_product_is_a_negative_zero():
    """acc = -0.0 at the start: +0 returns with the first product that is not -0 -- a pad column, a chunk's tail, any q[d] * C[d]
    that is not a negative zero.  So the mutation shows in a zero entry of a dim that is a multiple of the chunk, all of whose
    products are -0: a zero query against a row of negative centers, the edge the GPU test builds by hand."""
    c = sg.constants()
    D = c["kTabChunk"]
    Cp = np.abs(_centers(2, 16, D))
    Cp[1] = -Cp[1]
    q = np.zeros((2, D), dtype=np.float32)
    q[1] = -0.0
    want = tg.restate_tables(q, Cp)
    assert (want == 0).all() and np.signbit(want).all()
    got = tg.mutate_tables(q, Cp, "neg_zero")
    flipped = (~np.signbit(got)).reshape(2, 2, 16)
    assert flipped[0, 1].all() and flipped[1, 0].all() and not flipped[0, 0].any() and not flipped[1, 1].any()
    # on random data it never shows: the GPU cases of the table cannot see it, the hand-made edge must
    for x in tg.TAB_CASES[:8]:
        Cp, q = _centers(x.N, x.K, x.D), tg.queries(x)
        assert tg.bits_differ(tg.mutate_tables(q, Cp, "neg_zero"), tg.restate_tables(q, Cp)) == 0
