"""The first stage of every search entry (k_search_tables, k_code_norms, rnorm_of of quantization_amd/csrc/mcq_search_kernels.h;
include/mcq.h rules 1, 2 and 6): the numpy restatement of the tables and of the norms, operation by operation, and the case
table of tests/test_gpu_search_tables.py.  tests/search_grid.py restates rules 3 and 4 FROM the tables and norms the device
returned; this file restates those two arrays themselves, from the padded rows of `prepared` and the queries alone.

    T[q][r]  = f32(-2 * acc),  acc = +0, then for d = 0 .. Dp - 1 in turn  acc = f32(acc + f32(q[d] * C[r][d]))       (rule 1)
               fp16 queries widen to fp32 first; q[d] = +0 for d >= D: the pad columns are part of the chain (their products
               are zeros of either sign and NaN where the chain already is one, nothing else)
    t[b]     = v[d] = ((C[0][c_0][d] + C[1][c_1][d]) + ...), digits masked with K - 1; lane l of 64 takes the float4 groups
               l, l + 64, ... in turn, part = f32(part + f32(v[d] * v[d])) over a group's four components, part starting at
               +0; then the xor butterfly 32, 16, 8, 4, 2, 1                                                          (rule 2)
    r[b]     = search_metric_grid.restate_rnorms(t)                                                                   (rule 6)

Each case below CLAIMS the paths of the two kernels it reaches; tests/test_search_tables_host.py checks the claims against the
constants read from the source (search_grid.constants), so a moved constant fails there instead of hollowing out the GPU cases."""
from dataclasses import dataclass

import numpy as np

import search_grid as sg
from search_metric_grid import restate_rnorms          # noqa: F401  (rule 6: the tests of this stage take it from here)

TAB_THREADS = 256                                       # __launch_bounds__ of k_search_tables


# ------------------------------------------------------------------ rule 1 in numpy
def widen(q):
    """queries as the kernel reads them: fp16 widens exactly, anything else must be float32 already"""
    q = np.asarray(q)
    assert q.dtype in (np.float32, np.float16), q.dtype
    return q.astype(np.float32)


def restate_tables(q, Cp):
    """q (Q, D) float32 or float16, Cp (N, K, Dp) float32 -- the PADDED rows of `prepared` -- -> float32 (Q, N * K)"""
    q = widen(q)
    N, K, Dp = Cp.shape
    Q, D = q.shape
    assert Dp == sg.padded(D)
    Ct = np.ascontiguousarray(Cp.reshape(N * K, Dp).T)                # (Dp, NK): one contiguous row per feature
    qt = np.zeros((Dp, Q, 1), dtype=np.float32)
    qt[:D, :, 0] = q.T
    acc = np.zeros((Q, N * K), dtype=np.float32)
    prod = np.empty_like(acc)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(Dp):
            np.multiply(qt[d], Ct[d][None, :], out=prod)              # each product rounded to float32 ...
            np.add(acc, prod, out=acc)                                # ... then added: two operations, never one
        return np.multiply(acc, np.float32(-2.0), out=acc)


# ------------------------------------------------------------------ rule 2 in numpy
def row_sums(Cp, codes):
    """v of rule 2: (B, Dp) float32, the rows of the digits added n ascending (N - 1 additions per feature)"""
    N, K, Dp = Cp.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v = Cp[0][codes[:, 0].astype(np.int64) & (K - 1)].astype(np.float32)
        for n in range(1, N):
            v = (v + Cp[n][codes[:, n].astype(np.int64) & (K - 1)]).astype(np.float32)
    return v


def lane_sums(v, masks=(32, 16, 8, 4, 2, 1)):
    """sum_d v[d]^2 as rule 2 orders it: v (B, Dp) float32 -> float32 (B,).  masks: the butterfly's levels in turn"""
    B, Dp = v.shape
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sq = (v * v).astype(np.float32)
        groups = Dp // 4
        part = np.zeros((B, 64), dtype=np.float32)
        lanes = np.arange(64)
        for g0 in range(0, groups, 64):                              # lane l: the float4 groups l, l + 64, ... in turn
            g = g0 + lanes
            live = g < groups
            for c in range(4):
                term = np.zeros((B, 64), dtype=np.float32)
                term[:, live] = sq[:, 4 * g[live] + c]
                part = (part + term).astype(np.float32)
        for m in masks:                                              # the xor butterfly: every lane ends with the same sum
            part = (part + part[:, lanes ^ m]).astype(np.float32)
    return part[:, 0].copy()


def restate_norms(Cp, codes):
    """Cp (N, K, Dp) float32 -- the PADDED rows of `prepared` --, codes (B, N) -> float32 (B,)"""
    return lane_sums(row_sums(Cp, codes))


# ------------------------------------------------------------------ the float64 bounds of tests/test_gpu_search.py
EPS = 2.0 ** -24


def tables_bound(q, Cp, D):
    """(float64 reference (Q, NK), bound (Q, NK)) of test_gpu_search._check_tables: 2 * L * 2^-24 * S, S = 2 sum_d |q[d]| |C[r][d]|,
    L the padded dim"""
    N, K, Dp = Cp.shape
    q64, C64 = widen(q).astype(np.float64), Cp[:, :, :D].astype(np.float64).reshape(N * K, D)
    return -2.0 * q64 @ C64.T, 2 * sg.tables_chain(D) * EPS * (2.0 * np.abs(q64) @ np.abs(C64).T)


def norms_bound(Cp, codes, D):
    """(float64 reference (B,), bound (B,)) of test_gpu_search._check_norms: 4 * L * 2^-24 * sum_d (sum_n |C[n][c_n][d]|)^2, L the
    longer of the row-addition chain and the accumulation chain"""
    N, K, Dp = Cp.shape
    C64 = Cp[:, :, :D].astype(np.float64)
    dec, mag = np.zeros((len(codes), D)), np.zeros((len(codes), D))
    for n in range(N):
        col = codes[:, n].astype(np.int64) & (K - 1)
        dec += C64[n][col]
        mag += np.abs(C64[n])[col]
    return (dec ** 2).sum(1), 4 * max(sg.norms_chains(N, D)) * EPS * (mag ** 2).sum(1)


# ------------------------------------------------------------------ the paths of the two kernels
def tables_paths(N, K, D, Q, c):
    """what a launch of k_search_tables reaches, from the mirrored constants"""
    Dp, chunk, rows, tile = sg.padded(D), c["kTabChunk"], c["kTabRows"], c["kTabQueries"]
    own = tile // (TAB_THREADS // rows)                  # queries a thread owns: 4g .. 4g + 3
    return dict(small=Dp < chunk,                        # the only chunk is a partial one (Dp % chunk != 0)
                half_last=Dp > chunk and Dp % chunk != 0,  # the last of several chunks is a partial one
                ragged=D % 16 != 0,                      # d0 + dd < D and d0 + dd < Dp differ
                chunks=(Dp + chunk - 1) // chunk,
                row_blocks=(N * K + rows - 1) // rows,
                rows_short=(N * K) % rows != 0,          # a row block with rows past N * K
                qtiles=(Q + tile - 1) // tile,
                q_part=Q % own != 0,                     # a thread with fewer than its `own` queries
                q_tile_part=Q % tile != 0)               # threads of the last tile with none


def norms_paths(N, K, D, B, c):
    """what a launch of k_code_norms reaches"""
    groups = sg.padded(D) // 4
    return dict(groups=groups,                           # float4 groups of a padded row: a multiple of 4 ...
                data_groups=(D + 3) // 4,                # ... of which these hold a feature (63 of 64 at D = 252, 65 of 68 at 260)
                trips=(groups + 63) // 64,
                lanes_idle=groups % 64 != 0,             # lanes without a float4 group in the last trip
                no_row_add=N == 1, all_lanes_digits=N == 64,
                blocks=(B + c["kNormWaves"] - 1) // c["kNormWaves"],
                b_part=B % c["kNormWaves"] != 0)         # waves of the last workgroup past B


@dataclass(frozen=True)
class TabCase:
    name: str
    N: int
    K: int
    D: int
    Q: int
    fp16: bool = False
    small: bool = False                                  # claims, in the order of tables_paths
    half_last: bool = False
    ragged: bool = False
    chunks: int = 1
    row_blocks: int = 1
    rows_short: bool = False
    qtiles: int = 1
    q_part: bool = False
    q_tile_part: bool = False


@dataclass(frozen=True)
class NormCase:
    name: str
    N: int
    K: int
    D: int
    B: int
    codes: str = "random"                                # "random": digits below K | "bytes": 0 .. 255 (K = 16: the mask of rule 2)
    groups: int = 4                                      # claims, in the order of norms_paths
    data_groups: int = 4
    trips: int = 1
    lanes_idle: bool = False
    no_row_add: bool = False
    all_lanes_digits: bool = False
    blocks: int = 1
    b_part: bool = False


TAB_FLAGS = ("small", "half_last", "ragged", "chunks", "row_blocks", "rows_short", "qtiles", "q_part", "q_tile_part")
NORM_FLAGS = ("groups", "data_groups", "trips", "lanes_idle", "no_row_add", "all_lanes_digits", "blocks", "b_part")

TAB_CASES = [
    TabCase("d1_1x16_q1", 1, 16, 1, 1, small=True, ragged=True, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d15_2x16_q3_h", 2, 16, 15, 3, fp16=True, small=True, ragged=True, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d16_1x64_q4", 1, 64, 16, 4, small=True, q_tile_part=True),
    TabCase("d16_2x16_q5_h", 2, 16, 16, 5, fp16=True, small=True, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d17_2x16_q5_h", 2, 16, 17, 5, fp16=True, ragged=True, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d31_1x16_q15", 1, 16, 31, 15, ragged=True, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d32_1x64_q16_h", 1, 64, 32, 16, fp16=True),
    TabCase("d32_2x16_q16", 2, 16, 32, 16, rows_short=True),
    TabCase("d33_8x256_q17", 8, 256, 33, 17, half_last=True, ragged=True, chunks=2, row_blocks=32, qtiles=2, q_part=True,
            q_tile_part=True),
    TabCase("d40_8x256_q33_h", 8, 256, 40, 33, fp16=True, half_last=True, ragged=True, chunks=2, row_blocks=32, qtiles=3,
            q_part=True, q_tile_part=True),
    TabCase("d48_2x16_q16", 2, 16, 48, 16, half_last=True, chunks=2, rows_short=True),
    TabCase("d49_1x64_q5_h", 1, 64, 49, 5, fp16=True, ragged=True, chunks=2, q_part=True, q_tile_part=True),
    TabCase("d260_8x256_q17_h", 8, 256, 260, 17, fp16=True, half_last=True, ragged=True, chunks=9, row_blocks=32, qtiles=2,
            q_part=True, q_tile_part=True),
    TabCase("d260_1x64_q3", 1, 64, 260, 3, half_last=True, ragged=True, chunks=9, q_part=True, q_tile_part=True),
    TabCase("d512_8x256_q33", 8, 256, 512, 33, chunks=16, row_blocks=32, qtiles=3, q_part=True, q_tile_part=True),
    TabCase("d512_2x16_q15_h", 2, 16, 512, 15, fp16=True, chunks=16, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d1000_1x64_q3_h", 1, 64, 1000, 3, fp16=True, half_last=True, ragged=True, chunks=32, q_part=True, q_tile_part=True),
    TabCase("d1000_2x16_q1", 2, 16, 1000, 1, half_last=True, ragged=True, chunks=32, rows_short=True, q_part=True,
            q_tile_part=True),
    TabCase("d16384_1x16_q3", 1, 16, 16384, 3, chunks=512, rows_short=True, q_part=True, q_tile_part=True),
    TabCase("d24_64x256_q17", 64, 256, 24, 17, ragged=True, row_blocks=256, qtiles=2, q_part=True, q_tile_part=True),
]

NORM_CASES = [
    NormCase("d1_1x16_b1", 1, 16, 1, 1, groups=4, data_groups=1, lanes_idle=True, no_row_add=True, b_part=True),
    NormCase("d16_2x16_b3_bytes", 2, 16, 16, 3, codes="bytes", groups=4, data_groups=4, lanes_idle=True, b_part=True),
    NormCase("d17_8x16_b4_bytes", 8, 16, 17, 4, codes="bytes", groups=8, data_groups=5, lanes_idle=True),
    NormCase("d252_2x64_b5", 2, 64, 252, 5, groups=64, data_groups=63, blocks=2, b_part=True),
    NormCase("d256_64x256_b300", 64, 256, 256, 300, groups=64, data_groups=64, all_lanes_digits=True, blocks=75),
    NormCase("d260_8x256_b300", 8, 256, 260, 300, groups=68, data_groups=65, trips=2, lanes_idle=True, blocks=75),
    NormCase("d260_1x16_b3", 1, 16, 260, 3, groups=68, data_groups=65, trips=2, lanes_idle=True, no_row_add=True, b_part=True),
    NormCase("d512_64x16_b5_bytes", 64, 16, 512, 5, codes="bytes", groups=128, data_groups=128, trips=2, all_lanes_digits=True,
             blocks=2, b_part=True),
    NormCase("d1000_2x64_b300", 2, 64, 1000, 300, groups=252, data_groups=250, trips=4, lanes_idle=True, blocks=75),
    NormCase("d16384_1x16_b5", 1, 16, 16384, 5, groups=4096, data_groups=4096, trips=64, no_row_add=True, blocks=2, b_part=True),
    NormCase("d16384_8x16_b3_bytes", 8, 16, 16384, 3, codes="bytes", groups=4096, data_groups=4096, trips=64, b_part=True),
]

# the end-to-end cases: search under the three metrics from the RESTATED tables and norms, (N, K, D, Q, B, k)
END_TO_END = ((8, 256, 40, 17, 4099, 10), (2, 64, 1000, 5, 300, 10))


# ------------------------------------------------------------------ inputs (numpy only, the same on the host and on the device)
def state(N, K, D):
    """the synthetic state of a case, as tests/test_gpu_search._quantizer seeds it"""
    from quantization_amd import synthetic as gen
    return gen.synthetic_state(11 + N + K, D, K, N)


def host_centers(N, K, D):
    """the padded fp32 centers of that state as a host can form them, (N, K, Dp): centers * f32(exp(10 * centers_scale)).  The GPU
    tests read the rows out of `prepared` instead; the host tests need rows of the same size and spread, no more"""
    sd = state(N, K, D)
    Cp = np.zeros((N, K, sg.padded(D)), dtype=np.float32)
    Cp[:, :, :D] = sd["centers"] * np.float32(np.exp(10.0 * float(sd["centers_scale"])))
    return Cp


def queries(case):
    """(Q, D) float32, or float16 where the case says so"""
    from quantization_amd import synthetic as gen
    x = gen.make_gaussian(177 + case.Q + case.D, case.Q, case.D)
    return x.astype(np.float16) if case.fp16 else x


def codes(case):
    """(B, N) uint8: digits below K, or any byte where the case says so"""
    rs = np.random.RandomState(500 + case.B + case.N + case.D)
    hi = 256 if case.codes == "bytes" else case.K
    out = rs.randint(0, hi, size=(case.B, case.N)).astype(np.uint8)
    if case.codes == "bytes":
        assert case.K == 16
        out[0, 0] |= 0xF0                                            # a digit past K - 1 whatever the draw
    return out


# ------------------------------------------------------------------ mutations: what a bit-for-bit comparison must be able to see
def mutate_tables(q, Cp, how):
    """restate_tables with ONE thing changed -> float32 (Q, NK):
         "fma"       acc = f32(acc + q[d] * C[d]) rounded once (the product and the sum in float64: both exact there up to the one
                     rounding of the sum, far below float32's), what -ffp-contract=fast or fmaf would give
         "two_acc"   even d and odd d in two accumulators, added at the end
         "neg_zero"  the accumulator starts at -0.0"""
    q = widen(q)
    N, K, Dp = Cp.shape
    Q, D = q.shape
    C2 = Cp.reshape(N * K, Dp)
    qp = np.zeros((Q, Dp), dtype=np.float32)
    qp[:, :D] = q
    acc = np.zeros((2, Q, N * K), dtype=np.float32)
    if how == "neg_zero":
        acc[0] = -0.0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for d in range(Dp):
            a = acc[d & 1] if how == "two_acc" else acc[0]
            if how == "fma":
                a[...] = (a.astype(np.float64) + qp[:, d, None].astype(np.float64) * C2[None, :, d].astype(np.float64)).astype(np.float32)
            else:
                a[...] = a + (qp[:, d, None] * C2[None, :, d]).astype(np.float32)
        total = (acc[0] + acc[1]).astype(np.float32) if how == "two_acc" else acc[0]
        return (total * np.float32(-2.0)).astype(np.float32)


def mutate_norms(Cp, codes_, how):
    """restate_norms with ONE thing changed -> float32 (B,):
         "fma"        part = f32(part + v * v) rounded once
         "ascending"  the butterfly in the order 1, 2, 4, 8, 16, 32"""
    v = row_sums(Cp, codes_)
    if how == "ascending":
        return lane_sums(v, masks=(1, 2, 4, 8, 16, 32))
    assert how == "fma"
    B, Dp = v.shape
    groups, lanes = Dp // 4, np.arange(64)
    part = np.zeros((B, 64), dtype=np.float32)
    v64 = v.astype(np.float64)
    for g0 in range(0, groups, 64):
        g = g0 + lanes
        live = g < groups
        for c in range(4):
            term = np.zeros((B, 64))
            term[:, live] = v64[:, 4 * g[live] + c] ** 2
            part = (part.astype(np.float64) + term).astype(np.float32)
    for m in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, lanes ^ m]).astype(np.float32)
    return part[:, 0].copy()


def bits_differ(a, b):
    """entries whose bits differ, two NaN counting as equal"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())
