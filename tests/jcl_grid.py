"""The three kernels behind JointCodebookLoss restated in numpy, and the cases tests/test_gpu_jcl_kernels.py runs them on.

mcq_jcl_prefix_fwd, mcq_jcl_prefix_bwd and mcq_scatter_rows (include/mcq.h; k_jcl_prefix_fwd / k_jcl_prefix_bwd in
mcq_loss_kernels.h, k_decode_backward<int64_t, CW> in mcq_kernels.h) each appear twice here:

* `*32`: fp32, one numpy operation per operation of the kernel, in the kernel's order.  The library is built with
  -ffp-contract=off, so each kernel is a fixed sequence of individually rounded fp32 operations and the restatement must
  agree with it bit for bit (zeros by value: fmaxf may return either zero).
* `*64`: float64, with a bound per entry on what any fp32 evaluation in that order can differ by.  u = 2^-24 throughout.

No GPU and no library call in this file: host tests (tests/test_jcl_grid_host.py) and GPU tests import it.
"""
from collections import namedtuple

import numpy as np

import train_grid as tg

U = 2.0 ** -24


def jcl_scale(H, N):
    """first_embeddings_scale of the reference (prediction.py:52) as the kernels receive it: rounded to fp32"""
    return float(np.float32(0.5 * ((H / N) ** 0.5)))


# ---------------------------------------------------------------------------------------------- prefix, forward
def _prefix_fwd(hp, emb, idx, K, scale, dt):
    B, H = hp.shape
    N = idx.shape[1]
    sc = dt(scale)
    s = hp.astype(dt)
    mag = np.abs(s)
    A, S = np.empty((N, B, H), dt), np.empty((N, B, H), dt)
    A[0], S[0] = np.maximum(s, dt(0)), mag
    for n in range(1, N):
        k = np.maximum(idx[:, n - 1], 0)                      # k < 0 ? 0 : k
        p = emb[(n - 1) * K + k].astype(dt) * sc              # the product is rounded on its own ...
        s = s + p                                             # ... then the sum
        mag = mag + np.abs(p)
        A[n], S[n] = np.maximum(s, dt(0)), mag
    return A, S


def prefix_fwd32(hp, emb, idx, K, scale):
    """A [N][B][H] fp32 in the kernel's order: s_0 = hp[b], s_n = s_{n-1} + fl(emb[(n-1) K + max(idx[b][n-1], 0)] * scale),
    A[n][b] = max(s_n, 0).  The last index column is never read."""
    return _prefix_fwd(hp, emb, idx, K, scale, np.float32)[0]


def prefix_fwd64(hp, emb, idx, K, scale):
    """-> (A in float64, bound); bound[n][b][h] = (n + 1) u (|hp| + sum_{m <= n} |emb * scale|).

    Derivation.  s_n is a recursive sum of n + 1 terms: hp (exact) and n products, each rounded once:
    |fl(p) - p| <= u |p|.  Recursive summation of n + 1 floating-point terms t_i errs by at most n u sum |t_i| (Rump 2012,
    no higher-order term).  Together: |s_n(fp32) - s_n| <= u sum |p| + n u sum |fl(t_i)| <= (n + 1) u (|hp| + sum |p|),
    up to a factor 1 + u on the second term, which is below the resolution of the float64 comparison's bound itself
    (relative 2^-24 of the bound) and is ignored.  max(., 0) is exact and does not expand distances.  Products that
    underflow would add 2^-150 each; the inputs built here keep them normal, or exact (power-of-two scale)."""
    A, S = _prefix_fwd(hp, emb, idx, K, scale, np.float64)
    n1 = np.arange(1, idx.shape[1] + 1, dtype=np.float64).reshape(-1, 1, 1)
    return A, n1 * U * S


# ---------------------------------------------------------------------------------------------- prefix, backward
def relu_mask(A):
    """m_n / gA[n]: 1 where A > 0, as torch's ReLU backward has it (0 at +0 and -0, 1 at a positive subnormal)"""
    return A > 0


def _prefix_bwd(A, gA, scale, dt):
    N, B, H = A.shape
    sc = dt(scale)
    m = np.where(relu_mask(A), gA.astype(dt), dt(0))          # A is taken as given
    r, mag = np.zeros((B, H), dt), np.zeros((B, H), dt)
    gE, SE = np.empty((N - 1, B, H), dt), np.empty((N - 1, B, H), dt)
    for n in range(N - 1, 0, -1):
        r = r + m[n]
        mag = mag + np.abs(m[n])
        gE[n - 1], SE[n - 1] = r * sc, mag
    return r + m[0], gE, mag + np.abs(m[0]), SE


def prefix_bwd32(A, gA, scale):
    """-> (g_hp [B][H], gE [N-1][B][H]) fp32 in the kernel's order: r = 0; for n = N-1 .. 1: r = r + m_n,
    gE[n-1][b] = fl(r * scale); g_hp = r + m_0, with m_n = gA[n][b] where A[n][b] > 0, else 0."""
    g_hp, gE, _, _ = _prefix_bwd(A, gA, scale, np.float32)
    return g_hp, gE


def prefix_bwd64(A, gA, scale):
    """-> (g_hp, gE, bound of g_hp, bound of gE) in float64; bound = (N + 1) u sum |m| over the terms behind the entry,
    times scale for gE.

    Derivation.  r is a recursive sum of at most N + 1 terms (the initial 0 and m_{N-1} .. m_0, all exact inputs): error at
    most N u sum |m| (Rump 2012).  gE rounds r * scale once more: |fl(r s) - r s| <= u |r| s <= u s sum |m|.  So g_hp is
    within N u sum |m| and gE within (N + 1) u s sum |m|; one bound, (N + 1) u sum |m|, serves both."""
    g_hp, gE, S0, SE = _prefix_bwd(A, gA, scale, np.float64)
    c = (A.shape[0] + 1) * U
    return g_hp, gE, c * S0, c * SE * abs(scale)


# ---------------------------------------------------------------------------------------------- scatter
def _scatter(grad, stride_b, stride_n, idx, idx_stride, B, N, K, D, dt):
    out, mag = np.zeros((N * K, D), dt), np.zeros((N * K, D), dt)
    hits = np.zeros(N * K, np.int64)
    for n in range(N):
        for b in range(B):                                    # ascending b: the kernel's fixed order
            k = int(idx[b * idx_stride + n])
            if 0 <= k < K:                                    # negative indexes match nothing
                o = b * stride_b + n * stride_n
                g = grad[o:o + D].astype(dt)
                out[n * K + k] = out[n * K + k] + g
                mag[n * K + k] = mag[n * K + k] + np.abs(g)
                hits[n * K + k] += 1
    return out, mag, hits


def scatter_rows32(grad, stride_b, stride_n, idx, idx_stride, B, N, K, D):
    """out [N K][D] fp32: out[n K + k][d] = sum over ascending b with idx[b idx_stride + n] == k of
    grad[b stride_b + n stride_n + d], added one at a time to an accumulator that starts at 0 (the kernel adds matches
    eight at a time with zeros in the unused slots; x + 0 is exact).  Rows without a match are exactly 0."""
    return _scatter(grad, stride_b, stride_n, idx, idx_stride, B, N, K, D, np.float32)[0]


def scatter_rows64(grad, stride_b, stride_n, idx, idx_stride, B, N, K, D):
    """-> (out in float64, bound, hits per row); bound[row][d] = hits u sum |g|.

    Derivation.  A row is the recursive sum of its `hits` exact inputs: error at most (hits - 1) u sum |g| (Rump 2012),
    which hits u sum |g| covers; a row without a hit is exactly 0 and its bound is 0."""
    out, mag, hits = _scatter(grad, stride_b, stride_n, idx, idx_stride, B, N, K, D, np.float64)
    return out, hits.reshape(-1, 1) * U * mag, hits


# ---------------------------------------------------------------------------------------------- prefix cases
PREFIX_CASES = [(1, 2, 16, 1), (3, 3, 32, 63), (5, 5, 128, 65), (130, 16, 16, 64), (7, 4, 256, 130), (66, 4, 64, 64)]   # (B, N, K, H)
# feature columns of the special values where scale is a power of two: s_1 exactly +0, exactly -0, a positive subnormal
H_PZERO, H_NZERO, H_SUBNORMAL = 1, 2, 3
SUBNORMAL = np.float32(2.0 ** -140)


def prefix_special_frames(B, N):
    """frames that carry the special values (three, spread over the batch)"""
    return [2, B // 2, B - 1]


def scale_is_power_of_two(H, N):
    s = jcl_scale(H, N)
    return s == 0.5 * ((H / N) ** 0.5) and np.frexp(s)[0] == 0.5


def prefix_inputs(B, N, K, H):
    """-> hp [B][H], emb [(N-1) K][H] fp32, idx [B][N] int64, gA [N][B][H] fp32, scale.

    idx: a negative in every column, the last (never gathered) included, on a diagonal; a zero in every column where the
    batch has a second frame; one in ten of the rest -1.  gA: magnitudes in [0.5, 1.5) times powers of two from 2^-12 to 2^12.  Where
    scale is a power of two (products are exact), in the frames of prefix_special_frames: s_1 = hp + emb * scale is made
    exactly +0 in feature 1 (hp = -(emb * scale)), exactly -0 in feature 2 (both -0), and 2^-140 in feature 3 (hp = 2^-140,
    emb = 0; s_0 is the same subnormal)."""
    rng = np.random.RandomState(1000 * B + 100 * N + K + H)
    scale = jcl_scale(H, N)
    hp = rng.standard_normal((B, H)).astype(np.float32)
    emb = (rng.standard_normal(((N - 1) * K, H)) * H ** -0.5).astype(np.float32)
    idx = rng.randint(0, K, (B, N)).astype(np.int64)
    idx[rng.random_sample((B, N)) < 0.1] = -1
    for j in range(N):
        if B >= 2:
            idx[(j + 1) % B, j] = 0
        idx[j % B, j] = -100
    if scale_is_power_of_two(H, N):
        sc = np.float32(scale)
        for b in prefix_special_frames(B, N):
            idx[b, 0] = 3 + b % 5                              # a valid first entry for these frames
        for b in prefix_special_frames(B, N):
            row = idx[b, 0]
            emb[row, H_NZERO] = np.float32(-0.0)
            emb[row, H_SUBNORMAL] = np.float32(0.0)
        for b in prefix_special_frames(B, N):
            row = idx[b, 0]
            hp[b, H_PZERO] = -(emb[row, H_PZERO] * sc)
            hp[b, H_NZERO] = np.float32(-0.0)
            hp[b, H_SUBNORMAL] = SUBNORMAL
    e = rng.randint(-12, 13, N * B * H)
    e[0], e[-1] = -12, 12                                      # the spread holds at the smallest case too
    gA = (rng.choice([-1.0, 1.0], e.size) * (0.5 + rng.random_sample(e.size)) * 2.0 ** e).astype(np.float32).reshape(N, B, H)
    return hp, emb, idx, gA, scale


# ---------------------------------------------------------------------------------------------- scatter cases
# layout "loss": grad [N][B][D], stride_b = D, stride_n = B D, idx [B][N + 1] (the last column is not scattered);
# layout "decode": grad [B][D], stride_b = D, stride_n = 0, idx [B][N].  goff / ooff: floats by which grad / out start past
# a 16-byte boundary.  same: a column in which every frame picks entry 3.  path = (cw, chunks, XCD mapping) the case claims.
ScatterCase = namedtuple("ScatterCase", "layout B N K D goff ooff same path")
SCATTER_CASES = [
    ScatterCase("loss", 65, 3, 64, 64, 0, 0, False, (4, 1, True)),
    ScatterCase("loss", 63, 2, 64, 512, 0, 0, False, (4, 2, True)),
    ScatterCase("loss", 64, 2, 128, 1024, 0, 0, True, (4, 4, True)),        # 64 hits in one ballot group: eight rounds of eight
    ScatterCase("decode", 513, 2, 64, 2048, 0, 0, False, (4, 8, True)),
    ScatterCase("loss", 513, 3, 16, 512, 0, 0, True, (2, 4, True)),         # K = 16, H = 512; 513 hits in one row
    ScatterCase("decode", 64, 2, 16, 512, 0, 0, False, (2, 4, True)),
    ScatterCase("loss", 65, 4, 32, 130, 0, 0, False, (1, 3, False)),        # H % 4 != 0
    ScatterCase("decode", 1, 4, 256, 30, 0, 0, False, (1, 1, True)),        # H % 4 != 0, a single frame
    ScatterCase("loss", 1, 2, 16, 260, 0, 0, False, (1, 5, False)),
    ScatterCase("loss", 64, 2, 16, 600, 1, 0, True, (1, 10, False)),        # grad 4 bytes off: CW 1, more than 8 chunks
    ScatterCase("loss", 65, 2, 16, 512, 1, 0, False, (1, 8, True)),         # grad 4 bytes off
    ScatterCase("decode", 63, 3, 64, 64, 0, 1, False, (1, 1, True)),        # out 4 bytes off
    ScatterCase("loss", 513, 1, 16, 64, 0, 0, False, (1, 1, True)),         # one scattered codebook (a loss over two)
]


def scatter_strides(c):
    """-> (stride_b, stride_n, idx_stride, floats of grad)"""
    if c.layout == "loss":
        return c.D, c.B * c.D, c.N + 1, c.N * c.B * c.D
    return c.D, 0, c.N, c.B * c.D


def scatter_path(c):
    """(cw, chunks, XCD mapping) by the launch mirror of tests/train_grid.py, from the case's strides and byte offsets"""
    sb, sn, _, _ = scatter_strides(c)
    cw = tg.db_cw(c.D, c.K, sb, sn, 4 * c.goff, 4 * c.ooff)
    ch = tg.db_chunks(c.D, cw)
    return cw, ch, ch <= 8 and 8 % ch == 0


def scatter_inputs(c):
    """-> grad (flat fp32), idx (flat int64, [B][idx_stride]).  Entry K - 1 of the last scattered column is picked by no
    frame; about one index in seven is negative (-100 or -1), whole frames among them; with c.same every frame picks
    entry 3 in column 0 (no negatives there); in the loss layout the unused column holds values in [0, K) only."""
    sb, sn, istride, ng = scatter_strides(c)
    rng = np.random.RandomState(c.B + 7 * c.N + 31 * c.K + c.D + c.goff + 2 * c.ooff)
    grad = (rng.standard_normal(ng) * 2.0 ** rng.randint(-8, 9, ng)).astype(np.float32)
    idx = rng.randint(0, c.K, (c.B, istride)).astype(np.int64)
    idx[:, c.N - 1] = rng.randint(0, c.K - 1, c.B)
    neg = rng.random_sample((c.B, c.N)) < 0.1
    idx[:, :c.N][neg] = -1
    if c.B > 2:
        idx[1::9, :c.N] = -100                                 # whole frames
    if c.N > 1:
        idx[0, c.N - 1] = -100
    else:
        idx[c.B // 2, 0] = -100
    if c.same:
        idx[:, 0] = 3
    return grad, idx.reshape(-1)
