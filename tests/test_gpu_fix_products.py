"""The fixed-point products of quantization_amd/csrc/mcq_fix_kernels.h value by value against exact integers (gpu).

Every table the index search reads comes out of k_fix_rows / k_fix_rows2 (rows -> limb planes, row exponents, wmu, Q) and
k_fgemm (the ten limb products: the Gram matrix G, x.C, the logits).  The header promises EXACT products; the rest of the
suite sees them through an arg max.  Here every stage is compared with tests/fix_products.py (the definition in exact
integers, pinned on the CPU by tests/test_fix_products_host.py) applied to the DEVICE'S OWN upstream output, so a failure names
the stage: C from the inputs, the means and Q from the blob's C, the planes from the blob's C and means, G from the blob's
planes, x.C and the logits from the blob's planes, mean, wmu and bias.  Comparisons are bit for bit on the uint32 views
(-0.0, inf and an unwritten word count); the only bounds are the two derived ones for sums whose order the kernels do not
fix (the means, Q).  `prepared`, every output and every workspace start as 0xA5 bytes: padding a kernel forgets to write
shows up as a wrong value, not as a lucky zero.

Non-finite inputs stay out of scope: their contract is "terminates with codes in range" (include/mcq.h).  Every row here is
finite; products of two rows near 3e38 overflow to inf, which the definition gives as well."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import fix_products as fp
from logits_screen import limbs_of

pytestmark = pytest.mark.gpu
F = np.float32
U = 2.0 ** -24
X_FP16 = 4          # MCQ_ENCODE_X_FP16
ORDER = ("C", "Q", "Cf", "Ce", "Wf", "We", "wmu", "bias", "scales", "mean", "cmean", "G", "total")
LS = F(1.3498588)   # lscale_exp: no power of two, so the chain's multiplication rounds

ROW_SHAPES = [(1, 16, 1), (2, 16, 3), (4, 32, 17), (8, 64, 127), (2, 256, 128), (1, 1024, 129), (4, 128, 513), (2, 64, 1025),
              (2, 32, 1028), (1, 16, 2050)]
MANY_TILE_G = [(64, 64, 40), (16, 256, 130)]          # 32 x 32 tiles on at most 256 workgroups: four tiles each
XC_SHAPES = [(1, 16, 1), (2, 16, 45), (2, 256, 128), (8, 256, 129), (1, 1024, 33), (4, 128, 513), (2, 32, 1028)]
XC_BATCHES = [1, 127, 128, 129, 300]


def _L():
    from quantization_amd import _lib as m
    return m.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _filled(nbytes):
    return torch.full((int(nbytes),), 0xA5, dtype=torch.uint8, device="cuda")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(got, want, what):
    """bit for bit; the message names the first differing entries"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    first = [(tuple(int(i) for i in at), got[tuple(at)], want[tuple(at)]) for at in bad[:5]]
    raise AssertionError(f"{what}: {len(bad)} of {g.size} entries differ; (index, device, exact): {first}")


def _edge_positions(n_rows, n_edges):
    return [(i * n_rows) // n_edges for i in range(n_edges)]


def _state(N, K, D, variant):
    """centers [N][K][D], cscale, W [N*K][D], bias [N*K].  plain: standard normal centers; offset: a common offset of 10 on top,
    which the centering takes out again; zero: all-zero centers (the data mean is 0: the frames reach the products as they are);
    modest: plain; ties: plain, and two classifier rows per codebook that are copies of each other with the largest bias.
    W carries the edge rows in every variant -- all but the two near 3e38 in `modest` and `ties`, whose logits are formed with a
    non-zero mean: fixdot(W_r, mean) overflows for such a row, inf - inf is a NaN, and an undefined logit is as far outside the
    contract as a non-finite input (the `zero` variant has those rows on both sides, with wmu = 0)."""
    nk = N * K
    rs = np.random.RandomState(100003 * N + 101 * K + D + 17 * len(variant))
    centers = rs.standard_normal((N, K, D)).astype(F)
    if variant == "offset":
        centers = (centers + F(10.0)).astype(F)
    if variant == "zero":
        centers[:] = 0
    W = (rs.standard_normal((nk, D)) / np.sqrt(D)).astype(F)
    edges = fp.edge_rows(D, rs)
    for at, name in zip(_edge_positions(nk, len(edges)), edges):
        if not (variant in ("modest", "ties") and name.startswith("huge")):
            W[at] = edges[name]
    bias = (rs.standard_normal(nk) * 0.1).astype(F)
    if variant == "ties":
        for n in range(N):
            a, b = n * K + 3, n * K + K - 2
            W[a] = W[b] = (rs.standard_normal(D) / np.sqrt(D)).astype(F)
            bias[a] = bias[b] = F(6.0)
    return centers, F(0.8137), W, bias


def _state_m128(N, K, D):
    """the domain's edge D = 16,384: every row is the one the i32 accumulators are sized for (one element 1.0, the rest at limbs
    (0, -128, -128, -128)), or its negative; the rows of a codebook come in +/- pairs so that every mean is exactly 0 and the
    rows reach the products as they are"""
    base = np.full(D, fp.Q_M128 * 2.0 ** -29, np.float64).astype(F)

    def row(j, sign):
        v = base.copy()
        v[j % D] = 1.0
        return (sign * v).astype(F)

    centers = np.stack([row(4099 * (r // 2) + 5, 1 - 2 * (r % 2)) for r in range(N * K)]).reshape(N, K, D)
    W = np.stack([row(977 * r + 16, -1 if r % 3 == 0 else 1) for r in range(N * K)])
    bias = (np.arange(N * K) % 7 * 0.25 - 0.5).astype(F)
    x = np.stack([row(5, 1), row(9000, -1), row(D - 1, 1)])
    return centers, F(1.0), W, bias, x


def _prepare(centers, cs, W, bias):
    L = _L()
    N, K, D = centers.shape
    nk = N * K
    off = (ctypes.c_size_t * len(ORDER))()
    assert L.mcq_test_prepared_layout(N, K, D, off, len(ORDER)) == len(ORDER)
    off = dict(zip(ORDER, list(off)))
    assert off["total"] == L.mcq_prepared_bytes(N, K, D)
    blob_d = _filled(off["total"])
    cd, wd, bd = _dev(centers), _dev(W), _dev(bias)
    assert L.mcq_prepare(cd.data_ptr(), float(cs), wd.data_ptr(), bd.data_ptr(), N, K, D, blob_d.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    blob = blob_d.cpu().numpy()
    Dp, Dq, Rp = fp.round_up(D, 16), fp.round_up(D, 128), fp.round_up(nk, 128)
    f32 = lambda name, n: blob[off[name]:off[name] + 4 * n].view(np.float32)
    i32 = lambda name, n: blob[off[name]:off[name] + 4 * n].view(np.int32)
    p = types.SimpleNamespace(N=N, K=K, D=D, nk=nk, Dp=Dp, Dq=Dq, Rp=Rp, centers=centers, cs=cs, W=W, bias_in=bias,
                              blob_d=blob_d, off=off)
    p.C = f32("C", nk * Dp).reshape(N, K, Dp)
    p.Q = f32("Q", nk)
    p.Cf = blob[off["Cf"]:off["Cf"] + Rp * Dq * 4]
    p.Ce = i32("Ce", Rp)
    p.Wf = blob[off["Wf"]:off["Wf"] + Rp * Dq * 4]
    p.We = i32("We", Rp)
    p.wmu = f32("wmu", nk)
    p.bias = f32("bias", nk)
    p.mean = f32("mean", Dp)
    p.cmean = f32("cmean", N * Dp).reshape(N, Dp)
    p.G = f32("G", nk * nk).reshape(nk, nk)
    # the operands of the three products as the device holds them
    p.c_op = (fp.limbs_from_planes(p.Cf, Rp, Dq, nk), p.Ce[:nk].astype(np.int64))
    p.w_op = (fp.limbs_from_planes(p.Wf, Rp, Dq, nk), p.We[:nk].astype(np.int64))
    return p


@functools.lru_cache(maxsize=None)
def _prepared(N, K, D, variant="plain"):
    return _prepare(*_state(N, K, D, variant))


@functools.lru_cache(maxsize=None)
def _prepared_m128():
    centers, cs, W, bias, x = _state_m128(2, 16, 16384)
    p = _prepare(centers, cs, W, bias)
    p.x = x
    return p


# ------------------------------------------------------------------------------------------------ a. prepare, rows
def _check_rows(p):
    N, K, D, nk, Dp, Dq, Rp = p.N, p.K, p.D, p.nk, p.Dp, p.Dq, p.Rp
    want = np.zeros((N, K, Dp), F)
    want[:, :, :D] = (p.cs * p.centers).astype(F)
    _same(p.C, want, "C = fl(cscale * centers), zero columns D .. Dp")
    # the means: K additions and a division per codebook, N - 1 additions across them, in an order the kernel is free to choose
    C64 = p.C.astype(np.float64)
    absmean = np.abs(C64).mean(axis=1)                                   # [N][Dp]
    err = np.abs(p.cmean.astype(np.float64) - C64.mean(axis=1))
    bound = (K + N + 2) * U * absmean
    print(f"cmean: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), ("cmean", float((err - bound).max()))
    err = np.abs(p.mean.astype(np.float64) - C64.mean(axis=1).sum(axis=0))
    bound = (K + N + 2) * U * absmean.sum(axis=0)
    print(f"mean: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), ("mean", float((err - bound).max()))
    # the centered rows, their sums of squares (Dp products added in an unspecified order) and their planes
    centered = (p.C - p.cmean[:, None, :]).astype(F).reshape(nk, Dp)
    Q64 = (centered.astype(np.float64) ** 2).sum(axis=1)
    err = np.abs(p.Q.astype(np.float64) - Q64)
    print(f"Q: largest error / bound {float((err / np.maximum((Dp + 2) * U * Q64, 1e-300)).max()):.3f}")
    assert (err <= (Dp + 2) * U * Q64).all(), ("Q", float((err / np.maximum(Q64, 1e-300)).max()))
    for name, rows, planes, exps in (("C - mu_n", centered, p.Cf, p.Ce), ("W", p.W, p.Wf, p.We)):
        limbs, e = limbs_of(rows)
        we = np.full(Rp, -125, np.int32)                                 # a padding row is a zero row: exponent -125
        we[:nk] = e
        _same(exps, we, f"row exponents of {name} (rows {nk} .. {Rp}: -125)")
        _same(planes, fp.planes_of(limbs, Rp, Dq), f"limb planes of {name} (zero rows {nk} .. {Rp}, zero columns {D} .. {Dq})")
    _same(p.bias, p.bias_in, "bias")
    _same(p.wmu, fp.fixdot_matrix(p.W, p.mean[None, :D])[:, 0], "wmu = fixdot(W_r, mean)")


@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("N,K,D", ROW_SHAPES)
def test_prepare_rows(N, K, D, variant):
    _check_rows(_prepared(N, K, D, variant))


# ------------------------------------------------------------------------------------------------ b. G
def _check_gram(p, sampled):
    G = p.G.view(np.uint32)
    assert np.array_equal(G, G.T), "G is not symmetric bit for bit"
    idx = fp.sample_index(p.nk) if sampled else np.arange(p.nk)
    assert len(idx) <= 300 or not sampled
    op = ([l[idx] for l in p.c_op[0]], p.c_op[1][idx])
    _same(p.G[np.ix_(idx, idx)], fp.fixdot_matrix(op, op), "G = fixdot(C_r - mu, C_s - mu)")


@pytest.mark.parametrize("variant", ["plain", "offset"])
@pytest.mark.parametrize("N,K,D", ROW_SHAPES)
def test_gram(N, K, D, variant):
    _check_gram(_prepared(N, K, D, variant), sampled=False)


@pytest.mark.parametrize("N,K,D", MANY_TILE_G)
def test_gram_many_tiles(N, K, D):
    p = _prepared(N, K, D)
    assert (p.Rp // 128) ** 2 == 1024
    _check_rows(p)
    _check_gram(p, sampled=True)


# ------------------------------------------------------------------------------------------------ c. x.C and the logits
def _run(entry, p, x_ptr, B, flags=0):
    L = _L()
    out = _filled(B * p.nk * 4)
    nws = L.mcq_logits_workspace_bytes(B, p.N, p.D)
    ws = _filled(nws)
    if entry == "xc":
        rc = L.mcq_test_xc(x_ptr, B, p.blob_d.data_ptr(), p.N, p.K, p.D, out.data_ptr(), ws.data_ptr(), nws, _st(), flags)
    else:
        assert flags == 0
        rc = L.mcq_logits(x_ptr, B, p.blob_d.data_ptr(), float(LS), p.N, p.K, p.D, out.data_ptr(), ws.data_ptr(), nws, _st())
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.float32).reshape(B, p.nk)


def _frames(p, x):
    """what both products see of the frames x (fp32, widened already): fl(x - mean) with the blob's mean"""
    return (np.asarray(x, F) - p.mean[None, :p.D]).astype(F)


def _check_products(p, x, x_ptr, B, flags=0, sampled=False, logits=None):
    rows = fp.sample_index(B) if sampled else np.arange(B)
    cols = fp.sample_index(p.nk) if sampled else np.arange(p.nk)
    assert not sampled or (len(rows) <= 300 and len(cols) <= 300)
    fr = limbs_of(_frames(p, x)[rows])
    c_op = ([l[cols] for l in p.c_op[0]], p.c_op[1][cols])
    w_op = ([l[cols] for l in p.w_op[0]], p.w_op[1][cols])
    xc = _run("xc", p, x_ptr, B, flags)
    _same(xc[np.ix_(rows, cols)], fp.fixdot_matrix(fr, c_op), f"x.C = fixdot(x - mean, C_r - mu), B = {B}")
    if logits is None:
        logits = _run("logits", p, x_ptr, B)
    want = fp.logits_of(fr, w_op, p.wmu[cols], LS, p.bias[cols])
    assert not np.isnan(want).any(), "the case itself is outside the contract: an undefined logit"
    _same(logits[np.ix_(rows, cols)], want, f"logits = ((fixdot(x - mean, W_r) + wmu_r) * ls) + bias_r, B = {B}")
    return want


@pytest.mark.parametrize("B", XC_BATCHES)
@pytest.mark.parametrize("N,K,D", XC_SHAPES)
def test_xc_and_logits(N, K, D, B):
    p = _prepared(N, K, D, "modest")
    x = np.random.RandomState(B + D).standard_normal((B, D)).astype(F)
    xd = _dev(x)
    _check_products(p, x, xd.data_ptr(), B)


def test_xc_and_logits_many_tiles():
    # 16 table tiles x 18 frame tiles = 288 tiles on 256 workgroups, the last frame tile partial
    p = _prepared(8, 256, 130, "modest")
    B = 2300
    x = np.random.RandomState(B).standard_normal((B, p.D)).astype(F)
    xd = _dev(x)
    _check_products(p, x, xd.data_ptr(), B, sampled=True)


def test_edge_rows_as_frames_with_zero_centers():
    # all-zero centers: the mean is exactly 0, x - mean is x itself, and the frames carry the edge rows unmodified
    p = _prepared(2, 64, 130, "zero")
    assert not p.mean.view(np.uint32).any() and not p.wmu.view(np.uint32).any()
    B = 131
    rs = np.random.RandomState(5)
    x = rs.standard_normal((B, p.D)).astype(F)
    edges = fp.edge_rows(p.D, rs)
    for at, name in zip(_edge_positions(B, len(edges)), edges):
        x[at] = edges[name]
    x[B - 1] = edges["limbs_m128"]                                      # one in the partial frame tile
    _same(_frames(p, x), x, "x - 0")
    xd = _dev(x)
    want = _check_products(p, x, xd.data_ptr(), B)
    assert np.isinf(want).any() and not np.isnan(want).any()            # huge x huge overflows; nothing is undefined


def test_unaligned_frames_take_the_scalar_loads():
    # D % 4 == 0 and the frames one float past a 16-byte boundary: the rows kernel must not use 16-byte loads
    p = _prepared(2, 256, 128, "modest")
    B = 129
    x = np.random.RandomState(9).standard_normal((B, p.D)).astype(F)
    buf = _dev(np.concatenate([np.zeros(1, F), x.reshape(-1)]))
    ptr = buf.data_ptr() + 4
    assert ptr % 16 == 4
    _check_products(p, x, ptr, B)


# ------------------------------------------------------------------------------------------------ d. fp16 frames, the arg max
@pytest.mark.parametrize("N,K,D,B", [(8, 256, 129, 129), (4, 16, 45, 300)])
def test_fp16_frames_and_argmax(N, K, D, B):
    L = _L()
    p = _prepared(N, K, D, "ties")
    x16 = np.random.RandomState(B).standard_normal((B, D)).astype(np.float16)
    xd = _dev(x16)
    logits, amax = _filled(B * p.nk * 4), _filled(B * N * 8)
    nws = L.mcq_logits_workspace_bytes(B, N, D)
    ws = _filled(nws)
    assert L.mcq_logits_argmax(xd.data_ptr(), B, p.blob_d.data_ptr(), float(LS), N, K, D, logits.data_ptr(), amax.data_ptr(),
                               ws.data_ptr(), nws, _st(), X_FP16) == 0
    torch.cuda.synchronize()
    logits = logits.cpu().numpy().view(np.float32).reshape(B, p.nk)
    want = _check_products(p, x16.astype(F), xd.data_ptr(), B, flags=X_FP16, logits=logits)
    first = want.reshape(B, N, K).argmax(axis=2)                          # numpy: the first of equal maxima
    _same(amax.cpu().numpy().view(np.int64).reshape(B, N), first.astype(np.int64), "arg max")
    # the copied rows tie exactly, and often at the top: the lower row must be the one reported
    a, b = want.reshape(B, N, K)[:, :, 3], want.reshape(B, N, K)[:, :, K - 2]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (first == 3).sum() > B * N // 4 and not (first == K - 2).any()


# ------------------------------------------------------------------------------------------------ e. D = 16,384
def test_largest_limb_sums_at_the_largest_dim():
    p = _prepared_m128()
    assert not p.mean.view(np.uint32).any() and not p.cmean.view(np.uint32).any()
    l, _ = limbs_of(p.x)
    assert sorted(np.unique(l[1]).tolist()) == [-128, -127, 0] and ((l[1] == -128).sum(axis=1) >= p.D - 1).any()
    _check_rows(p)
    _check_gram(p, sampled=False)
    xd = _dev(p.x)
    _check_products(p, p.x, xd.data_ptr(), len(p.x))
