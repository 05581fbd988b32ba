"""The three kernels behind JointCodebookLoss one by one: mcq_jcl_prefix_fwd, mcq_jcl_prefix_bwd and mcq_scatter_rows through
the C ABI on the cases of tests/jcl_grid.py, against its numpy restatements.

Each output is allocated inside a larger buffer filled with NaN: every element of the output must be overwritten, the guard
elements before and after it untouched.  The output must equal the fp32 restatement bit for bit (the library is built without
contraction; zeros compare by value), lie within the float64 restatement's bound, and a second call must give the same bits.
With B = 0 the prefix entry points return 0 and write nothing; mcq_scatter_rows returns 0 and stores its sums over no frame:
every row 0, the guards untouched (include/mcq.h: a row without a match is 0)."""
import numpy as np
import pytest
import torch

import jcl_grid as jg
from test_gpu_train_kernels import _check, _lib, _same, _st

pytestmark = pytest.mark.gpu
GUARD = 64          # floats: 256 bytes, so the guard does not move the output's 16-byte alignment


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(n, off=0):
    """-> (buffer of NaN, its view of n floats that starts GUARD + off floats in)"""
    buf = torch.full((GUARD + off + n + GUARD,), float("nan"), device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + off:GUARD + off + n]


def _guards_untouched(buf, view, what):
    lo = (view.data_ptr() - buf.data_ptr()) // 4
    assert lo >= GUARD and buf.numel() - lo - view.numel() >= GUARD
    assert torch.isnan(buf[:lo]).all() and torch.isnan(buf[lo + view.numel():]).all(), f"{what}: written outside the output"


def _bitwise(got, want, what):
    """equal as values everywhere (no NaN on either side, so only the sign of a zero may differ)"""
    got = got.cpu().numpy().reshape(want.shape)
    assert not np.isnan(got).any(), f"{what}: elements left unwritten"
    bad = got != want
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} entries differ from the fp32 restatement; first at {i}: "
                             f"got {float(got[i])!r} want {float(want[i])!r}")


@pytest.mark.parametrize("B,N,K,H", jg.PREFIX_CASES, ids=lambda v: str(v))
def test_prefix_fwd_matches_its_restatements(B, N, K, H):
    L = _lib()
    hp, emb, idx, _, scale = jg.prefix_inputs(B, N, K, H)
    d_hp, d_emb, d_idx = _dev(hp), _dev(emb), _dev(idx)

    def run():
        buf, A = _guarded(N * B * H)
        assert L.mcq_jcl_prefix_fwd(d_hp.data_ptr(), d_emb.data_ptr(), d_idx.data_ptr(), B, N, K, H, scale, A.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        _guards_untouched(buf, A, "mcq_jcl_prefix_fwd")
        return (A,)

    a = run()
    _same(a, run(), "mcq_jcl_prefix_fwd")
    _bitwise(a[0], jg.prefix_fwd32(hp, emb, idx, K, scale), "mcq_jcl_prefix_fwd A")
    A64, bound = jg.prefix_fwd64(hp, emb, idx, K, scale)
    _check("mcq_jcl_prefix_fwd", "A", a[0].cpu(), torch.from_numpy(A64), torch.from_numpy(bound))
    if jg.scale_is_power_of_two(H, N):       # exact zeros of either sign, and a subnormal that is kept
        got = a[0].cpu().numpy().reshape(N, B, H)
        for b in jg.prefix_special_frames(B, N):
            assert got[1, b, jg.H_PZERO] == 0 and got[1, b, jg.H_NZERO] == 0 and got[1, b, jg.H_SUBNORMAL] == jg.SUBNORMAL


@pytest.mark.parametrize("B,N,K,H", jg.PREFIX_CASES, ids=lambda v: str(v))
def test_prefix_bwd_matches_its_restatements(B, N, K, H):
    L = _lib()
    hp, emb, idx, gA, scale = jg.prefix_inputs(B, N, K, H)
    A = jg.prefix_fwd32(hp, emb, idx, K, scale)            # A is taken as given
    d_A, d_gA = _dev(A), _dev(gA)

    def run():
        b1, g_hp = _guarded(B * H)
        b2, gE = _guarded((N - 1) * B * H)
        assert L.mcq_jcl_prefix_bwd(d_A.data_ptr(), d_gA.data_ptr(), B, N, H, scale, g_hp.data_ptr(), gE.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        _guards_untouched(b1, g_hp, "mcq_jcl_prefix_bwd g_hp")
        _guards_untouched(b2, gE, "mcq_jcl_prefix_bwd gE")
        return g_hp, gE

    a = run()
    _same(a, run(), "mcq_jcl_prefix_bwd")
    w_hp, w_E = jg.prefix_bwd32(A, gA, scale)
    _bitwise(a[0], w_hp, "mcq_jcl_prefix_bwd g_hp")
    _bitwise(a[1], w_E, "mcq_jcl_prefix_bwd gE")
    g64, e64, bg, be = jg.prefix_bwd64(A, gA, scale)
    _check("mcq_jcl_prefix_bwd", "g_hp", a[0].cpu(), torch.from_numpy(g64), torch.from_numpy(bg))
    _check("mcq_jcl_prefix_bwd", "gE", a[1].cpu(), torch.from_numpy(e64), torch.from_numpy(be))


def test_prefix_bwd_mask_at_zeros_and_subnormals():
    """A handed in as +0, -0, a positive subnormal, 1 and 0 in codebook 1 (all 0 in codebook 0), scale 1: gE[0] is gA[1]
    under the mask 0, 0, 1, 1, 0 and g_hp the same, as torch's ReLU backward has it"""
    L = _lib()
    A = np.zeros((2, 1, 5), np.float32)
    A[1, 0] = [0.0, -0.0, jg.SUBNORMAL, 1.0, 0.0]
    gA = np.array([[[3.0, 5.0, 7.0, 9.0, 11.0]], [[2.0, -4.0, 6.0, -8.0, 10.0]]], np.float32)
    d_A, d_gA = _dev(A), _dev(gA)
    b1, g_hp = _guarded(5)
    b2, gE = _guarded(5)
    assert L.mcq_jcl_prefix_bwd(d_A.data_ptr(), d_gA.data_ptr(), 1, 2, 5, 1.0, g_hp.data_ptr(), gE.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert gE.tolist() == [0.0, 0.0, 6.0, -8.0, 0.0] and g_hp.tolist() == [0.0, 0.0, 6.0, -8.0, 0.0]
    _guards_untouched(b1, g_hp, "g_hp")
    _guards_untouched(b2, gE, "gE")


@pytest.mark.parametrize("c", jg.SCATTER_CASES, ids=lambda c: "-".join(map(str, c[:7])))
def test_scatter_rows_matches_its_restatements(c):
    L = _lib()
    sb, sn, istride, ng = jg.scatter_strides(c)
    grad, idx = jg.scatter_inputs(c)
    gbuf = torch.empty(c.goff + ng, device="cuda")
    d_grad = gbuf[c.goff:]
    d_grad.copy_(torch.from_numpy(grad))
    d_idx = _dev(idx)
    assert gbuf.data_ptr() % 16 == 0 and d_grad.data_ptr() % 16 == 4 * c.goff

    def run():
        buf, out = _guarded(c.N * c.K * c.D, c.ooff)
        assert out.data_ptr() % 16 == 4 * c.ooff       # with scatter_path: the launch takes the path the case claims
        assert L.mcq_scatter_rows(d_grad.data_ptr(), sb, sn, d_idx.data_ptr(), istride, c.B, c.N, c.K, c.D, out.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        _guards_untouched(buf, out, "mcq_scatter_rows")
        return (out,)

    assert jg.scatter_path(c) == c.path
    a = run()
    _same(a, run(), "mcq_scatter_rows")
    _bitwise(a[0], jg.scatter_rows32(grad, sb, sn, idx, istride, c.B, c.N, c.K, c.D), "mcq_scatter_rows out")
    o64, bound, hits = jg.scatter_rows64(grad, sb, sn, idx, istride, c.B, c.N, c.K, c.D)
    _check("mcq_scatter_rows", "out", a[0].cpu(), torch.from_numpy(o64), torch.from_numpy(bound))
    got = a[0].cpu().numpy().reshape(c.N * c.K, c.D)
    assert (hits == 0).any() and not got[hits == 0].any(), "a row without a hit is 0.0"


def test_no_frames():
    """B = 0: each entry point returns 0; the prefix entry points write nothing, mcq_scatter_rows stores the empty sums
    (every row 0) and nothing outside its output"""
    L = _lib()
    N, K, H = 3, 16, 40
    src = torch.zeros(1024, device="cuda")
    isrc = torch.zeros(16, dtype=torch.int64, device="cuda")
    b1, A = _guarded(N * 4 * H)
    assert L.mcq_jcl_prefix_fwd(src.data_ptr(), src.data_ptr(), isrc.data_ptr(), 0, N, K, H, 0.5, A.data_ptr(), _st()) == 0
    b2, g_hp = _guarded(4 * H)
    b3, gE = _guarded((N - 1) * 4 * H)
    assert L.mcq_jcl_prefix_bwd(src.data_ptr(), src.data_ptr(), 0, N, H, 0.5, g_hp.data_ptr(), gE.data_ptr(), _st()) == 0
    b4, out = _guarded((N - 1) * K * H)
    assert L.mcq_scatter_rows(src.data_ptr(), H, 0, isrc.data_ptr(), N, 0, N - 1, K, H, out.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    for b in (b1, b2, b3):
        assert torch.isnan(b).all(), "a prefix entry point wrote with B = 0"
    _guards_untouched(b4, out, "mcq_scatter_rows with B = 0")
    assert not out.cpu().numpy().any() and not torch.isnan(out).any()
