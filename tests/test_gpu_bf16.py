"""The Lloyd step over a bf16 store on the device (include/mcq_bf16.h rules 56-59) against numpy float64 and against the fp32
entries, and coarse_train_bf16 end to end.  Every call of a C entry runs between the guards of tests/arena.py, as in
tests/test_gpu_half.py: outputs and scratch of exactly the stated sizes, guards intact and inputs unchanged after every call."""
import numpy as np
import pytest
import torch

import arena
from test_gpu_kmeans import _bits, _update

pytestmark = pytest.mark.gpu
VT = 256                                                     # vectors of the assign kernel's tile


def _dev16(a, offset=0):
    """a (float32) on the device as bf16, rounded by torch; offset = 1: the base is 2 bytes past a 16-byte boundary, so the
    2-byte loads run -> (the view, its values as float64)"""
    flat = torch.empty(a.size + offset, dtype=torch.bfloat16, device="cuda")
    view = flat[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view, view.float().cpu().numpy().astype(np.float64)


def _planes(c):
    """rule 57's three planes of fp32 c by torch's conversion on the CPU, as float64"""
    rest, out = torch.from_numpy(c), []
    for _ in range(3):                                       # (both subtractions are exact in fp32)
        out.append(rest.bfloat16().float())
        rest = rest - out[-1]
    return [p.numpy().astype(np.float64) for p in out]


def _assign(x, c, parts=None, prev=None):
    """the C entry between guards -> (assign, score, changed) as numpy / int"""
    from quantization_amd import _lib, coarse_terms
    lib = _lib.lib()
    (B, D), L = x.shape, c.shape[0]
    terms = coarse_terms(c)
    parts = parts or lib.mcq_kmeans_bf16_parts(B, L, D)
    out = [arena.guarded((B,), torch.int32), arena.guarded((B,), torch.float32), arena.guarded((1,), torch.int32),
           arena.guarded((B, parts), torch.float32), arena.guarded((B, parts), torch.int32),
           arena.guarded((lib.mcq_kmeans_bf16_planes(L, D),), torch.int16)]
    with arena.frozen(x, c, terms, prev):
        rc = lib.mcq_kmeans_assign_bf16(x.data_ptr(), B, c.data_ptr(), L, D, terms.data_ptr(), parts,
                                        None if prev is None else prev.data_ptr(), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                        out[4].ptr, out[5].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out) and (prev is not None or out[2].untouched())
    return out[0].t.cpu().numpy(), out[1].t.cpu().numpy(), None if prev is None else int(out[2].t[0])


def _grid(B, L, D):
    """vector elements integers in [-2, 2]; centroid elements a + b 2^-13, |a| <= 4, |b| <= 7.  There hi = a, mid = b 2^-13 and
    lo is zero everywhere, so element l % D of row l is +-(16 + 2^-5 + 2^-13) instead: planes 16, 2^-5 and 2^-13.  Every plane
    is a multiple of 2^-13 and every partial sum stays below 2 (4.001 (D - 1) + 16.04) < 2^10 for D <= 80: exact in fp32 in
    any order.  Rows 0 and 1 come again at a higher index, the second one in another tile where there is one"""
    rs = np.random.RandomState(1000 * B + 10 * L + D)
    x = rs.randint(-2, 3, (B, D)).astype(np.float32)
    c = (rs.randint(-4, 5, (L, D)) + rs.randint(-7, 8, (L, D)) * 2.0 ** -13).astype(np.float32)
    rows = np.arange(L)
    c[rows, rows % D] = (1 - 2 * (rows % 2)) * np.float32(16 + 2.0 ** -5 + 2.0 ** -13)
    if L > 1:
        c[L - 1] = c[0]
    if L > 200:
        c[200] = c[1]
    hi, mid, lo = _planes(c)
    assert hi.any() and mid.any() and lo.any() and np.array_equal(hi + mid + lo, c.astype(np.float64))
    return x, c


def _exact(x, c, cd):
    """the expected (assign, score): fl(h[l] - dot) in fp32 with the exact dot, h as coarse_terms (shipped code) makes it"""
    from quantization_amd import coarse_terms
    s = coarse_terms(cd).cpu().numpy()[None, :] - (x.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    assert s.dtype == np.float32
    want = s.argmin(1)
    return want, s[np.arange(len(x)), want]


@pytest.mark.parametrize("B,L,D,offset", [
    (1, 1, 1, 0), (VT - 1, 129, 15, 1), (VT, 127, 16, 0), (VT + 1, 128, 17, 1), (300, 300, 33, 0), (1, 300, 64, 0), (300, 1, 65, 1),
    (VT + 1, 300, 80, 0), (VT, 128, 64, 1), (VT - 1, 127, 80, 1), (2 * VT + 1, 129, 16, 1), (VT + 1, 129, 33, 0)])
def test_assign_exact(B, L, D, offset):
    """assign and score are float64's bit for bit, ties to the lower list, one part and the most; offset 1: the 2-byte loads"""
    x, c = _grid(B, L, D)
    (xd, _), cd = _dev16(x, offset), torch.from_numpy(c).cuda()
    assert xd.data_ptr() % 4 == 2 * offset
    want, score = _exact(x, c, cd)
    for parts in {1, -(-L // 128)}:
        got, gs, _ = _assign(xd, cd, parts)
        assert np.array_equal(got, want) and np.array_equal(_bits(gs), _bits(score)), parts


def test_assign_nan_inf_and_changed():
    """a NaN row and an inf against a zero column: (-1, +inf), the neighbours keep their bits; `changed` counts exactly"""
    x, c = _grid(VT + 1, 300, 33)
    c[:, 5] = 0
    cd = torch.from_numpy(c).cuda()
    want, score = _exact(x, c, cd)
    got, gs, none = _assign(_dev16(x)[0], cd)
    assert none is None and np.array_equal(got, want) and np.array_equal(_bits(gs), _bits(score))
    assert _assign(_dev16(x)[0], cd, 3, prev=torch.from_numpy(got).cuda())[2] == 0
    prev = got.copy()
    prev[[0, 5, 64, 100, VT]] += 1
    assert _assign(_dev16(x)[0], cd, 2, prev=torch.from_numpy(prev).cuda())[2] == 5
    x[64, 3], x[70, 5] = np.nan, np.inf
    got2, gs2, _ = _assign(_dev16(x)[0], cd, 2)
    assert (got2[[64, 70]] == -1).all() and (gs2[[64, 70]] == np.inf).all()
    keep = ~np.isin(np.arange(VT + 1), (64, 70))
    assert np.array_equal(got2[keep], want[keep]) and np.array_equal(_bits(gs2[keep]), _bits(score[keep]))


@pytest.mark.parametrize("B,L,D", ((500, 300, 96), (300, 129, 65)))
def test_assign_real_inputs(B, L, D):
    """Gaussian rows against the float64 value of h[l] - sum_e v_e (hi_e + mid_e + lo_e), S = sum_e |v_e| (|hi_e| + |mid_e| +
    |lo_e|).  Products of two bf16 numbers are exact in fp32; over T = ceil(D / 16) steps the accumulator takes 48 T products
    and 3 T accumulator additions, each off by at most 2^-23 of a partial sum of magnitudes (<= S); the last subtraction rounds
    once.  So |score - ref| <= 1.01 ((51 T 2^-23 + 2^-24) S + 2^-24 |h|).  assign is the float64 argmin wherever the float64
    gap between best and second exceeds twice the row's largest bound; at most 1 % of rows are excused."""
    from quantization_amd import coarse_terms
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((L, D)).astype(np.float32)
    (xd, x64), cd = _dev16(x), torch.from_numpy(c).cuda()
    hi, mid, lo = _planes(c)
    assert np.array_equal(hi + mid + lo, c.astype(np.float64))
    h = coarse_terms(cd).cpu().numpy().astype(np.float64)
    ref = h[None, :] - x64 @ (hi + mid + lo).T
    S = np.abs(x64) @ (np.abs(hi) + np.abs(mid) + np.abs(lo)).T
    bound = 1.01 * ((51 * -(-D // 16) * 2.0 ** -23 + 2.0 ** -24) * S + 2.0 ** -24 * np.abs(h)[None, :])
    got, score, _ = _assign(xd, cd)
    rows = np.arange(B)
    assert (got >= 0).all()
    ratio = float((np.abs(score - ref[rows, got]) / bound[rows, got]).max())
    two = np.sort(ref, 1)[:, :2]
    sure = two[:, 1] - two[:, 0] > 2 * bound.max(1)
    print(f"[bf16 assign] {B} x {L} x {D}: largest error / bound {ratio:.4f}, excused rows {int((~sure).sum())}")
    assert ratio < 1 and (~sure).mean() <= 0.01 and np.array_equal(got[sure], ref.argmin(1)[sure])


@pytest.mark.parametrize("D", (1, 65, 68, 1030))
def test_update_is_the_fp32_update_on_widened_rows(D):
    """tests/test_gpu_half.py's case: 9,000 rows in lists of 5,300, 0 and 3,700, two order entries that name no row: the bits of
    mcq_kmeans_update on the rows widened to fp32.  D = 68 takes the 8-byte loads, 1,030 a second slab"""
    from quantization_amd import _lib
    lib, rs, B, L = _lib.lib(), np.random.RandomState(D), 9000, 3
    x = rs.standard_normal((B, D)).astype(np.float32)
    order, offsets = rs.permutation(B).astype(np.int64), np.array([0, 5300, 5300, B], np.int64)
    order[7], order[5400] = -1, B
    cin = rs.standard_normal((L, D)).astype(np.float32)
    xd = _dev16(x)[0]
    want, wcounts = _update(xd.float(), order, offsets, cin)
    od, fd, cd = torch.from_numpy(order).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(cin).cuda()
    out = [arena.guarded((L, D), torch.float32), arena.guarded((L,), torch.int32), arena.guarded((L + 1,), torch.int64),
           arena.guarded((lib.mcq_kmeans_blocks(B, L, D),), torch.float64)]
    with arena.frozen(xd, od, fd, cd):
        rc = lib.mcq_kmeans_update_bf16(xd.data_ptr(), B, D, od.data_ptr(), fd.data_ptr(), L, cd.data_ptr(), out[0].ptr, out[1].ptr,
                                        out[2].ptr, out[3].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out)
    assert np.array_equal(_bits(out[0].t.cpu().numpy()), _bits(want)) and np.array_equal(out[1].t.cpu().numpy(), wcounts)
    assert list(wcounts) == [5299, 0, 3699] and np.array_equal(_bits(want[1]), _bits(cin[1]))


@pytest.mark.parametrize("B,L,D,most", ((2 * VT + 1, 129, 16, 2), (VT + 1, 300, 33, 3)))
def test_assign_is_the_fp32_assign_on_exact_inputs(B, L, D, most):
    """_grid inputs are exact in fp32 in any order, so mcq_kmeans_assign on the widened rows gives the same assign, score bits
    and `changed`, with one part and with the most.  (513, 129, 16): the 16-byte loads; (257, 300, 33): the element-wise ones"""
    from test_gpu_kmeans import _assign as _assign32
    x, c = _grid(B, L, D)
    (xd, _), cd = _dev16(x), torch.from_numpy(c).cuda()
    xf = xd.float()
    assert xd.data_ptr() % 16 == 0 and xf.data_ptr() % 16 == 0
    prev = np.asarray(_assign(xd, cd, 1)[0]).copy()
    prev[[0, 5, 64, 100, B - 1]] += 1
    pd = torch.from_numpy(prev).cuda()
    for parts in (1, most):
        a16, s16, n16 = _assign(xd, cd, parts, prev=pd)
        a32, s32, n32 = _assign32(xf, cd, parts, prev=pd)
        assert np.array_equal(a16, a32) and np.array_equal(_bits(s16), _bits(s32)) and n16 == n32 == 5, parts


def test_step_is_the_fp32_step_on_exact_inputs():
    """kmeans_step_bf16(x16, c, prev_assign=p) against kmeans_step(x16.float(), c, prev_assign=p) on _grid(300, 5, 33), list 4
    empty (row 4 of c is row 0): the same new centroids bit for bit, the same assign, counts and changed"""
    from quantization_amd import kmeans_step, kmeans_step_bf16
    x, c = _grid(300, 5, 33)
    assert np.array_equal(c[4], c[0])
    (xd, _), cd = _dev16(x), torch.from_numpy(c).cuda()
    p = torch.zeros(300, dtype=torch.int32, device="cuda")
    new16, a16, n16, ch16 = kmeans_step_bf16(xd, cd, prev_assign=p)
    new32, a32, n32, ch32 = kmeans_step(xd.float(), cd, prev_assign=p)
    assert torch.equal(new16.view(torch.int32), new32.view(torch.int32)) and torch.equal(a16, a32) and torch.equal(n16, n32)
    assert int(ch16) == int(ch32) == int((a32 != 0).sum()) and int(n32[4]) == 0
    assert torch.equal(new32[4].view(torch.int32), cd[4].view(torch.int32)) and int(n32.sum()) == 300


def test_coarse_train_bf16_end_to_end():
    """tests/test_gpu_kmeans.py's 8 blobs rounded to bf16, init one point of each.  After 3 steps assign is the blob label and
    every centroid element lies within 2^-24 |mean| + n 2^-53 mean(|x|) of the float64 mean of the bf16 rows."""
    from quantization_amd import coarse_assign_bf16, coarse_train_bf16, kmeans_step_bf16
    rs = np.random.RandomState(0)
    D, n = 33, 300
    label = rs.permutation(np.repeat(np.arange(8), n))
    x = (np.eye(8, D)[label] * (100 / np.sqrt(2)) + rs.standard_normal((8 * n, D))).astype(np.float32)
    first = np.array([np.nonzero(label == k)[0][0] for k in range(8)])
    xd, x64 = _dev16(x)
    init = xd[torch.from_numpy(first).cuda()].float()
    c2, c3 = coarse_train_bf16(xd, 8, iters=2, init=init), coarse_train_bf16(xd, 8, iters=3, init=init)
    again, a2, _, none = kmeans_step_bf16(xd, c2)
    assert none is None and torch.equal(again.view(torch.int32), c3.view(torch.int32))      # the trainer is `iters` steps
    assert torch.equal(coarse_train_bf16(xd, 8, iters=3, init=init).view(torch.int32), c3.view(torch.int32))
    _, a3, counts, changed = kmeans_step_bf16(xd, c3, prev_assign=a2)
    assert np.array_equal(a3.cpu().numpy(), label) and int(changed) == 0 and (counts.cpu().numpy() == n).all()
    assert torch.equal(coarse_assign_bf16(xd, c3), a3)
    for k in range(8):
        mean, mag = x64[label == k].mean(0), np.abs(x64[label == k]).mean(0)
        assert (np.abs(c3[k].cpu().numpy() - mean) <= 2.0 ** -24 * np.abs(mean) + n * 2.0 ** -53 * mag).all()
    dup = init.clone()
    dup[5] = dup[2]                                          # ties go to the lower list: list 5 gets no vector
    assert int(kmeans_step_bf16(xd, dup)[2][5]) == 0
    assert bool((kmeans_step_bf16(xd, coarse_train_bf16(xd, 8, iters=1, init=dup))[2] > 0).all())   # reseeded from the largest
    a, b = coarse_train_bf16(xd, 8, iters=2, seed=3), coarse_train_bf16(xd, 8, iters=2, seed=3)
    assert a.shape == (8, D) and a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))
