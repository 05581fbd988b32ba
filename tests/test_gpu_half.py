"""The Lloyd step over an fp16 store on the device (mcq_kmeans_assign_half, mcq_kmeans_update_half, include/mcq_half.h rules
48-51) against numpy float64 and against the fp32 entries, and coarse_train_half end to end.  Every call of a C entry here runs
between guards (tests/arena.py): outputs and scratch (the planes among them) of exactly the stated sizes, pre-filled with 0xA5,
between 64 KiB of 0x5C; the guards are intact and the inputs unchanged after every call."""
import numpy as np
import pytest
import torch

import arena
from test_gpu_kmeans import _bits, _update

pytestmark = pytest.mark.gpu


def _dev16(a, offset=0):
    """a (float16) on the device; offset = 1: a view whose base is 2 bytes past a 16-byte boundary: the 2-byte loads run"""
    flat = torch.empty(a.size + offset, dtype=torch.float16, device="cuda")
    view = flat[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _assign(x, c, parts=None, prev=None):
    """the C entry between guards -> (assign, score, changed) as numpy / int"""
    from quantization_amd import _lib, coarse_terms
    lib = _lib.lib()
    (B, D), L = x.shape, c.shape[0]
    terms = coarse_terms(c)
    parts = parts or lib.mcq_kmeans_half_parts(B, L, D)
    out = [arena.guarded((B,), torch.int32), arena.guarded((B,), torch.float32), arena.guarded((1,), torch.int32),
           arena.guarded((B, parts), torch.float32), arena.guarded((B, parts), torch.int32),
           arena.guarded((lib.mcq_kmeans_half_planes(L, D),), torch.int16)]
    with arena.frozen(x, c, terms, prev):
        rc = lib.mcq_kmeans_assign_half(x.data_ptr(), B, c.data_ptr(), L, D, terms.data_ptr(), parts,
                                        None if prev is None else prev.data_ptr(), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                        out[4].ptr, out[5].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out) and (prev is not None or out[2].untouched())
    return out[0].t.cpu().numpy(), out[1].t.cpu().numpy(), None if prev is None else int(out[2].t[0])


def _grid(B, L, D):
    """vector elements integers in [-2, 2]; centroid elements a + b 2^-13, |a| <= 4, |b| <= 7: hi + lo 2^-11 is the element and
    every partial sum of either accumulator, and their sum, is a multiple of 2^-13 below 2^10 -- exact in fp32 in any order.
    Rows 0 and 1 come again at a higher index, the second one in another tile where there is one"""
    rs = np.random.RandomState(1000 * B + 10 * L + D)
    x = rs.randint(-2, 3, (B, D)).astype(np.float16)
    c = (rs.randint(-4, 5, (L, D)) + rs.randint(-7, 8, (L, D)) * 2.0 ** -13).astype(np.float32)
    if L > 1:
        c[L - 1] = c[0]
    if L > 200:
        c[200] = c[1]
    return x, c


def _exact(x, c, cd):
    """the expected (assign, score): fl(h[l] - dot) in fp32 with the exact dot, h as coarse_terms (shipped code) makes it"""
    from quantization_amd import coarse_terms
    h = coarse_terms(cd).cpu().numpy()
    s = h[None, :] - (x.astype(np.float64) @ c.astype(np.float64).T).astype(np.float32)
    assert s.dtype == np.float32
    want = s.argmin(1)
    return want, s[np.arange(len(x)), want]


@pytest.mark.parametrize("B,L,D,offset", [
    (1, 1, 1, 0), (127, 129, 15, 1), (128, 127, 16, 0), (129, 128, 17, 1), (300, 300, 33, 0), (1, 300, 64, 0), (300, 1, 65, 1),
    (129, 300, 80, 0), (128, 128, 64, 1), (127, 127, 80, 1), (300, 129, 16, 1), (129, 129, 33, 0)])
def test_assign_exact(B, L, D, offset):
    """assign and score are float64's, bit for bit, ties to the lower list (np.argmin's), with one part and with the most.
    D % 8 == 0 at offset 0 takes the 16-byte loads; offset 1 leaves them for a base that is 2-byte aligned only"""
    x, c = _grid(B, L, D)
    xd, cd = _dev16(x, offset), torch.from_numpy(c).cuda()
    assert xd.data_ptr() % 4 == 2 * offset
    want, score = _exact(x, c, cd)
    for parts in {1, -(-L // 128)}:
        got, gs, _ = _assign(xd, cd, parts)
        assert np.array_equal(got, want) and np.array_equal(_bits(gs), _bits(score)), parts


def test_assign_nan_inf_and_changed():
    """a NaN row and a row with an fp16 inf against a zero column (inf * 0 is NaN in both planes): (-1, +inf), the neighbours
    keep their bits; `changed` counts against a shifted prev_assign"""
    x, c = _grid(129, 300, 33)
    c[:, 5] = 0
    cd = torch.from_numpy(c).cuda()
    want, score = _exact(x, c, cd)
    got, gs, none = _assign(_dev16(x), cd)
    assert none is None and np.array_equal(got, want) and np.array_equal(_bits(gs), _bits(score))
    assert _assign(_dev16(x), cd, 3, prev=torch.from_numpy(got).cuda())[2] == 0
    prev = got.copy()
    prev[[0, 5, 64, 100, 128]] += 1
    assert _assign(_dev16(x), cd, 2, prev=torch.from_numpy(prev).cuda())[2] == 5
    x[64, 3], x[70, 5] = np.nan, np.inf
    got2, gs2, _ = _assign(_dev16(x), cd, 2)
    assert (got2[[64, 70]] == -1).all() and (gs2[[64, 70]] == np.inf).all()
    keep = ~np.isin(np.arange(129), (64, 70))
    assert np.array_equal(got2[keep], want[keep]) and np.array_equal(_bits(gs2[keep]), _bits(score[keep]))


@pytest.mark.parametrize("B,L,D", ((500, 300, 96), (300, 129, 65)))
def test_assign_real_inputs(B, L, D):
    """Gaussian rows.  The reference is the float64 value of h[l] - sum_e v_e (hi_e + lo_e 2^-11), S = sum_e |v_e| (|hi_e| +
    |lo_e| 2^-11).  The bound: the products of two fp16 numbers are exact, and over T = ceil(D / 16) steps an accumulator takes
    16 T products and T accumulator additions; in whatever order and with rounding or chopping inside the instruction each of
    those 17 T additions errs by at most u = 2^-23 of a partial sum of magnitudes, which never exceeds the plane's share of S.
    Scaling A_lo by 2^-11 is exact; fl(A_hi + .) and fl(h - dot) each round once, 2^-24 |dot| <= 2^-24 S and 2^-24 (|h| + S).
    So |score - ref| <= (17 T u + 2^-23) S + 2^-24 |h|, times 1.01 for the second-order terms.  assign is the float64 argmin
    wherever the float64 gap between best and second exceeds twice the row's largest bound; at most 1 % of rows are excused."""
    from quantization_amd import coarse_terms
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((B, D)).astype(np.float16), rs.standard_normal((L, D)).astype(np.float32)
    cd = torch.from_numpy(c).cuda()
    hi = c.astype(np.float16)
    lo = ((c - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    x64, c64 = x.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11
    h = coarse_terms(cd).cpu().numpy().astype(np.float64)
    ref = h[None, :] - x64 @ c64.T
    S = np.abs(x64) @ (np.abs(hi.astype(np.float64)) + np.abs(lo.astype(np.float64)) * 2.0 ** -11).T
    bound = 1.01 * ((17 * -(-D // 16) * 2.0 ** -23 + 2.0 ** -23) * S + 2.0 ** -24 * np.abs(h)[None, :])
    got, score, _ = _assign(_dev16(x), cd)
    rows = np.arange(B)
    assert (got >= 0).all()
    ratio = float((np.abs(score - ref[rows, got]) / bound[rows, got]).max())
    two = np.sort(ref, 1)[:, :2]
    sure = two[:, 1] - two[:, 0] > 2 * bound.max(1)
    print(f"[half assign] {B} x {L} x {D}: largest error / bound {ratio:.4f}, excused rows {int((~sure).sum())}")
    assert ratio < 1 and (~sure).mean() <= 0.01 and np.array_equal(got[sure], ref.argmin(1)[sure])


@pytest.mark.parametrize("D", (1, 65, 68, 1030))
def test_update_is_the_fp32_update_on_widened_rows(D):
    """9,000 Gaussian fp16 rows in 3 lists of 5,300 (two blocks, a ragged second quarter of the second), 0 and 3,700 members, two
    order entries that name no row: centroids_out and counts of mcq_kmeans_update on the rows widened to fp32, bit for bit.
    D = 68 takes the 8-byte loads, 1,030 a second slab"""
    from quantization_amd import _lib
    lib = _lib.lib()
    rs = np.random.RandomState(D)
    B, L = 9000, 3
    x = rs.standard_normal((B, D)).astype(np.float16)
    order, offsets = rs.permutation(B).astype(np.int64), np.array([0, 5300, 5300, B], np.int64)
    order[7], order[5400] = -1, B
    cin = rs.standard_normal((L, D)).astype(np.float32)
    xd = _dev16(x)
    want, wcounts = _update(xd.float(), order, offsets, cin)
    od, fd, cd = torch.from_numpy(order).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(cin).cuda()
    out = [arena.guarded((L, D), torch.float32), arena.guarded((L,), torch.int32), arena.guarded((L + 1,), torch.int64),
           arena.guarded((lib.mcq_kmeans_blocks(B, L, D),), torch.float64)]
    with arena.frozen(xd, od, fd, cd):
        rc = lib.mcq_kmeans_update_half(xd.data_ptr(), B, D, od.data_ptr(), fd.data_ptr(), L, cd.data_ptr(), out[0].ptr, out[1].ptr,
                                        out[2].ptr, out[3].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out)
    assert np.array_equal(_bits(out[0].t.cpu().numpy()), _bits(want)) and np.array_equal(out[1].t.cpu().numpy(), wcounts)
    assert list(wcounts) == [5299, 0, 3699] and np.array_equal(_bits(want[1]), _bits(cin[1]))


def test_coarse_train_half_end_to_end():
    """tests/test_gpu_kmeans.py's blobs as fp16 rows: 8 blobs in D = 33, centres 100 apart, spread 1, 300 points each, init one
    point of each.  After 3 steps assign is the blob label; every centroid element lies within 2^-24 |mean| + n 2^-53 mean(|x|)
    of the float64 mean of the fp16 rows (one fp32 rounding of the quotient; n float64 additions and the division)."""
    from quantization_amd import coarse_assign_half, coarse_train_half, kmeans_step_half
    rs = np.random.RandomState(0)
    D, n = 33, 300
    label = rs.permutation(np.repeat(np.arange(8), n))
    x = (np.eye(8, D)[label] * (100 / np.sqrt(2)) + rs.standard_normal((8 * n, D))).astype(np.float16)
    first = np.array([np.nonzero(label == k)[0][0] for k in range(8)])
    xd, init = _dev16(x), torch.from_numpy(x[first].astype(np.float32)).cuda()
    c2, c3 = coarse_train_half(xd, 8, iters=2, init=init), coarse_train_half(xd, 8, iters=3, init=init)
    again, a2, _, none = kmeans_step_half(xd, c2)
    assert none is None and torch.equal(again.view(torch.int32), c3.view(torch.int32))      # the trainer is `iters` steps
    assert torch.equal(coarse_train_half(xd, 8, iters=3, init=init).view(torch.int32), c3.view(torch.int32))
    _, a3, counts, changed = kmeans_step_half(xd, c3, prev_assign=a2)
    assert np.array_equal(a3.cpu().numpy(), label) and int(changed) == 0 and (counts.cpu().numpy() == n).all()
    assert torch.equal(coarse_assign_half(xd, c3), a3)
    x64 = x.astype(np.float64)
    for k in range(8):
        mean, mag = x64[label == k].mean(0), np.abs(x64[label == k]).mean(0)
        assert (np.abs(c3[k].cpu().numpy() - mean) <= 2.0 ** -24 * np.abs(mean) + n * 2.0 ** -53 * mag).all()
    dup = init.clone()
    dup[5] = dup[2]                                          # ties go to the lower list: list 5 gets no vector
    assert int(kmeans_step_half(xd, dup)[2][5]) == 0
    assert bool((kmeans_step_half(xd, coarse_train_half(xd, 8, iters=1, init=dup))[2] > 0).all())   # reseeded from the largest
    a, b = coarse_train_half(xd, 8, iters=2, seed=3), coarse_train_half(xd, 8, iters=2, seed=3)
    assert a.shape == (8, D) and a.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("B,L,D,most", ((257, 129, 16, 2), (129, 300, 33, 3)))
def test_assign_is_the_fp32_assign_on_exact_inputs(B, L, D, most):
    """_grid inputs: every product and partial sum is exact in fp32 in any order, so mcq_kmeans_assign on the widened rows and
    mcq_kmeans_assign_half on the fp16 rows give the same assign, the same score bits and the same `changed` against a shifted
    prev_assign, with one part and with the most.  (257, 129, 16): a last vector tile of one row, two centroid tiles, the
    16-byte loads of both kernels; (129, 300, 33): the element-wise loads"""
    from test_gpu_kmeans import _assign as _assign32
    x, c = _grid(B, L, D)
    xd, cd = _dev16(x), torch.from_numpy(c).cuda()
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
    """kmeans_step_half(x16, c, prev_assign=p) and kmeans_step(x16.float(), c, prev_assign=p) on _grid(300, 5, 33), row 4 of c a
    copy of row 0 (list 4 is empty and keeps its centroid): the same new centroids bit for bit, the same assign, counts and
    changed -- one _step and one sums kernel behind both"""
    from quantization_amd import kmeans_step, kmeans_step_half
    x, c = _grid(300, 5, 33)
    assert np.array_equal(c[4], c[0])
    xd, cd = _dev16(x), torch.from_numpy(c).cuda()
    p = torch.zeros(300, dtype=torch.int32, device="cuda")
    new16, a16, n16, ch16 = kmeans_step_half(xd, cd, prev_assign=p)
    new32, a32, n32, ch32 = kmeans_step(xd.float(), cd, prev_assign=p)
    assert torch.equal(new16.view(torch.int32), new32.view(torch.int32)) and torch.equal(a16, a32) and torch.equal(n16, n32)
    assert int(ch16) == int(ch32) == int((a32 != 0).sum()) and int(n32[4]) == 0
    assert torch.equal(new32[4].view(torch.int32), cd[4].view(torch.int32)) and int(n32.sum()) == 300
