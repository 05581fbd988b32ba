"""The assignment of fp32 rows by six bf16 plane products (include/mcq_split.h rules 60-63) against numpy float64, the bf16 and
the fp32 entries, and coarse_train_split end to end.  Every call of a C entry runs between the guards of tests/arena.py."""
import numpy as np
import pytest
import torch

import arena
from test_gpu_bf16 import _assign as _assign16, _dev16, _planes
from test_gpu_kmeans import _bits, _dev

pytestmark = pytest.mark.gpu
VT = 128                                                     # vectors of the assign kernel's tile
KEPT = ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))      # rule 61: (vector plane, centroid plane), 0 = hi, 1 = mid, 2 = lo
THREE = np.float32(1 + 2.0 ** -9 + 2.0 ** -18)               # planes 1, 2^-9 and 2^-18, each below half an ulp of the one before


def _assign(x, c, parts=None, prev=None):
    """the C entry between guards -> (assign, score, changed) as numpy / int"""
    from quantization_amd import _lib, coarse_terms
    lib = _lib.lib()
    (B, D), L = x.shape, c.shape[0]
    terms = coarse_terms(c)
    parts = parts or lib.mcq_kmeans_split_parts(B, L, D)
    out = [arena.guarded((B,), torch.int32), arena.guarded((B,), torch.float32), arena.guarded((1,), torch.int32),
           arena.guarded((B, parts), torch.float32), arena.guarded((B, parts), torch.int32),
           arena.guarded((lib.mcq_kmeans_split_planes(L, D),), torch.int16)]
    with arena.frozen(x, c, terms, prev):
        rc = lib.mcq_kmeans_assign_split(x.data_ptr(), B, c.data_ptr(), L, D, terms.data_ptr(), parts, None if prev is None else
                                         prev.data_ptr(), *(o.ptr for o in out), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out) and (prev is not None or out[2].untouched())
    return out[0].t.cpu().numpy(), out[1].t.cpu().numpy(), None if prev is None else int(out[2].t[0])


def _grid(B, L, D, three=True):
    """vector and centroid elements integers in [-1, 1]: hi only.  With `three`, element b % D of vector b and element l % D of
    centroid l are +-THREE instead, so a three-plane vector element meets ordinary centroid elements in most pairs and a
    three-plane one where b % D == l % D.  Plane p of either side is a multiple of 2^(-9 p), so each of the six kept products
    is a multiple of 2^-18; asserted here, with the sum of their magnitudes below 2^24 of it (64, hence the small integers):
    every partial sum is exact in fp32 in any order.  Rows 0 and 1 of c come again at a higher index, the second one in another
    tile where there is one -> (x, c, c on the device, the expected assign and score: fl(h[l] - dot) in fp32 with dot the
    float64 sum of the six kept plane products and h as coarse_terms (shipped code) makes it)"""
    from quantization_amd import coarse_terms
    rs = np.random.RandomState(1000 * B + 10 * L + D)
    x, c = rs.randint(-1, 2, (B, D)).astype(np.float32), rs.randint(-1, 2, (L, D)).astype(np.float32)
    if three:
        for a in (x, c):
            rows = np.arange(len(a))
            a[rows, rows % D] = (1 - 2 * (rows % 2)) * THREE
    if L > 1:
        c[L - 1] = c[0]
    if L > 200:
        c[200] = c[1]
    xp, cp = _planes(x), _planes(c)
    for planes, a in ((xp, x), (cp, c)):
        assert np.array_equal(sum(planes), a.astype(np.float64)) and all(p.any() for p in planes) == three
        assert all((p % 2.0 ** (-9 * k) == 0).all() for k, p in enumerate(planes))
    dot = sum(xp[v] @ cp[w].T for v, w in KEPT)
    assert sum(np.abs(xp[v]) @ np.abs(cp[w]).T for v, w in KEPT).max() < 2.0 ** 24 * 2.0 ** -18 and (dot % 2.0 ** -18 == 0).all()
    cd = torch.from_numpy(c).cuda()
    s = coarse_terms(cd).cpu().numpy()[None, :] - dot.astype(np.float32)
    return x, c, cd, s.argmin(1), s.min(1)


@pytest.mark.parametrize("B,L,D,offset", [
    (1, 1, 1, 0), (VT - 1, 129, 15, 1), (VT, 127, 16, 0), (VT + 1, 128, 17, 1), (2 * VT + 1, 300, 33, 0), (1, 300, 64, 0), (300, 1, 65, 1),
    (VT + 1, 300, 80, 0), (VT, 128, 64, 1), (VT - 1, 127, 80, 1), (2 * VT + 1, 129, 16, 1), (VT + 1, 129, 36, 0)])
def test_assign_exact(B, L, D, offset):
    """bit for bit, ties to the lower list, one part and the most; offset 1 or D % 4 != 0: the element-wise loads; D = 36: a group of four past the row's end"""
    x, c, cd, want, score = _grid(B, L, D)
    xd = _dev(x, offset)
    assert xd.data_ptr() % 16 == 4 * offset
    for parts in {1, -(-L // 128)}:
        got, gs, _ = _assign(xd, cd, parts)
        assert np.array_equal(got, want) and np.array_equal(_bits(gs), _bits(score)), parts


@pytest.mark.parametrize("B,L,D", ((2 * 256 + 1, 129, 48), (257, 300, 33)))
def test_bf16_valued_rows_give_the_bf16_entry(B, L, D):
    """rule 61: on Gaussian rows rounded to bf16 and widened, the bits of mcq_kmeans_assign_bf16 on the bf16 rows"""
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((L, D)).astype(np.float32)
    (xd, _), cd = _dev16(x), torch.from_numpy(c).cuda()
    a16, s16, _ = _assign16(xd, cd)
    a32, s32, _ = _assign(xd.float(), cd)
    assert np.array_equal(a16, a32) and np.array_equal(_bits(s16), _bits(s32))


def test_assign_nan_inf_and_changed():
    """a NaN row and an inf element (a NaN mid: rule 62): (-1, +inf), the neighbours keep their bits; `changed` counts exactly"""
    x, c, cd, want, score = _grid(VT + 1, 300, 33)
    got, gs, none = _assign(_dev(x), cd)
    assert none is None and np.array_equal(got, want) and np.array_equal(_bits(gs), _bits(score))
    assert _assign(_dev(x), cd, 3, prev=torch.from_numpy(got).cuda())[2] == 0
    prev = got.copy()
    prev[[0, 5, 64, 100, VT]] += 1
    assert _assign(_dev(x), cd, 2, prev=torch.from_numpy(prev).cuda())[2] == 5
    x[64, 3], x[70, 5] = np.nan, np.inf
    got2, gs2, _ = _assign(_dev(x), cd, 2)
    assert (got2[[64, 70]] == -1).all() and (gs2[[64, 70]] == np.inf).all()
    keep = ~np.isin(np.arange(VT + 1), (64, 70))
    assert np.array_equal(got2[keep], want[keep]) and np.array_equal(_bits(gs2[keep]), _bits(score[keep]))


@pytest.mark.parametrize("B,L,D", ((500, 300, 96), (300, 129, 65)))
def test_assign_real_inputs(B, L, D):
    """Gaussian fp32 rows against the float64 value of h[l] - <x, c> on the true rows, S = sum_e |x_e| |c_e|.  Products of two
    bf16 numbers are exact in fp32; a step adds 96 products and rounds the accumulator 6 times, each addition off by at most
    2^-23 of a partial sum of magnitudes (<= S): 102 T 2^-23 S over T = ceil(D / 16) steps.  The three products that are not
    formed are below (2^-27 + 2^-27 + 2^-36) S < 2 2^-23 S, and the last subtraction rounds once.  So |score - ref| <=
    1.01 (((102 T + 2) 2^-23 + 2^-24) S + 2^-24 |h|).  assign is the float64 argmin wherever the float64 gap between best and
    second exceeds twice the row's largest bound; at most 1 % of rows are excused."""
    from quantization_amd import coarse_terms
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((L, D)).astype(np.float32)
    xd, cd = _dev(x), torch.from_numpy(c).cuda()
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    h = coarse_terms(cd).cpu().numpy().astype(np.float64)
    ref = h[None, :] - x64 @ c64.T
    S = np.abs(x64) @ np.abs(c64).T
    bound = 1.01 * (((102 * -(-D // 16) + 2) * 2.0 ** -23 + 2.0 ** -24) * S + 2.0 ** -24 * np.abs(h)[None, :])
    got, score, _ = _assign(xd, cd)
    rows = np.arange(B)
    ratio = float((np.abs(score - ref[rows, got]) / bound[rows, got]).max()) if (got >= 0).all() else np.inf
    two = np.sort(ref, 1)[:, :2]
    sure = two[:, 1] - two[:, 0] > 2 * bound.max(1)
    print(f"[split assign] {B} x {L} x {D}: largest error / bound {ratio:.4f}, excused rows {int((~sure).sum())}")
    assert ratio < 1 and (~sure).mean() <= 0.01 and np.array_equal(got[sure], ref.argmin(1)[sure])


def test_step_is_the_fp32_step_on_exact_inputs():
    """integer rows and centroids (_grid without the three-plane elements) are exact in both kernels: kmeans_step_split's four
    results, mcq_kmeans_update behind the new assignment, are kmeans_step's bit for bit, list 4 empty (row 4 of c is row 0)"""
    from quantization_amd import kmeans_step, kmeans_step_split
    x, c, cd, _, _ = _grid(300, 5, 33, three=False)
    assert np.array_equal(c[4], c[0])
    xd = _dev(x)
    p = torch.zeros(300, dtype=torch.int32, device="cuda")
    new6, a6, n6, ch6 = kmeans_step_split(xd, cd, prev_assign=p)
    new32, a32, n32, ch32 = kmeans_step(xd, cd, prev_assign=p)
    assert torch.equal(new6.view(torch.int32), new32.view(torch.int32)) and torch.equal(a6, a32) and torch.equal(n6, n32)
    assert int(ch6) == int(ch32) == int((a32 != 0).sum()) and int(n32[4]) == 0 and int(n32.sum()) == 300
    assert torch.equal(new6[4].view(torch.int32), cd[4].view(torch.int32))


def test_coarse_train_split_end_to_end():
    """tests/test_gpu_kmeans.py's 8 blobs, init one point of each.  After 3 steps assign is the blob label and every centroid
    element lies within 2^-24 |mean| + n 2^-53 mean(|x|) of the float64 blob mean; the same bits twice."""
    from quantization_amd import coarse_assign_split, coarse_train_split, kmeans_step_split
    rs = np.random.RandomState(0)
    D, n = 33, 300
    label = rs.permutation(np.repeat(np.arange(8), n))
    x = (np.eye(8, D)[label] * (100 / np.sqrt(2)) + rs.standard_normal((8 * n, D))).astype(np.float32)
    first = np.array([np.nonzero(label == k)[0][0] for k in range(8)])
    xd, x64 = _dev(x), x.astype(np.float64)
    init = xd[torch.from_numpy(first).cuda()].clone()
    c2, c3 = coarse_train_split(xd, 8, iters=2, init=init), coarse_train_split(xd, 8, iters=3, init=init)
    again, a2, _, none = kmeans_step_split(xd, c2)
    assert none is None and torch.equal(again.view(torch.int32), c3.view(torch.int32))      # the trainer is `iters` steps
    assert torch.equal(coarse_train_split(xd, 8, iters=3, init=init).view(torch.int32), c3.view(torch.int32))
    _, a3, counts, changed = kmeans_step_split(xd, c3, prev_assign=a2)
    assert np.array_equal(a3.cpu().numpy(), label) and int(changed) == 0 and (counts.cpu().numpy() == n).all()
    assert torch.equal(coarse_assign_split(xd, c3), a3)
    for k in range(8):
        mean, mag = x64[label == k].mean(0), np.abs(x64[label == k]).mean(0)
        assert (np.abs(c3[k].cpu().numpy() - mean) <= 2.0 ** -24 * np.abs(mean) + n * 2.0 ** -53 * mag).all()
    assert coarse_train_split(xd, 8, iters=1, seed=3).shape == (8, D)
