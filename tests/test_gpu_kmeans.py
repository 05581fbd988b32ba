"""The Lloyd step on the device (mcq_kmeans_assign, mcq_kmeans_update, include/mcq_kmeans.h rules 44-47) against numpy float64,
and coarse_train end to end.  Every call of a C entry here runs between guards (tests/arena.py): outputs and scratch buffers of
exactly the stated sizes between 64 KiB of 0x5C; the guards are intact and the inputs unchanged after every call."""
import numpy as np
import pytest
import torch

import arena

pytestmark = pytest.mark.gpu
SIZES = (0, 1, 1023, 1025, 4097, 2 * 4096 + 1024 + 37)      # the last: two blocks and a ragged second quarter of the third


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev(a, offset=0):
    """a on the device; offset = 1: a view whose base is 4 bytes past a 16-byte boundary, so the element-wise loads run"""
    flat = torch.empty(a.size + offset, dtype=torch.float32, device="cuda")
    view = flat[offset:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    return view


def _assign(x, c, parts=None, prev=None):
    """the C entry between guards -> (assign, score, changed) as numpy / int"""
    from quantization_amd import _lib, coarse_terms
    lib = _lib.lib()
    (B, D), L = x.shape, c.shape[0]
    terms = coarse_terms(c)
    parts = parts or lib.mcq_kmeans_parts(B, L, D)
    out = [arena.guarded((B,), torch.int32), arena.guarded((B,), torch.float32), arena.guarded((1,), torch.int32),
           arena.guarded((B, parts), torch.float32), arena.guarded((B, parts), torch.int32)]
    with arena.frozen(x, c, terms, prev):
        rc = lib.mcq_kmeans_assign(x.data_ptr(), B, c.data_ptr(), L, D, terms.data_ptr(), parts,
                                   None if prev is None else prev.data_ptr(), out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr,
                                   out[4].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out) and (prev is not None or out[2].untouched())
    return out[0].t.cpu().numpy(), out[1].t.cpu().numpy(), None if prev is None else int(out[2].t[0])


@pytest.mark.parametrize("B,L,D,parts,offset", [
    (1, 1, 1, 1, 0), (127, 127, 3, 1, 0), (129, 129, 31, 2, 0), (257, 300, 33, 3, 0), (257, 127, 70, 1, 1), (1, 300, 70, 2, 0),
    (127, 129, 1, 2, 0), (129, 300, 3, 1, 1), (257, 1, 31, 1, 0), (129, 129, 64, 1, 0), (257, 300, 64, 3, 1)])
def test_assign_exact(B, L, D, parts, offset):
    """integers in [-4, 4]: every product and partial sum is exact in fp32, so assign and score are float64's, bit for bit,
    ties to the lower list (np.argmin's).  D = 64 takes the 16-byte loads, and with offset = 1 leaves them again"""
    rs = np.random.RandomState(B + L + D)
    x, c = rs.randint(-4, 5, (B, D)).astype(np.float32), rs.randint(-4, 5, (L, D)).astype(np.float32)
    s64 = 0.5 * (c.astype(np.float64) ** 2).sum(1)[None] - x.astype(np.float64) @ c.astype(np.float64).T + 0.0
    want = s64.argmin(1)
    got, score, _ = _assign(_dev(x, offset), _dev(c, offset), parts)
    assert np.array_equal(got, want)
    assert np.array_equal(_bits(score), _bits(s64[np.arange(B), want].astype(np.float32)))


@pytest.mark.parametrize("B,L,D", ((257, 300, 70), (129, 129, 33)))
def test_assign_is_the_shipped_probe(B, L, D):
    from quantization_amd import _lib, coarse_assign, coarse_terms
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((L, D)).astype(np.float32)
    xd, cd = _dev(x), _dev(c)
    want = coarse_assign(xd, cd).cpu().numpy()
    ws, wl, ps, pl = (torch.empty(B, dtype=t, device="cuda") for t in (torch.float32, torch.int32) * 2)
    assert _lib.lib().mcq_coarse_probe(xd.data_ptr(), B, cd.data_ptr(), L, D, coarse_terms(cd).data_ptr(), 1, 0, 1, wl.data_ptr(),
                                       ws.data_ptr(), None, ps.data_ptr(), pl.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    for parts in (1, 2):                                     # with and without a centroid split
        got, score, _ = _assign(xd, cd, parts)
        assert np.array_equal(got, want) and np.array_equal(_bits(score), _bits(ws.cpu().numpy()))
    assert _assign(xd, cd, prev=torch.from_numpy(got).cuda())[2] == 0
    prev = got.copy()
    prev[[0, 5, 64, 100, B - 1]] += 1
    assert _assign(xd, cd, 2, prev=torch.from_numpy(prev).cuda())[2] == 5
    x[64, 3] = np.nan                                        # every score of row 64 is NaN; its neighbours keep their bits
    got2, score2, _ = _assign(_dev(x), cd)
    assert got2[64] == -1 and score2[64] == np.inf
    keep = np.arange(B) != 64
    assert np.array_equal(got2[keep], got[keep]) and np.array_equal(_bits(score2[keep]), _bits(score[keep]))


def _update(xd, order, offsets, cin):
    """the C entry between guards -> (centroids_out, counts) as numpy"""
    from quantization_amd import _lib
    lib = _lib.lib()
    (B, D), L = xd.shape, cin.shape[0]
    od, fd, cd = torch.from_numpy(order).cuda(), torch.from_numpy(offsets).cuda(), torch.from_numpy(cin).cuda()
    out = [arena.guarded((L, D), torch.float32), arena.guarded((L,), torch.int32), arena.guarded((L + 1,), torch.int64),
           arena.guarded((lib.mcq_kmeans_blocks(B, L, D),), torch.float64)]
    with arena.frozen(xd, od, fd, cd):
        rc = lib.mcq_kmeans_update(xd.data_ptr(), B, D, od.data_ptr(), fd.data_ptr(), L, cd.data_ptr(), out[0].ptr, out[1].ptr,
                                   out[2].ptr, out[3].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out)
    return out[0].t.cpu().numpy(), out[1].t.cpu().numpy()


def _tree_mean(rows, n):
    """rule 47 restated: rows (members, D) float64 in member order, a member that names no row as zeros; n those that do"""
    total = np.zeros(rows.shape[1])
    for b0 in range(0, len(rows), 4096):
        q = [np.zeros(rows.shape[1]) for _ in range(4)]
        for j in range(4):
            for r in rows[b0 + 1024 * j:min(b0 + 1024 * (j + 1), b0 + 4096)]:
                q[j] = q[j] + r
        total = total + (((q[0] + q[1]) + q[2]) + q[3])
    return (total / n).astype(np.float32)


@pytest.mark.parametrize("D", (1, 5, 1027))
@pytest.mark.parametrize("kind", ("integer", "gaussian"))
def test_update_against_the_tree(kind, D):
    """integer rows: every float64 partial sum is exact, so the mean is (x64[members].sum(0) / n).astype(float32); Gaussian
    rows: the header's tree, bit for bit.  Then the same lists at other indexes of a longer store: the same rows"""
    rs = np.random.RandomState(D)
    B, L = sum(SIZES), len(SIZES)
    x = rs.randint(-4, 5, (B, D)).astype(np.float32) if kind == "integer" else rs.standard_normal((B, D)).astype(np.float32)
    order, offsets = rs.permutation(B).astype(np.int64), np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    order[offsets[3] + 7], order[offsets[5] + 5000] = -1, B  # two entries that name no row: skipped, not counted
    cin = rs.standard_normal((L, D)).astype(np.float32)
    xd = _dev(x)
    got, counts = _update(xd, order, offsets, cin)
    x64, named = x.astype(np.float64), (order >= 0) & (order < B)
    for l in range(L):
        at = slice(offsets[l], offsets[l + 1])
        n = int(named[at].sum())
        assert counts[l] == n == SIZES[l] - (l in (3, 5))
        want = cin[l] if n == 0 else _tree_mean(x64[order[at].clip(0, B - 1)] * named[at, None], n)
        assert np.array_equal(_bits(got[l]), _bits(want)), l
        if kind == "integer" and n:
            assert np.array_equal(_bits(got[l]), _bits((x64[order[at][named[at]]].sum(0) / n).astype(np.float32)))
    place = np.array([8, 6, 0, 3, 1, 4])                     # list l of the first store is list place[l] of 9
    sizes2 = np.zeros(9, np.int64)
    sizes2[place] = SIZES
    offsets2 = np.concatenate([[0], np.cumsum(sizes2)]).astype(np.int64)
    order2 = np.concatenate([order[offsets[l]:offsets[l + 1]] for l in np.argsort(place)])
    cin2 = rs.standard_normal((9, D)).astype(np.float32)
    got2, counts2 = _update(xd, order2, offsets2, cin2)
    assert np.array_equal(_bits(got2[place[1:]]), _bits(got[1:])) and np.array_equal(counts2[place], counts)
    empty = np.setdiff1d(np.arange(9), place[1:])
    assert np.array_equal(_bits(got2[empty]), _bits(cin2[empty])) and not counts2[empty].any()


def test_coarse_train_end_to_end():
    """8 blobs in D = 33, centres 100 apart, spread 1, 300 points each, init one point of each.  After 3 steps assign is the blob
    label and nothing changes; every centroid element lies within 2^-24 |mean| + n 2^-53 mean(|x|) of the float64 blob mean
    (one fp32 rounding of the quotient; n float64 additions and the division, each within 2^-53 of the running magnitude)."""
    from quantization_amd import coarse_train, kmeans_step
    rs = np.random.RandomState(0)
    D, n = 33, 300
    label = rs.permutation(np.repeat(np.arange(8), n))
    x = (np.eye(8, D)[label] * (100 / np.sqrt(2)) + rs.standard_normal((8 * n, D))).astype(np.float32)
    first = np.array([np.nonzero(label == k)[0][0] for k in range(8)])
    xd, init = _dev(x), _dev(x[first])
    c2, c3 = coarse_train(xd, 8, iters=2, init=init), coarse_train(xd, 8, iters=3, init=init)
    again, a2, _, none = kmeans_step(xd, c2)
    assert none is None and torch.equal(again.view(torch.int32), c3.view(torch.int32))      # the trainer is `iters` steps
    assert torch.equal(coarse_train(xd, 8, iters=3, init=init).view(torch.int32), c3.view(torch.int32))
    _, a3, counts, changed = kmeans_step(xd, c3, prev_assign=a2)
    assert np.array_equal(a3.cpu().numpy(), label) and int(changed) == 0 and (counts.cpu().numpy() == n).all()
    x64 = x.astype(np.float64)
    for k in range(8):
        mean, mag = x64[label == k].mean(0), np.abs(x64[label == k]).mean(0)
        assert (np.abs(c3[k].cpu().numpy() - mean) <= 2.0 ** -24 * np.abs(mean) + n * 2.0 ** -53 * mag).all()
    dup = init.clone()
    dup[5] = dup[2]                                          # ties go to the lower list: list 5 gets no vector
    assert int(kmeans_step(xd, dup)[2][5]) == 0
    assert bool((kmeans_step(xd, coarse_train(xd, 8, iters=1, init=dup))[2] > 0).all())      # reseeded from the largest list
    a, b = coarse_train(xd, 8, iters=2, seed=3), coarse_train(xd, 8, iters=2, seed=3)
    assert a.shape == (8, D) and torch.equal(a.view(torch.int32), b.view(torch.int32))
