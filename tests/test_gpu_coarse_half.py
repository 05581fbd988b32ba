"""The coarse probes for fp16 queries on the device (include/mcq_coarse_half.h rules 52-55) against numpy float64, against
mcq_kmeans_assign_half and against mcq_coarse_probe on the widened queries.  Every call of a C entry runs between guards
(tests/arena.py), outputs pre-filled with 0xA5; the inputs, the planes among them, are unchanged after every call."""
import numpy as np
import pytest
import torch

import arena
from test_gpu_coarse import METRICS
from test_gpu_half import _assign, _dev16, _grid
from test_gpu_kmeans import _bits

pytestmark = pytest.mark.gpu


def _terms(cd, metric):
    from quantization_amd import coarse_terms
    return coarse_terms(cd, metric) if cd.shape[0] else None


def _run(xd, cd, P, metric, parts=None, bias=True, terms=None):
    """split and probe between guards -> (lists, scores, biases) as numpy.  terms: the caller's instead of coarse_terms'"""
    from quantization_amd import _lib
    lib = _lib.lib()
    (Q, D), L = xd.shape, cd.shape[0]
    terms = _terms(cd, metric) if terms is None else terms
    st = torch.cuda.current_stream().cuda_stream
    planes = arena.guarded((lib.mcq_kmeans_half_planes(L, D),), torch.int16)
    with arena.frozen(cd):
        assert lib.mcq_coarse_half_split(cd.data_ptr(), L, D, planes.ptr, st) == 0
        torch.cuda.synchronize()
    parts = parts or lib.mcq_coarse_half_parts(Q, L, D, P)
    out = [arena.guarded((Q, P), torch.int32), arena.guarded((Q, P), torch.float32), arena.guarded((Q, P), torch.float32),
           arena.guarded((Q, parts, P), torch.float32), arena.guarded((Q, parts, P), torch.int32)]
    with arena.frozen(xd, cd, terms, planes.t):
        rc = lib.mcq_coarse_probe_half(xd.data_ptr(), Q, cd.data_ptr(), planes.ptr, L, D, None if terms is None else terms.data_ptr(),
                                       P, METRICS[metric], parts, out[0].ptr, out[1].ptr, out[2].ptr if bias else None, out[3].ptr,
                                       out[4].ptr, st)
        torch.cuda.synchronize()
    assert rc == 0 and planes.damage() is None and all(o.damage() is None for o in out) and (bias or out[2].untouched())
    part_list = out[4].t.cpu().numpy()
    assert L == 0 or ((part_list >= -1) & (part_list < L)).all()        # part buffers: written in full, with lists or the tail
    return tuple(o.t.cpu().numpy() for o in out[:3])


def _want(x, c, terms, P, metric):
    """(lists, scores): the float64 dot rounded once into the metric's fp32 formula, the P least by (score, list); a NaN is
    never listed, the tail is (-1, +inf)"""
    with np.errstate(all="ignore"):
        dot = (x.astype(np.float64) @ c.astype(np.float64).T + 0.0).astype(np.float32)
        t = None if terms is None else terms.cpu().numpy()[None, :]
        s = t - dot if metric == "l2" else (-dot if metric == "ip" else -(dot * t))
    assert s.dtype == np.float32
    order = np.argsort(s, axis=1, kind="stable")[:, :P]     # ties by the lower list; NaN behind everything
    ws = np.take_along_axis(s, order, 1)
    pad = ((0, 0), (0, P - order.shape[1]))
    lists = np.pad(np.where(np.isnan(ws), -1, order), pad, constant_values=-1).astype(np.int32)
    return lists, np.pad(np.where(np.isnan(ws), np.inf, ws), pad, constant_values=np.inf).astype(np.float32)


# both sides of the query tile (64), the centroid tile (64), a step (16), a chunk (32), the classes of P (16 | 64) and the sort
# trigger (M - P - 32 pending entries: 0 at P = 96, where every block with an offer sorts)
@pytest.mark.parametrize("metric", tuple(METRICS))
@pytest.mark.parametrize("Q,L,D,P,offset", [
    (1, 1, 1, 1, 0), (33, 129, 15, 7, 1), (65, 127, 16, 128, 0), (129, 300, 33, 128, 1), (5, 3, 17, 8, 0), (127, 257, 80, 1, 1),
    (64, 128, 64, 32, 0), (31, 300, 65, 33, 1), (128, 129, 32, 96, 0), (129, 129, 72, 97, 1), (63, 65, 48, 16, 1), (2, 64, 8, 65, 0),
    (66, 130, 40, 17, 0), (3, 200, 24, 64, 1)])
def test_exact_grid(Q, L, D, P, offset, metric):
    """_grid inputs: every partial sum is exact and rows 0 and 1 come again at higher lists, so lists and scores are the
    reference's bit for bit with one part and with the most; the biases are -2 x the exact dot"""
    x, c = _grid(Q, L, D)
    xd, cd = _dev16(x, offset), torch.from_numpy(c).cuda()
    assert xd.data_ptr() % 4 == 2 * offset
    wl, ws = _want(x, c, _terms(cd, metric), P, metric)
    wb = np.where(wl < 0, 0.0, -2.0 * np.take_along_axis(x.astype(np.float64) @ c.astype(np.float64).T + 0.0, np.maximum(wl, 0), 1))
    for parts in {1, -(-L // 64)}:
        lists, scores, biases = _run(xd, cd, P, metric, parts)
        assert np.array_equal(lists, wl) and np.array_equal(_bits(scores), _bits(ws)), parts
        assert np.array_equal(_bits(biases), _bits(wb.astype(np.float32))), parts


@pytest.mark.parametrize("B,L,D", ((500, 300, 96), (300, 129, 65)))
def test_first_probe_is_the_shipped_assign(B, L, D):
    """Gaussian rows, P = 1, l2: list and score are mcq_kmeans_assign_half's assign and score, bit for bit (rule 53)"""
    rs = np.random.RandomState(D)
    xd = _dev16(rs.standard_normal((B, D)).astype(np.float16))
    cd = torch.from_numpy(rs.standard_normal((L, D)).astype(np.float32)).cuda()
    assign, score, _ = _assign(xd, cd)
    lists, scores, _ = _run(xd, cd, 1, "l2", bias=False)
    assert np.array_equal(lists[:, 0], assign) and np.array_equal(_bits(scores[:, 0]), _bits(score))


@pytest.mark.parametrize("metric", tuple(METRICS))
@pytest.mark.parametrize("Q,L,D,P", ((37, 1000, 96, 8), (5, 300, 65, 128)))
def test_real_inputs_against_float64(Q, L, D, P, metric):
    """Gaussian rows against the float64 value of the score over the two planes, within test_assign_real_inputs' derived bound
    (tests/test_gpu_half.py): |dot - dot64| <= (17 T u + 2^-24) S and one rounding of the score: l2 (17 T u + 2^-23) S + 2^-24
    |h|; ip no more than (17 T u + 2^-23) S; cosine that times r, and 2^-24 |dot r| for its multiply; times 1.01 for the
    second-order terms.  With E the row's largest bound: every centroid more than 2 E below the float64 P-th score is listed,
    none more than 2 E above it, and the reported scores ascend.  No case is excused."""
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((Q, D)).astype(np.float16), rs.standard_normal((L, D)).astype(np.float32)
    cd = torch.from_numpy(c).cuda()
    hi = c.astype(np.float16)
    lo = ((c - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    x64, c64 = x.astype(np.float64), hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -11
    dot = x64 @ c64.T
    S = np.abs(x64) @ (np.abs(hi.astype(np.float64)) + np.abs(lo.astype(np.float64)) * 2.0 ** -11).T
    e_dot = (17 * -(-D // 16) * 2.0 ** -23 + 2.0 ** -23) * S
    t = None if metric == "ip" else _terms(cd, metric).cpu().numpy().astype(np.float64)[None, :]
    ref, bound = {"l2": lambda: (t - dot, e_dot + 2.0 ** -24 * np.abs(t)), "ip": lambda: (-dot, e_dot),
                  "cosine": lambda: (-(dot * t), e_dot * t + 2.0 ** -24 * np.abs(dot * t))}[metric]()
    bound = 1.01 * bound
    lists, scores, _ = _run(_dev16(x), cd, P, metric)
    worst = 0.0
    for j in range(Q):
        got = lists[j].astype(np.int64)
        assert (got >= 0).all() and len(set(got.tolist())) == P
        worst = max(worst, float((np.abs(scores[j] - ref[j, got]) / bound[j, got]).max()))
        E, kth = bound[j].max(), np.sort(ref[j])[P - 1]
        assert np.isin(np.nonzero(ref[j] < kth - 2 * E)[0], got).all() and (ref[j, got] <= kth + 2 * E).all()
        assert (np.diff(scores[j]) >= 0).all()
    print(f"[coarse half] {metric} {Q} x {L} x {D}, P = {P}: largest error / bound {worst:.4f}")
    assert worst < 1


@pytest.mark.parametrize("metric", ("l2", "ip"))
@pytest.mark.parametrize("D", (33, 64))
def test_bias_is_the_fp32_probe_bias(D, metric):
    """P = L + 3 = 43: both entries list every centroid, so entry by entry, matched by list, out_bias has the bits
    mcq_coarse_probe reports on the queries widened to fp32; the three tail entries carry 0"""
    from test_gpu_coarse import _run as run32
    rs = np.random.RandomState(D)
    x, c = rs.standard_normal((33, D)).astype(np.float16), rs.standard_normal((40, D)).astype(np.float32)
    lists, _, biases = _run(_dev16(x), torch.from_numpy(c).cuda(), 43, metric)
    l32, _, b32 = run32(x.astype(np.float32), c, 43, metric)
    assert (lists[:, 40:] == -1).all() and (_bits(biases[:, 40:]) == 0).all() and (np.sort(lists[:, :40], 1) == np.arange(40)).all()
    by16, by32 = np.argsort(lists[:, :40], 1), np.argsort(l32[:, :40], 1)
    assert np.array_equal(_bits(np.take_along_axis(biases, by16, 1)), _bits(np.take_along_axis(b32, by32, 1)))


@pytest.mark.parametrize("kind", ("descending", "equal", "nan", "inf"))
@pytest.mark.parametrize("Q", (1, 33))
def test_hostile_orders(Q, kind):
    """L = 1,000, P = 128, D = 1 (one query) or 2, all values exact.  descending: ip with c_l = l / 8 and positive queries: every
    centroid beats every bound and every block of offers fills; equal: the first P lists in order; nan: a NaN centroid is never
    listed; inf: l2 with the caller's terms, 0 but for one +inf: not listed among 999 finite scores, and listed behind the 99
    finite ones when the rows from 100 on are NaN.  Distinct scores: the same result for permuted rows, the lists mapped back"""
    L, P, D = 1000, 128, 1 if Q == 1 else 2
    x, c = np.zeros((Q, D), np.float16), np.zeros((L, D), np.float32)
    x[:, 0], c[:, 0] = 1 + np.arange(Q) % 3, np.arange(L) / 8.0
    c[:, D - 1] += (np.arange(L) % 7) * (D - 1)              # (D = 2: a column the queries hold 0 against)
    metric, terms = "ip", None
    if kind == "equal":
        c[:] = 3
    if kind == "nan":
        c[7, 0] = np.nan
    if kind == "inf":
        metric, terms = "l2", np.zeros(L, np.float32)
        terms[5] = np.inf
    xd = _dev16(x)
    for finite in ((L, 100) if kind == "inf" else (L,)):
        cc = c.copy()
        cc[finite:] = np.nan
        td = None if terms is None else torch.from_numpy(terms).cuda()
        wl, ws = _want(x, cc, td, P, metric)
        lists, scores, _ = _run(xd, torch.from_numpy(cc).cuda(), P, metric, terms=td)
        assert np.array_equal(lists, wl) and np.array_equal(_bits(scores), _bits(ws))
        if kind == "inf":
            assert (lists[:, 99] == 5).all() == (finite == 100) and not (lists[:, :99] == 5).any()
        if kind != "equal":
            perm = np.random.RandomState(Q).permutation(L)
            tp = None if terms is None else torch.from_numpy(terms[perm]).cuda()
            l2, s2, _ = _run(xd, torch.from_numpy(cc[perm]).cuda(), P, metric, parts=3, terms=tp)
            assert np.array_equal(np.where(l2 < 0, -1, perm[np.maximum(l2, 0)]), lists) and np.array_equal(_bits(s2), _bits(scores))


def test_no_lists():
    """L == 0 writes the tail and reads no input"""
    lists, scores, biases = _run(_dev16(np.ones((5, 8), np.float16)), torch.zeros((0, 8), device="cuda"), 4, "ip")
    assert (lists == -1).all() and np.isposinf(scores).all() and (_bits(biases) == 0).all()


@pytest.mark.parametrize("metric", ("l2", "ip", "cosine"))
def test_end_to_end_residual_search(metric):
    """tests/test_gpu_search_residual.py's recipe at its size, its queries rounded to fp16: coarse_probe_half(with_bias=True)
    feeds search_lists(probe_bias=), every returned value within that file's derived bound (its docstring; the formulas below
    are its, on the rounded queries) of the float64 value at the returned index.  The probes are coarse_probe's on the widened
    queries, as sets, where the float64 scores of the 4th and 5th list differ by more than twice test_gpu_coarse._bounds'"""
    import search_grid as sg
    import test_gpu_coarse as co
    import test_gpu_search as base
    import test_gpu_search_residual as res
    from quantization_amd import coarse_planes, coarse_probe, coarse_probe_half, list_assign
    qz, xq_d, codes, off, _, _, norms, rnorms, _, _, _ = res._setup()
    cen = (np.random.RandomState(21).standard_normal((res.NL, res.D)) * 2.0).astype(np.float32)      # _setup's first draw
    cd, q16 = torch.from_numpy(cen).cuda(), xq_d.half()
    probes, bias = coarse_probe_half(q16, cd, res.NPROBE, planes=coarse_planes(cd), with_bias=True)
    qn = q16.float().cpu().numpy()
    s64 = np.sort(co._score64(qn, cen, "l2")[0], 1)
    clear = s64[:, res.NPROBE] - s64[:, res.NPROBE - 1] > 2 * co._bounds(qn, cen, "l2")[0].max(1)
    p32 = coarse_probe(q16.float(), cd, res.NPROBE).cpu().numpy()
    assert clear.any() and np.array_equal(np.sort(probes.cpu().numpy(), 1)[clear], np.sort(p32, 1)[clear])
    val, idx = qz.search_lists(q16.float(), codes, off, probes, k=res.KTOP, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias)
    val, idx, off_h = val.cpu().numpy().astype(np.float64), idx.cpu().numpy(), off.cpu().numpy()
    D, N, EPS = res.D, res.N, res.EPS
    C, flat, l_of = base._centers(qz), codes.cpu().numpy(), list_assign(off, res.B).cpu().numpy().astype(np.int64)
    q64, C64, cen64 = qn.astype(np.float64), C.astype(np.float64), cen.astype(np.float64)
    xhat, mag, A_r = cen64[l_of] + base._decode64(C, flat), np.abs(cen64)[l_of], np.zeros((res.Q, res.B))
    for n in range(N):
        mag = mag + np.abs(C64[n])[flat[:, n]]
        A_r += (np.abs(q64) @ np.abs(C64[n]).T)[:, flat[:, n]]
    A_c = (np.abs(q64) @ np.abs(cen64).T)[:, l_of]
    M, t, qq = (mag ** 2).sum(1)[None, :], (xhat ** 2).sum(1)[None, :], (q64 ** 2).sum(1)[:, None]
    E_sb, E_t = 2 * EPS * ((D + N + 3) * A_r + (D + 2) * A_c), 4 * max(N, sg.norms_chains(N, D)[1]) * EPS * M
    ip = q64 @ xhat.T
    exact = {"l2": ((q64[:, None, :] - xhat[None]) ** 2).sum(2), "ip": ip, "cosine": ip / np.sqrt(qq * t)}[metric]
    bound = {"l2": E_sb + E_t + 2 * EPS * (2 * (A_r + A_c) + M) + (D + 3) * EPS * qq, "ip": E_sb / 2,
             "cosine": E_sb / 2 / np.sqrt(qq * t) + np.abs(ip / np.sqrt(qq * t)) * (E_t / (2 * t) + ((D + 1) / 2 + 5) * EPS)}[metric]
    for j, row in enumerate(probes.cpu().numpy()):
        cand = np.concatenate([np.arange(off_h[l], off_h[l + 1]) for l in row])
        assert len(set(row.tolist())) == res.NPROBE and np.isin(idx[j], cand).all()
        assert (np.abs(val[j] - exact[j, idx[j]]) <= bound[j, idx[j]]).all()
