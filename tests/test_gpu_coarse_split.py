"""The coarse probes for fp32 queries by six bf16 plane products on the device (include/mcq_coarse_split.h rules 64-67) against
numpy float64, against mcq_kmeans_assign_split and against mcq_coarse_probe.  Every call of a C entry runs between guards
(tests/arena.py), outputs and scratch pre-filled with 0xA5; the inputs, the centroids' planes among them, are unchanged after."""
import numpy as np
import pytest
import torch

import arena
from test_gpu_bf16 import _planes
from test_gpu_coarse import METRICS, _run as _run32
from test_gpu_kmeans import _bits, _dev
from test_gpu_split import KEPT, _assign, _grid

pytestmark = pytest.mark.gpu


def _run(xd, cd, P, metric, parts=None, bias=True, terms=None):
    """planes and probe between guards -> (lists, scores, biases) as numpy.  terms: the caller's instead of coarse_terms'"""
    from quantization_amd import _lib, coarse_terms
    lib = _lib.lib()
    (Q, D), L = xd.shape, cd.shape[0]
    terms = coarse_terms(cd, metric) if terms is None else terms
    st = torch.cuda.current_stream().cuda_stream
    planes = arena.guarded((lib.mcq_kmeans_split_planes(L, D),), torch.int16)
    with arena.frozen(cd):
        assert lib.mcq_coarse_split_planes(cd.data_ptr(), L, D, planes.ptr, st) == 0
        torch.cuda.synchronize()
    parts = parts or lib.mcq_coarse_split_parts(Q, L, D, P)
    out = [arena.guarded((Q, P), torch.int32), arena.guarded((Q, P), torch.float32), arena.guarded((Q, P), torch.float32),
           arena.guarded((Q, parts, P), torch.float32), arena.guarded((Q, parts, P), torch.int32),
           arena.guarded((lib.mcq_kmeans_split_planes(Q, D),), torch.int16)]
    with arena.frozen(xd, cd, terms, planes.t):
        rc = lib.mcq_coarse_probe_split(xd.data_ptr(), Q, cd.data_ptr(), planes.ptr, L, D, None if terms is None else terms.data_ptr(),
                                        P, METRICS[metric], parts, out[0].ptr, out[1].ptr, out[2].ptr if bias else None, out[3].ptr,
                                        out[4].ptr, out[5].ptr, st)
        torch.cuda.synchronize()
    assert rc == 0 and planes.damage() is None and all(o.damage() is None for o in out) and (bias or out[2].untouched())
    part_list = out[4].t.cpu().numpy()
    assert L == 0 or ((part_list >= -1) & (part_list < L)).all()        # part buffers: written in full, with lists or the tail
    return tuple(o.t.cpu().numpy() for o in out[:3])


def _want(dot, terms, P, metric):
    """(lists, scores): the exact dot (a callable: a NaN row warns where it is formed) rounded once into the metric's fp32 formula, the P least by (score, list); a NaN is never
    listed, the tail is (-1, +inf)"""
    with np.errstate(all="ignore"):
        dot = (dot() + 0.0).astype(np.float32)
        t = None if terms is None else terms.cpu().numpy()[None, :]
        s = t - dot if metric == "l2" else (-dot if metric == "ip" else -(dot * t))
    order = np.argsort(s, axis=1, kind="stable")[:, :P]     # ties by the lower list (-0.0 == +0.0); NaN behind everything
    ws = np.take_along_axis(s, order, 1)
    pad = ((0, 0), (0, P - order.shape[1]))
    lists = np.pad(np.where(np.isnan(ws), -1, order), pad, constant_values=-1).astype(np.int32)
    return lists, np.pad(np.where(np.isnan(ws), np.inf, ws), pad, constant_values=np.inf).astype(np.float32)


# both sides of the query tiles (128; 64 for P > 64), the wave (32), the centroid tile (128), a step (16), the padding (32) and the
# classes of P (32 | 64); P > L gives the tail
@pytest.mark.parametrize("metric", tuple(METRICS))
@pytest.mark.parametrize("Q,L,D,P,offset", [
    (1, 1, 1, 1, 0), (33, 127, 16, 8, 1), (128, 128, 17, 33, 0), (129, 129, 40, 64, 1), (129, 300, 40, 65, 0), (33, 300, 17, 128, 1),
    (128, 127, 16, 128, 0), (1, 300, 40, 32, 0), (65, 129, 1, 8, 1), (129, 5, 16, 8, 0), (64, 300, 33, 64, 0), (33, 128, 40, 1, 1)])
def test_exact_grid(Q, L, D, P, offset, metric):
    """test_gpu_split._grid: all three planes of both rows hold something and every partial sum is exact, rows 0 and 1 come
    again at higher lists: lists and scores are, bit for bit, those of the float64 sum of the six kept products, with one part
    and with the most"""
    from quantization_amd import coarse_terms
    x, c, cd, _, _ = _grid(Q, L, D)
    xp, cp = _planes(x), _planes(c)
    wl, ws = _want(lambda: sum(xp[v] @ cp[w].T for v, w in KEPT), coarse_terms(cd, metric), P, metric)
    xd = _dev(x, offset)
    for parts in {1, -(-L // 128)}:
        lists, scores, _ = _run(xd, cd, P, metric, parts)
        assert np.array_equal(lists, wl) and np.array_equal(_bits(scores), _bits(ws)), parts


@pytest.mark.parametrize("metric", tuple(METRICS))
@pytest.mark.parametrize("Q,L,D,P", ((130, 300, 33, 8), (70, 40, 64, 43)))
def test_integer_rows_give_the_fp32_probe(Q, L, D, P, metric):
    """small integers are bf16 numbers and exact in both kernels: lists, scores and biases are mcq_coarse_probe's bit for bit;
    under l2 the first probe and its score are mcq_kmeans_assign_split's assign and score"""
    x, c, cd, _, _ = _grid(Q, L, D, three=False)
    got = _run(_dev(x), cd, P, metric)
    for mine, theirs in zip(got, _run32(x, c, P, metric)):
        assert np.array_equal(_bits(mine), _bits(theirs))
    if metric == "l2":
        assign, score, _ = _assign(_dev(x), cd)
        assert np.array_equal(got[0][:, 0], assign) and np.array_equal(_bits(got[1][:, 0]), _bits(score))


@pytest.mark.parametrize("P", (8, 64))
def test_gaussian_rows_against_float64(P):
    """Q = 200, L = 1,000, D = 96, l2, true fp32 rows: every reported score within tests/test_gpu_split.py's derived bound
    E = ((102 T + 2) 2^-23 + 2^-24) S + 2^-24 |h| of the float64 score of its listed centroid; the reported order ascends under
    (score, list); no unlisted centroid lies more than twice the row's largest E below the largest listed float64 score; the
    first probe and its score are mcq_kmeans_assign_split's bits (rule 65)"""
    from quantization_amd import coarse_terms
    Q, L, D = 200, 1000, 96
    rs = np.random.RandomState(P)
    x, c = rs.standard_normal((Q, D)).astype(np.float32), rs.standard_normal((L, D)).astype(np.float32)
    xd, cd = _dev(x), torch.from_numpy(c).cuda()
    h = coarse_terms(cd).cpu().numpy().astype(np.float64)[None, :]
    x64, c64 = x.astype(np.float64), c.astype(np.float64)
    ref = h - x64 @ c64.T
    bound = ((102 * -(-D // 16) + 2) * 2.0 ** -23 + 2.0 ** -24) * (np.abs(x64) @ np.abs(c64).T) + 2.0 ** -24 * np.abs(h)
    lists, scores, _ = _run(xd, cd, P, "l2", bias=False)
    assert (lists >= 0).all() and all(len(set(row)) == P for row in lists.tolist())
    listed = np.take_along_axis(ref, lists.astype(np.int64), 1)
    worst = float((np.abs(scores - listed) / np.take_along_axis(bound, lists.astype(np.int64), 1)).max())
    print(f"[coarse split] {Q} x {L} x {D}, P = {P}: largest error / bound {worst:.4f}")
    assert worst < 1
    assert ((np.diff(scores, axis=1) > 0) | ((np.diff(scores, axis=1) == 0) & (np.diff(lists, axis=1) > 0))).all()
    unlisted = ref.copy()
    np.put_along_axis(unlisted, lists.astype(np.int64), np.inf, 1)
    assert (unlisted.min(1) >= listed.max(1) - 2 * bound.max(1)).all()
    assign, score, _ = _assign(xd, cd)
    assert np.array_equal(lists[:, 0], assign) and np.array_equal(_bits(scores[:, 0]), _bits(score))


@pytest.mark.parametrize("kind", ("descending", "equal", "zeros", "inf", "nan"))
@pytest.mark.parametrize("P", (8, 128))
def test_hostile_orders(P, kind):
    """one part, Q = 33, L = 3,000, D = 8, all values exact.  descending: ip with c_l = l / 8 and positive queries: every centroid
    beats all before it and every offer goes through the heap; equal: the first P lists in order; zeros: l2 with the caller's
    terms, +0.0 and -0.0 in turn, against zero rows: equal scores, the lower lists, each with its own bits; inf: one +inf term
    among 99 finite scores (the rows from 100 on are NaN): listed last, behind them the tail; nan: a NaN row is never listed"""
    Q, L, D = 33, 3000, 8
    x, c = np.zeros((Q, D), np.float32), np.zeros((L, D), np.float32)
    x[:, 0], c[:, 0], c[:, D - 1] = 1 + np.arange(Q) % 3, np.arange(L) / 8.0, np.arange(L) % 7
    metric, terms = "ip", None
    if kind == "equal":
        c[:] = 3
    if kind == "zeros":
        c[:], metric, terms = 0, "l2", np.where(np.arange(L) % 2, -0.0, 0.0).astype(np.float32)
    if kind == "inf":
        metric, terms = "l2", np.zeros(L, np.float32)
        terms[5], c[100:] = np.inf, np.nan
    if kind == "nan":
        c[7, 0] = np.nan
    td = None if terms is None else torch.from_numpy(terms).cuda()
    wl, ws = _want(lambda: x.astype(np.float64) @ c.astype(np.float64).T, td, P, metric)
    lists, scores, _ = _run(_dev(x), torch.from_numpy(c).cuda(), P, metric, parts=1, terms=td)
    assert np.array_equal(lists, wl) and np.array_equal(_bits(scores), _bits(ws))
    assert kind != "inf" or ((lists[:, 99] == 5).all() and (lists[:, 100:] == -1).all() if P == 128 else not (lists == 5).any())
    assert kind != "nan" or not (lists == 7).any()


def test_no_lists():
    """L == 0 writes the tail and reads no input"""
    lists, scores, biases = _run(torch.ones((5, 8), device="cuda"), torch.zeros((0, 8), device="cuda"), 4, "ip",
                                 terms=torch.zeros(1, device="cuda"))
    assert (lists == -1).all() and np.isposinf(scores).all() and (_bits(biases) == 0).all()


@pytest.mark.parametrize("metric", ("l2", "ip", "cosine"))
def test_end_to_end_residual_search(metric):
    """tests/test_gpu_search_residual.py's recipe at its size: coarse_probe_split(with_bias=True) feeds
    search_lists(probe_bias=), every returned value within that file's derived bound (its docstring; the formulas below are
    its) of the float64 value at the returned index.  The probes are coarse_probe's, as sets, where the float64 scores of the
    4th and 5th list differ by more than twice test_gpu_coarse._bounds'"""
    import search_grid as sg
    import test_gpu_coarse as co
    import test_gpu_search as base
    import test_gpu_search_residual as res
    from quantization_amd import coarse_planes_split, coarse_probe, coarse_probe_split, list_assign
    qz, xq_d, codes, off, _, _, norms, rnorms, _, _, _ = res._setup()
    cen = (np.random.RandomState(21).standard_normal((res.NL, res.D)) * 2.0).astype(np.float32)      # _setup's first draw
    cd, qn = torch.from_numpy(cen).cuda(), xq_d.cpu().numpy()
    probes, bias = coarse_probe_split(xq_d, cd, res.NPROBE, planes=coarse_planes_split(cd), with_bias=True)
    s64 = np.sort(co._score64(qn, cen, "l2")[0], 1)
    clear = s64[:, res.NPROBE] - s64[:, res.NPROBE - 1] > 2 * co._bounds(qn, cen, "l2")[0].max(1)
    p32 = coarse_probe(xq_d, cd, res.NPROBE).cpu().numpy()
    assert clear.any() and np.array_equal(np.sort(probes.cpu().numpy(), 1)[clear], np.sort(p32, 1)[clear])
    val, idx = qz.search_lists(xq_d, codes, off, probes, k=res.KTOP, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias)
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
