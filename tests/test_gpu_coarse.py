"""The coarse probes on the device (mcq_coarse_probe, include/mcq_coarse.h rules 40-43) against numpy float64.

Every call of the C entry here runs between guards (tests/arena.py): outputs and part buffers of exactly the stated sizes,
pre-filled with 0xA5 between 64 KiB of 0x5C; the guards are intact and the inputs unchanged after every call.

The bound of the real-input tests.  u = 2^-23 (twice the unit roundoff: each product is rounded and so is each addition), A =
sum_e |q_e c_e|, cc = sum_e c_e^2.  A dot of D rounded products added in ANY order, zero padding included, is within
(D + 4) u A of the exact one (first order, with room for the step's inner pair); that is E_dot, and the bias fl(-2 dot') is
within 2 E_dot (doubling is exact).  The term's share: h = fl(0.5 cc) is within (D + 4) u cc / 2, and the subtraction adds
u (|h| + |dot|) at most; r = 1 / sqrt(cc) carries half the relative error of cc plus a root and a division, (D + 8) u r at
most, and the product one more rounding, so E_cos = (E_dot + |dot| (D + 9) u) r.  E is the largest bound of a query's row.
Two score sequences that differ by at most E elementwise have order statistics that differ by at most E, so: every list whose
float64 score beats the float64 P-th best by more than 2 E is present, and every listed one lies within 2 E of it."""
import numpy as np
import pytest
import torch

import arena

pytestmark = pytest.mark.gpu
U = 2.0 ** -23
METRICS = {"l2": 0, "ip": 1, "cosine": 2}


def _score64(q, c, metric):
    q, c = q.astype(np.float64), c.astype(np.float64)
    with np.errstate(all="ignore"):
        dot, cc = q @ c.T + 0.0, (c * c).sum(1)              # (+ 0.0: an accumulator that starts at +0.0 is never -0.0)
        if metric == "l2":
            return 0.5 * cc[None] - dot, dot
        r = np.where(cc == 0, 0.0, 1.0 / np.sqrt(np.where(cc == 0, 1.0, cc)))
        return (-dot if metric == "ip" else -(dot * r[None])), dot


def _run(q, c, P, metric, parts=None, bias=True):
    """the C entry between guards -> (lists, scores, biases) as numpy"""
    from quantization_amd import _lib, coarse_terms
    lib = _lib.lib()
    qd, cd = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    (Q, D), L = q.shape, c.shape[0]
    terms = coarse_terms(cd, metric)
    parts = parts or lib.mcq_coarse_parts(Q, L, D, P)
    out = [arena.guarded((Q, P), torch.int32), arena.guarded((Q, P), torch.float32), arena.guarded((Q, P), torch.float32),
           arena.guarded((Q, parts, P), torch.float32), arena.guarded((Q, parts, P), torch.int32)]
    with arena.frozen(qd, cd, terms):
        rc = lib.mcq_coarse_probe(qd.data_ptr(), Q, cd.data_ptr(), L, D, None if terms is None else terms.data_ptr(), P,
                                  METRICS[metric], parts, out[0].ptr, out[1].ptr, out[2].ptr if bias else None, out[3].ptr,
                                  out[4].ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0 and all(o.damage() is None for o in out) and (bias or out[2].untouched())
    part_list = out[4].t.cpu().numpy()
    assert ((part_list >= -1) & (part_list < L)).all()       # part buffers: written in full, with lists or the tail
    return tuple(o.t.cpu().numpy() for o in out[:3])


def _exact(q, c, P, metric, parts=None):
    """inputs whose every product and partial sum is exact in fp32: lists, scores and biases bit for bit"""
    s64, dot = _score64(q, c, metric)
    order = np.argsort(s64, axis=1, kind="stable")[:, :P]   # ties by the lower index; NaN behind everything
    want_s = np.take_along_axis(s64, order, 1)
    none = np.isnan(want_s)
    want_l = np.where(none, -1, order)
    with np.errstate(all="ignore"):
        want_b = np.where(none, 0.0, -2.0 * np.take_along_axis(dot, order, 1))
    pad = ((0, 0), (0, P - order.shape[1]))
    want_l = np.pad(want_l, pad, constant_values=-1).astype(np.int32)
    want_s = np.pad(np.where(none, np.inf, want_s), pad, constant_values=np.inf).astype(np.float32)
    want_b = np.pad(want_b, pad, constant_values=0.0).astype(np.float32)
    lists, scores, biases = _run(q, c, P, metric, parts)
    assert np.array_equal(lists, want_l)
    assert np.array_equal(scores.view(np.uint32), want_s.view(np.uint32))
    assert np.array_equal(biases.view(np.uint32), want_b.view(np.uint32))


@pytest.mark.parametrize("Q,L,D,P,parts,metric", [
    (1, 1, 1, 1, 1, "l2"), (31, 127, 2, 5, 1, "ip"), (33, 129, 3, 64, 2, "l2"), (65, 300, 31, 128, 3, "ip"),
    (1, 300, 33, 128, 2, "l2"), (33, 127, 70, 128, 1, "l2"), (65, 129, 70, 5, 2, "ip"), (31, 300, 1, 64, 3, "l2"),
    (33, 1, 33, 5, 1, "ip"), (65, 300, 2, 1, 1, "l2")])
def test_exact_grid(Q, L, D, P, parts, metric):
    rs = np.random.RandomState(Q + L + D + P)
    _exact(rs.randint(-4, 5, (Q, D)).astype(np.float32), rs.randint(-4, 5, (L, D)).astype(np.float32), P, metric, parts)


@pytest.mark.parametrize("P", (1, 128))
@pytest.mark.parametrize("order", ("descending", "identical", "nan_query", "inf_centroid"))
def test_hostile_orders(order, P):
    L = 1000
    q = np.array([[1, 0], [0, 1], [-1, 0], [2, 1]], np.float32)
    c = np.stack([np.arange(1, L + 1), np.arange(L) % 7], 1).astype(np.float32)      # ip: every tile beats every bound of rows 0, 3
    if order == "identical":
        c[:] = (3, -2)
    if order == "nan_query":
        q[1, 0] = np.nan
    if order == "inf_centroid":
        c[5] = (np.inf, 0)                                   # -inf for row 0, NaN for row 1, +inf for row 2
    _exact(q, c, P, "ip")
    if order != "inf_centroid":                              # (inf - inf: a NaN score in both, but h itself is checked elsewhere)
        _exact(q, c, P, "l2", parts=3)


def _real(shape):
    Q, L, D, P = shape
    rs = np.random.RandomState(D)
    return rs.standard_normal((Q, D)).astype(np.float32), rs.standard_normal((L, D)).astype(np.float32)


def _bounds(q, c, metric):
    """(E per (query, list), the bias' bound): the docstring's"""
    D = q.shape[1]
    a, cc = np.abs(q.astype(np.float64)) @ np.abs(c.astype(np.float64)).T, (c.astype(np.float64) ** 2).sum(1)[None]
    dot = np.abs(_score64(q, c, "ip")[0])
    e_dot = (D + 4) * U * a
    if metric == "l2":
        return e_dot + (D + 4) * U * cc / 2 + U * (cc / 2 + dot), 2 * e_dot
    return (e_dot if metric == "ip" else (e_dot + dot * (D + 9) * U) / np.sqrt(cc)), 2 * e_dot


@pytest.mark.parametrize("metric", tuple(METRICS))
@pytest.mark.parametrize("shape", ((37, 1000, 96, 10), (5, 300, 515, 128)))
def test_real_inputs_against_float64(shape, metric):
    q, c = _real(shape)
    P = shape[3]
    lists, scores, biases = _run(q, c, P, metric)
    s64, dot = _score64(q, c, metric)
    e, e_bias = _bounds(q, c, metric)
    for j in range(shape[0]):
        got = lists[j].astype(np.int64)
        assert (got >= 0).all() and len(set(got.tolist())) == P
        E, kth = e[j].max(), np.sort(s64[j])[P - 1]
        assert (np.abs(scores[j] - s64[j, got]) <= e[j, got]).all()
        assert np.isin(np.nonzero(s64[j] < kth - 2 * E)[0], got).all() and (s64[j, got] <= kth + 2 * E).all()
        assert (np.diff(scores[j]) >= 0).all()
        assert (np.abs(biases[j] + 2 * dot[j, got]) <= e_bias[j, got]).all()


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_a_function_of_the_rows_alone(metric):
    q, c = _real((65, 300, 70, 5))
    lists, scores, biases = _run(q, c, 5, metric, parts=1)
    for other in (_run(q, c, 5, metric, parts=3), _run(q[17:18], c, 5, metric, parts=2)):
        at = slice(17, 18) if other[0].shape[0] == 1 else slice(None)
        assert all(np.array_equal(a[at].view(np.uint32), b.view(np.uint32)) for a, b in zip((lists, scores, biases), other))
    rs = np.random.RandomState(3)
    pq, pc = rs.permutation(65), rs.permutation(300)
    l2, s2, b2 = _run(q[pq], c[pc], 5, metric, parts=2)
    assert np.array_equal(pc[l2], lists[pq]) and np.array_equal(s2.view(np.uint32), scores[pq].view(np.uint32))
    assert np.array_equal(b2.view(np.uint32), biases[pq].view(np.uint32))


def test_coarse_assign():
    from quantization_amd import coarse_assign, coarse_probe
    rs = np.random.RandomState(5)
    x, c = rs.randint(-4, 5, (1000, 3)).astype(np.float32), rs.randint(-4, 5, (129, 3)).astype(np.float32)
    got = coarse_assign(torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda())
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), _score64(x, c, "l2")[0].argmin(1))
    x, c = rs.standard_normal((1000, 40)).astype(np.float32), rs.standard_normal((129, 40)).astype(np.float32)
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    got = coarse_assign(xd, cd).cpu().numpy().astype(np.int64)
    s64 = _score64(x, c, "l2")[0]
    E = _bounds(x, c, "l2")[0].max(1)
    two = np.sort(s64, 1)[:, :2]
    clear = two[:, 1] - two[:, 0] > 2 * E
    assert clear.mean() > 0.9 and np.array_equal(got[clear], s64.argmin(1)[clear])
    assert (s64[np.arange(1000), got] <= two[:, 0] + 2 * E).all()
    assert torch.equal(coarse_probe(xd.reshape(10, 100, 40), cd, 1).reshape(-1), torch.from_numpy(got).int().cuda())


def test_a_refused_call_writes_nothing():
    from quantization_amd import _lib
    lib = _lib.lib()
    ins = torch.ones(64 * 8, device="cuda")
    outs = [arena.guarded((8, 4), torch.float32) for _ in range(5)]
    for D, P, metric in ((0, 4, 0), (8, 129, 0), (8, 4, 7)):
        rc = lib.mcq_coarse_probe(ins.data_ptr(), 8, ins.data_ptr(), 8, D, ins.data_ptr(), P, metric, 1, outs[0].ptr, outs[1].ptr,
                                  outs[2].ptr, outs[3].ptr, outs[4].ptr, None)
        torch.cuda.synchronize()
        assert rc in (_lib.MCQ_EINVAL, _lib.MCQ_EUNSUPPORTED) and all(o.untouched() and o.damage() is None for o in outs)


@pytest.mark.parametrize("metric", ("l2", "ip", "cosine"))
def test_end_to_end_residual_search(metric):
    """coarse_probe(with_bias=True) feeds search_lists on the residual recipe of test_gpu_search_residual: every returned value
    within that test's derived bound of the float64 distance to c_l + decode"""
    import test_gpu_search_residual as res
    from quantization_amd import coarse_probe
    qz, xq_d, codes, off, _, _, norms, rnorms, exact, bound, _ = res._setup()
    cen = (np.random.RandomState(21).standard_normal((res.NL, res.D)) * 2.0).astype(np.float32)      # _setup's first draw
    probes, bias = coarse_probe(xq_d, torch.from_numpy(cen).cuda(), res.NPROBE, with_bias=True)
    val, idx = qz.search_lists(xq_d, codes, off, probes, k=res.KTOP, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias)
    val, idx, off_h = val.cpu().numpy().astype(np.float64), idx.cpu().numpy(), off.cpu().numpy()
    for j, row in enumerate(probes.cpu().numpy()):
        cand = np.concatenate([np.arange(off_h[l], off_h[l + 1]) for l in row])
        assert len(set(row.tolist())) == res.NPROBE and np.isin(idx[j], cand).all()
        assert (np.abs(val[j] - exact[metric][j, idx[j]]) <= bound[metric][j, idx[j]]).all()
