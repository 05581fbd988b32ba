"""The search over stored codes (Quantizer.search_tables / code_norms / _search_scan / search; include/mcq.h rules 1-5) on the GPU.

Oracles are numpy only.  Per case:
  * tables and norms against float64, ENTRY BY ENTRY, within  c * L * 2^-24 * S  (the bound form of test_gpu_train_kernels.py):
      tables: S = 2 * sum_d |q[d]| |C[n][k][d]|, L = the padded dim (one chain over d), c = 2: a rounded product and L additions
              per entry give (L + 1) * 2^-24 * S to first order; c = 2 covers the higher-order terms;
      norms:  S = sum_d (sum_n |C[n][code][d]|)^2, L = the longer of the row-addition chain (N - 1) and the accumulation chain
              (four per float4 group of a lane plus six butterfly levels), c = 4: the row sum's error enters the square twice
              (2 * (N - 1)), the square rounds once and the accumulation adds its chain -- at most 3 * L + 1 roundings;
  * _search_scan scores and indexes, and search indexes, EQUAL (bit for bit) to rules 3 and 4 restated in numpy
    (tests/search_grid.py) from the tables and norms the GPU returned -- every row, no near-tie allowance;
  * distances of the returned positions against float64 |q - decode64(codes[b])|^2 within the sum of the N table bounds and the
    norm bound above plus D * 2^-24 * |q|^2, the rounding of |q|^2 (D rounded squares and additions in any order);
  * a second call returns identical bits.
The largest error / bound ratios are printed (run with -s) and written to the JSON file MCQ_SEARCH_RATIOS names, if set."""
import json
import os

import numpy as np
import pytest
import torch

import search_grid as sg

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
RATIOS = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_d512_b8_p2.npz")


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    path = os.environ.get("MCQ_SEARCH_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _note(case, what, ratio):
    RATIOS[f"{case}:{what}"] = ratio
    print(f"[search] {case}: largest error / bound of {what} = {ratio:.4f}")


def _quantizer(case):
    from quantization_amd import Quantizer
    from quantization_amd import synthetic as gen
    if case.state == "trained":
        z = np.load(GOLDEN)
        sd = {k[len("state."):]: z[k] for k in z.files if k.startswith("state.") and k != "state.id_buf"}
        assert (int(z["D"]), int(z["K"]), int(z["N"])) == (case.D, case.K, case.N)
    else:
        sd = gen.synthetic_state(11 + case.N + case.K, case.D, case.K, case.N)
    q = Quantizer(case.D, case.K, case.N)
    st = q.state_dict()
    for k_, v in sd.items():
        st[k_] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(st)
    return q.to("cuda:0").requires_grad_(False)


def _centers(q):
    """the fp32 rows of `prepared` that mcq_decode sums, (N, K, D)"""
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    Dp = (D + 15) & ~15
    blob = q._prepared(any_flavour=True)
    torch.cuda.synchronize()
    C = blob[:N * K * Dp * 4].view(torch.float32).reshape(N, K, Dp).cpu().numpy()
    assert not C[:, :, D:].any()
    return np.ascontiguousarray(C[:, :, :D])


def _store(case, q):
    """(codes as the caller keeps them, unpacked uint8 (B, N) numpy)"""
    from quantization_amd import synthetic as gen
    N, K, B = case.N, case.K, case.B
    rs = np.random.RandomState(1000 + B % 977 + N)
    if case.codes == "encode":
        chunks = []
        for a in range(0, B, 262144):
            x = gen.make_gaussian(31 + a, min(262144, B - a), case.D)
            chunks.append(q.encode(torch.from_numpy(x).cuda(), refine_indexes_iters=2))
        kept = torch.cat(chunks)
        assert q._prep.flavour == "host"
    else:
        assert not case.packed
        if case.codes == "dup16":
            kept = rs.randint(0, K, size=(16, N)).astype(np.uint8)[rs.randint(0, 16, size=B)]
        else:
            kept = rs.randint(0, K, size=(B, N)).astype(np.uint8)
        kept = torch.from_numpy(kept).cuda()
        if case.state == "decode_only":
            q.decode(kept[:1])
            assert q._prep.flavour == "decode"
    flat = kept.cpu().numpy()
    if flat.shape[1] != N:
        assert case.packed and K == 16 and flat.shape[1] * 2 == N
        flat = np.stack([flat & 15, flat >> 4], axis=2).reshape(B, N)
    else:
        assert not case.packed
    return kept, np.ascontiguousarray(flat)


def _queries(case, q, kept):
    from quantization_amd import synthetic as gen
    x = gen.make_gaussian(77 + case.Q, case.Q, case.D)
    if case.queries == "stored":
        rows = np.random.RandomState(3).randint(0, case.B, size=case.Q)
        return q.decode(kept[torch.from_numpy(rows).cuda()]), rows
    xq = torch.from_numpy(x).cuda()
    return (xq.half() if case.queries == "fp16" else xq), None


def _decode64(C, flat):
    out = np.zeros((flat.shape[0], C.shape[2]))
    for n in range(C.shape[0]):
        out += C[n].astype(np.float64)[flat[:, n]]
    return out


def _check_tables(case, qh, C, T):
    N, K, D = C.shape
    L = sg.tables_chain(D)
    q64, C64 = qh.astype(np.float64), C.astype(np.float64).reshape(N * K, D)
    ref = -2.0 * q64 @ C64.T
    S = 2.0 * np.abs(q64) @ np.abs(C64).T
    bound = 2 * L * EPS * S
    err = np.abs(T.reshape(len(qh), N * K).astype(np.float64) - ref)
    _note(case.name, "tables", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), f"{int((err > bound).sum())} table entries out of bound"
    return bound.reshape(len(qh), N, K)


def _check_norms(case, C, flat, t):
    N, K, D = C.shape
    L = max(sg.norms_chains(N, D))
    bound = np.empty(len(flat))
    worst = 0.0
    A = np.abs(C).astype(np.float64)
    for a in range(0, len(flat), 16384):
        f = flat[a:a + 16384]
        ref = (_decode64(C, f) ** 2).sum(1)
        mag = np.zeros((len(f), D))
        for n in range(N):
            mag += A[n][f[:, n]]
        bound[a:a + 16384] = 4 * L * EPS * (mag ** 2).sum(1)
        err = np.abs(t[a:a + 16384].astype(np.float64) - ref)
        bad = err > bound[a:a + 16384]
        assert not bad.any(), f"{int(bad.sum())} norms out of bound in rows {a}.."
        worst = max(worst, float((err / np.maximum(bound[a:a + 16384], 1e-300)).max()))
    _note(case.name, "norms", worst)
    return bound


def run_case(case):
    q = _quantizer(case)
    kept, flat = _store(case, q)
    xq, rows = _queries(case, q, kept)
    qh = xq.float().cpu().numpy()                      # fp16 queries widen exactly
    C = _centers(q)
    N, K, D, Q, B, k = case.N, case.K, case.D, case.Q, case.B, case.k

    tables = q.search_tables(xq)
    norms = q.code_norms(kept)
    assert tables.dtype == torch.float32 and tuple(tables.shape) == (Q, N, K)
    assert norms.dtype == torch.float32 and tuple(norms.shape) == (B,)
    T, t = tables.cpu().numpy(), norms.cpu().numpy()
    tb = _check_tables(case, qh, C, T)
    nb = _check_norms(case, C, flat, t)

    flat_d = torch.from_numpy(flat).cuda()
    s1, i1 = q._search_scan(tables, flat_d, norms, k)
    dist, idx = q.search(xq, kept, k=k, norms=norms)
    dist0, idx0 = q.search(xq, kept, k=k)             # norms formed inside
    assert s1.dtype == torch.float32 and i1.dtype == torch.int64 and tuple(s1.shape) == tuple(i1.shape) == (Q, k)
    assert dist.dtype == torch.float32 and idx.dtype == torch.int64 and tuple(dist.shape) == tuple(idx.shape) == (Q, k)
    want_s, want_i = sg.restate(T, t, flat, k)
    got_s, got_i = s1.cpu().numpy(), i1.cpu().numpy()
    assert np.array_equal(got_i, want_i), f"indexes differ in rows {np.flatnonzero((got_i != want_i).any(1))[:8]}"
    assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), "scores differ from rule 3"
    assert np.array_equal(idx.cpu().numpy(), want_i) and np.array_equal(idx0.cpu().numpy(), want_i)
    assert torch.equal(dist, dist0)
    if case.short:
        assert (want_i[:, B:] == -1).all() and np.isinf(got_s[:, B:]).all() and np.isinf(dist.cpu().numpy()[:, B:]).all()

    # distances of the returned positions against float64
    d = dist.cpu().numpy().astype(np.float64)
    assert (d >= 0).all()
    worst = 0.0
    for qi in range(Q):
        m = min(k, B)
        pos = want_i[qi, :m]
        ref = ((qh[qi].astype(np.float64)[None, :] - _decode64(C, flat[pos])) ** 2).sum(1)
        bound = nb[pos] + D * EPS * float((qh[qi].astype(np.float64) ** 2).sum())
        for n in range(N):
            bound = bound + tb[qi, n][flat[pos, n]]
        err = np.abs(d[qi, :m] - ref)
        assert (err <= bound).all(), (qi, err.max(), bound.min())
        worst = max(worst, float((err / bound).max()))
    _note(case.name, "distances", worst)
    if rows is not None:
        # every query is a stored vector's decode: its own code (at its lowest position) comes first, at distance ~0 (checked
        # against float64 above; the clamp keeps a negative rounding residue out)
        same = [(flat[want_i[qi, 0]] == flat[rows[qi]]).all() for qi in range(Q)]
        assert all(same)

    # determinism: a second call gives the same bits
    s2, i2 = q._search_scan(tables, flat_d, norms, k)
    dist2, idx2 = q.search(xq, kept, k=k, norms=norms)
    assert torch.equal(q.search_tables(xq), tables) and torch.equal(q.code_norms(kept), norms)
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(i1, i2)
    assert torch.equal(dist.view(torch.int32), dist2.view(torch.int32)) and torch.equal(idx, idx2)


@pytest.mark.parametrize("case", sg.CASES, ids=lambda c: c.name)
def test_search_case(case):
    run_case(case)


def test_composed_encode_then_search():
    """65,536 frames encoded, 64 of them searched for: each query's own position comes first or ties the first score"""
    from quantization_amd import synthetic as gen
    case = sg.Case("composed", 8, 256, 512, 64, 65536, 10)
    q = _quantizer(case)
    x = torch.from_numpy(gen.make_gaussian(8, case.B, case.D)).cuda()
    codes = q.encode(x)
    norms = q.code_norms(codes)
    rows = torch.arange(0, case.B, case.B // case.Q, device="cuda")[:case.Q] + 5
    tables = q.search_tables(x[rows])
    scores, idx = q._search_scan(tables, codes, norms, case.k)
    dist, idx_s = q.search(x[rows], codes, k=case.k, norms=norms)
    assert torch.equal(idx, idx_s)
    own = (tables.reshape(case.Q, 8, 256).gather(2, codes[rows].long().unsqueeze(2)).squeeze(2))
    acc = own[:, 0]
    for n in range(1, 8):
        acc = acc + own[:, n]
    own_score = acc + norms[rows]
    first = (idx[:, 0] == rows) | (scores[:, 0] == own_score)
    assert bool(first.all()), (idx[:, 0].tolist(), rows.tolist())
    # the distance of the own position is the encode's reconstruction error
    err = ((x[rows] - q.decode(codes[rows])) ** 2).sum(1)
    assert torch.allclose(dist[:, 0], err, rtol=1e-3, atol=1e-3)


def test_search_interface():
    from quantization_amd._lib import McqError
    case = sg.Case("iface", 8, 256, 24, 3, 100, 10)
    q = _quantizer(case)
    x = torch.randn(2, 3, 24, device="cuda")
    codes = torch.randint(0, 256, (100, 8), dtype=torch.uint8, device="cuda")
    d, i = q.search(x, codes, k=5)
    assert tuple(d.shape) == tuple(i.shape) == (2, 3, 5) and not d.requires_grad
    with pytest.raises(McqError):
        q.search(x.cpu(), codes)
    with pytest.raises(McqError):
        q.search(x, codes.cpu())
    with pytest.raises(McqError):
        q.code_norms(codes.cpu())
    with pytest.raises(McqError):
        q.search_tables(x.cpu())
    with pytest.raises(McqError):
        q.search(x, codes, k=65)
    # an empty store and no queries: rule 4's fill
    d, i = q.search(x, codes[:0], k=4)
    assert bool(torch.isinf(d).all()) and bool((i == -1).all())
    d, i = q.search(x[:0], codes, k=4)
    assert tuple(d.shape) == (0, 3, 4)
    # a non-finite query neither faults nor hangs (its row is unspecified)
    xb = x.clone().reshape(6, 24)
    xb[1, 3] = float("nan")
    xb[2, 0] = float("inf")
    d, i = q.search(xb, codes, k=4)
    torch.cuda.synchronize()
    d2, i2 = q.search(x.reshape(6, 24), codes, k=4)
    keep = [0, 3, 4, 5]
    assert torch.equal(i[keep], i2[keep])
