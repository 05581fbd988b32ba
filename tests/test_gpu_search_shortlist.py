"""The search over a shortlist on the GPU (mcq_search_shortlist / mcq_search_shortlist_u16 through ctypes,
Quantizer.search_shortlist; include/mcq_shortlist.h rules 36-39), BIT FOR BIT -- scores as uint32 views, and positions --
against the numpy restatement of tests/search_shortlist_grid.py and against the entries that already ship.  No tolerance appears
before the last test, whose bound is the derived one of tests/test_gpu_search.py.  Stores have at most 4,099 vectors.

  cases         the table of tests/search_shortlist_grid.py: every chunk width and one, two and eight chunks a row, the
                two-byte shapes, S = 0 .. 1,000 on both sides of a step and of a round of four waves, k = 1 .. 1,024 on both
                sides of S, Q = 1, 5, 70 and Qs whose plan has a single part, three metrics; shortlists with -1 in the middle
                and at the end, a row of -1 only, the values B, 2**40, -7 and INT64_MIN, duplicates; row_of as a permutation
                with entries outside [0, B) and Bs != B; biases with zeros, negatives and a -0.0.  The workspace and both
                outputs are pre-filled with 0xA5 bytes.
  contents      a row and its reversal; junk replaced by -1; row_of = arange and row_of = None; a bias of -0.0 and no bias; a
                bias that changes the result where the restatement says so
  shipped       row q against _search_wide_scan under the mask of its shortlist; arange(B) against the whole store; the
                positions of the probed lists with the per-entry bias against search over the lists with probe_bias; the
                two-byte entry on codes.to(int16) against the one-byte entry
  orders        S = 3,000 in one part at k = 1,024 and 100, zero tables, scores driven by w
  selection     every cell of launch_short once
  public call   leading dimensions, int32 shortlists, a shortlist straight from search_wide, the errors
  end to end    the residual recipe of tests/test_gpu_search_residual.py with a second, finer quantizer"""
import numpy as np
import pytest
import torch

import search_grid as sg
import search_shortlist_grid as hg
import search_wide_grid as wg

pytestmark = pytest.mark.gpu
INT64_MIN = np.iinfo(np.int64).min


def _lib():
    from quantization_amd import _lib
    return _lib


def _dev(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:                                  # the int16 store of pack_codes: the same bits
        a = a.view(np.int16)
    return torch.from_numpy(a).cuda()


def _abi(T_d, codes_d, w_d, short_d, k, metric, row_of_d=None, bias_d=None):
    """the entry the dtype of codes_d names, with the workspace and both outputs pre-filled with 0xA5 bytes -> (scores,
    positions) on the device"""
    m = _lib()
    L = m.lib()
    (Q, N, K), B, S = T_d.shape, codes_d.shape[0], short_d.shape[1]
    need = L.mcq_search_shortlist_workspace_bytes(Q, S, N, K, k)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    scores = torch.full((Q, k), 0xA5, dtype=torch.uint8, device="cuda").repeat(1, 4).view(torch.float32)
    pos = torch.full((Q, k), 0xA5, dtype=torch.uint8, device="cuda").repeat(1, 8).view(torch.int64)
    assert scores.shape == pos.shape == (Q, k) and short_d.dtype == torch.int64 and short_d.is_contiguous()
    entry = L.mcq_search_shortlist_u16 if codes_d.dtype == torch.int16 else L.mcq_search_shortlist
    assert codes_d.dtype in (torch.int16, torch.uint8) and tuple(codes_d.shape) == (B, N) and codes_d.is_contiguous()
    rc = entry(T_d.data_ptr(), Q, codes_d.data_ptr(), None if metric == "ip" or w_d is None else w_d.data_ptr(), B, N, K, k,
               hg.CODE[metric], short_d.data_ptr(), S, None if row_of_d is None else row_of_d.data_ptr(),
               0 if row_of_d is None else row_of_d.numel(), None if bias_d is None else bias_d.data_ptr(), scores.data_ptr(),
               pos.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return scores, pos


def _same(got, want, what):
    gs, gi = got[0].cpu().numpy(), got[1].cpu().numpy()
    want_s, want_i = want
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gs.shape == gi.shape == want_i.shape, what
    assert np.array_equal(gi, want_i), f"{what}: positions differ from rule 38 in rows {np.flatnonzero((gi != want_i).any(1))[:8]}"
    assert np.array_equal(gs.view(np.uint32), want_s.view(np.uint32)), f"{what}: scores differ from rule 37"
    tail = want_i == -1
    assert (gi[tail] == -1).all() and np.isposinf(gs[tail]).all(), f"{what}: the tail is not (+inf, -1)"
    return int(tail.sum())


def _equal(a, b):
    return torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def _quant(N, K, D=24):
    """a Quantizer for the calls that need one only for its shape (_search_wide_scan, _search_scan: no state is read)"""
    from quantization_amd import Quantizer
    return Quantizer(D, K, N)


# ------------------------------------------------------------------ the case table
@pytest.mark.parametrize("x", hg.CASES, ids=lambda c: c.name)
def test_case(x):
    T, w, codes, short, row_of, bias = hg.make(x)
    want_s, want_i, _ = hg.restate(T, w, codes, short, x.k, x.metric, row_of, bias)
    T_d, w_d, codes_d, short_d, row_d, bias_d = (_dev(a) for a in (T, w, codes, short, row_of, bias))
    got = _abi(T_d, codes_d, w_d, short_d, x.k, x.metric, row_d, bias_d)
    tail = _same(got, (want_s, want_i), x.name)
    pos, _ = hg.rg.candidates(short, x.B, row_of)
    assert tail == int(np.maximum(x.k - (pos >= 0).sum(1), 0).sum()) if x.S else tail == x.Q * x.k
    assert _equal(got, _abi(T_d, codes_d, w_d, short_d, x.k, x.metric, row_d, bias_d)), "a second call differs"
    if x.S and x.short == "junk":                             # junk replaced by -1: the same bits
        clean = np.where(pos >= 0, short, -1)
        assert (clean != short).any() and _equal(got, _abi(T_d, codes_d, w_d, _dev(clean), x.k, x.metric, row_d, bias_d))
    if x.Q > 1 and x.S:                                       # a query alone: another number of parts, the same bits
        j = x.Q - 1
        alone = _abi(T_d[j:j + 1].contiguous(), codes_d, w_d, short_d[j:j + 1].contiguous(), x.k, x.metric, row_d,
                     None if bias_d is None else bias_d[j:j + 1].contiguous())
        assert _equal(alone, (got[0][j:j + 1], got[1][j:j + 1])), "a query alone differs from the same query among others"


# ------------------------------------------------------------------ the contents of a shortlist, row_of and the bias
def test_contents_row_of_and_bias():
    x = next(c for c in hg.CASES if c.name == "n8_k256_s257_k1024")
    T, w, codes, short, row_of, bias = hg.make(x)
    T_d, w_d, codes_d, short_d, row_d, bias_d = (_dev(a) for a in (T, w, codes, short, row_of, bias))
    assert {len(row_of), 2 ** 40, -7, INT64_MIN} <= set(short[0].tolist())
    for metric in hg.METRICS:
        for k in (10, 300):
            plain = _abi(T_d, codes_d, w_d, short_d, k, metric)
            _same(plain, hg.restate(T, w, codes, short, k, metric)[:2], (metric, k))
            assert _equal(plain, _abi(T_d, codes_d, w_d, short_d.flip(1).contiguous(), k, metric)), "a reversed row gives another result"
            ar = torch.arange(x.B, device="cuda")
            assert _equal(plain, _abi(T_d, codes_d, w_d, short_d, k, metric, ar)), "row_of = arange differs from row_of = None"
            neg = torch.full(short_d.shape, -0.0, device="cuda")
            assert _equal(plain, _abi(T_d, codes_d, w_d, short_d, k, metric, None, neg)), "a bias of -0.0 differs from no bias"
            biased = _abi(T_d, codes_d, w_d, short_d, k, metric, None, bias_d)
            want_b = hg.restate(T, w, codes, short, k, metric, None, bias)[:2]
            _same(biased, want_b, (metric, k, "bias"))
            want_p = hg.restate(T, w, codes, short, k, metric)[:2]
            assert not np.array_equal(want_b[0], want_p[0]) and not _equal(biased, plain)     # where the restatement says so
            mapped = _abi(T_d, codes_d, w_d, short_d, k, metric, row_d, bias_d)
            _same(mapped, hg.restate(T, w, codes, short, k, metric, row_of, bias)[:2], (metric, k, "row_of"))
    # a row of -1 only, -1 in the middle and at the end
    pad = short.copy()
    pad[1] = -1
    pad[:, 100] = -1
    pad[:, -30:] = -1
    got = _abi(T_d, codes_d, w_d, _dev(pad), 300, "l2")
    _same(got, hg.restate(T, w, codes, pad, 300, "l2")[:2], "pad")
    assert bool((got[1][1] == -1).all())


# ------------------------------------------------------------------ against the entries that ship
@pytest.mark.parametrize("NK", ((8, 256), (64, 256), (4, 16)), ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_against_the_masked_scan_and_the_whole_store(NK):
    N, K = NK
    B, Q = 4099, 9
    rs = np.random.RandomState(6)
    quant = _quant(N, K)
    T_d = _dev(rs.standard_normal((Q, N, K)).astype(np.float32))
    codes_d = _dev(rs.randint(0, K, size=(B, N)).astype(np.uint8))
    w_d = _dev((rs.rand(B) * 4).astype(np.float32))
    for metric in hg.METRICS:
        for k, S in ((10, 300), (300, 1000), (1024, 257)):
            short = np.stack([rs.permutation(B + 40)[:S] - 20 for _ in range(Q)]).astype(np.int64)     # distinct; some junk
            got = _abi(T_d, codes_d, w_d, _dev(short), k, metric)
            for q in range(Q):
                keep = np.zeros(B, dtype=bool)
                keep[short[q][(short[q] >= 0) & (short[q] < B)]] = True
                want = quant._search_wide_scan(T_d[q:q + 1].contiguous(), codes_d, w_d, k, metric=metric, mask=_dev(keep))
                assert _equal((got[0][q:q + 1], got[1][q:q + 1]), want), (metric, k, S, q)
        for k in (10, 1024):
            every = torch.arange(B, device="cuda").repeat(Q, 1).contiguous()
            assert _equal(_abi(T_d, codes_d, w_d, every, k, metric), quant._search_wide_scan(T_d, codes_d, w_d, k, metric=metric)), (metric, k)


def test_against_the_lists_with_a_probe_bias():
    import search_selection_grid as sel
    N, K, Q = 8, 256, 3
    rs = np.random.RandomState(7)
    off, probes = sel.lists_layout()
    off, probes = np.asarray(off, dtype=np.int64), np.asarray(probes, dtype=np.int32)
    B = int(off[-1]) + 13
    assert probes.shape[0] == Q and (probes == -1).any()
    quant = _quant(N, K)
    T_d = _dev(rs.standard_normal((Q, N, K)).astype(np.float32))
    codes_d = _dev(rs.randint(0, K, size=(B, N)).astype(np.uint8))
    w_d = _dev((rs.rand(B) * 4).astype(np.float32))
    pb = rs.standard_normal(probes.shape).astype(np.float32)
    rows, biases = [], []
    for q in range(Q):
        named = [(p, int(l)) for p, l in enumerate(probes[q]) if 0 <= l < len(off) - 1]
        rows.append(np.concatenate([np.arange(off[l], off[l + 1]) for _, l in named]))
        biases.append(np.concatenate([np.full(off[l + 1] - off[l], pb[q, p], dtype=np.float32) for p, l in named]))
    S = max(len(r) for r in rows)
    short = np.full((Q, S), -1, dtype=np.int64)
    bias = np.full((Q, S), np.nan, dtype=np.float32)          # (the bias of an entry that names no candidate does not matter)
    for q in range(Q):
        short[q, :len(rows[q])], bias[q, :len(rows[q])] = rows[q], biases[q]
    for metric in hg.METRICS:
        for k in (10, 300):
            want = quant._search_wide_scan(T_d, codes_d, w_d, k, metric=metric, lists=(_dev(off), _dev(probes)), bias=_dev(pb))
            assert _equal(_abi(T_d, codes_d, w_d, _dev(short), k, metric, None, _dev(bias)), want), (metric, k)


@pytest.mark.parametrize("NK", hg.CROSS, ids=lambda nk: f"{nk[0]}x{nk[1]}")
def test_two_byte_entry_against_the_one_byte_entry(NK):
    N, K = NK
    x = hg.Case("cross", N, K, 5, 300, 65, short="junk", row_of="perm_bad", bias="random")
    T, w, codes, short, row_of, bias = hg.make(x)
    T_d, w_d, codes_d, short_d, row_d, bias_d = (_dev(a) for a in (T, w, codes, short, row_of, bias))
    for metric in hg.METRICS:
        one = _abi(T_d, codes_d, w_d, short_d, x.k, metric, row_d, bias_d)
        two = _abi(T_d, codes_d.to(torch.int16), w_d, short_d, x.k, metric, row_d, bias_d)
        assert _equal(one, two), metric
        _same(one, hg.restate(T, w, codes, short, x.k, metric, row_of, bias)[:2], metric)


# ------------------------------------------------------------------ hand-made orders
ORDER_Q, ORDER_S, ORDER_B = 600, 3000, 3200
ORDERS = ("descending", "ascending", "all_equal", "zeros", "inf", "nan")


@pytest.mark.parametrize("order", ORDERS)
def test_orders_in_one_part(order):
    """one codebook of 16 entries, every table entry -0.0 and the metric L2: the score of a row is the bits of its w"""
    N, K = wg.ORDER_N, wg.ORDER_K
    assert hg.short_plan(ORDER_Q, ORDER_S, N, K, 1024).parts == 1
    rs = np.random.RandomState(8)
    w = wg.order_w(order, ORDER_B)
    short = np.arange(ORDER_S, dtype=np.int64) if order in ("descending", "ascending") else rs.permutation(ORDER_B)[:ORDER_S].astype(np.int64)
    if order == "descending":
        assert (np.diff(w[short]) < 0).all()                  # every candidate beats the bound when it arrives
    T = np.full((1, N, K), -0.0, dtype=np.float32)
    codes = rs.randint(0, K, size=(ORDER_B, N)).astype(np.uint8)
    want = {k: hg.restate(T, w, codes, short[None, :], k, "l2")[:2] for k in (1024, 100)}
    T_d, codes_d, w_d = _dev(np.repeat(T, ORDER_Q, 0)), _dev(codes), _dev(w)
    short_d = _dev(np.repeat(short[None, :], ORDER_Q, 0))
    got = {k: _abi(T_d, codes_d, w_d, short_d, k, "l2") for k in (1024, 100)}
    for k in (1024, 100):
        _same(got[k], (np.repeat(want[k][0], ORDER_Q, 0), np.repeat(want[k][1], ORDER_Q, 0)), f"{order} k={k}")
    assert _equal((got[1024][0][:, :100], got[1024][1][:, :100]), got[100]), "k = 100 is not the prefix of k = 1,024"
    if order in ("all_equal", "zeros"):                       # position decides, and a zero keeps its bits
        assert np.array_equal(want[1024][1][0], np.sort(short)[:1024])
        assert np.array_equal(want[1024][0][0].view(np.uint32), w[np.sort(short)[:1024]].view(np.uint32))
    if order == "inf":
        assert np.isposinf(want[1024][0][0][want[1024][1][0] >= 0]).any() and np.isneginf(want[1024][0][0][0])
    if order == "nan":
        assert np.isnan(w[short]).sum() > 1000 and not np.isnan(want[1024][0]).any()


# ------------------------------------------------------------------ selection
def test_every_cell_of_the_launcher_runs_once():
    rs = np.random.RandomState(9)
    B, Q, S, k = 70, 3, 90, 10
    short = rs.randint(-2, B + 2, size=(Q, S)).astype(np.int64)
    cells = 0
    for two in (False, True):
        for N in hg.NS:
            K = 16 if N == 64 or not two else 256
            T = rs.standard_normal((Q, N, K)).astype(np.float32)
            codes = rs.randint(0, K, size=(B, N)).astype(np.uint16 if two else np.uint8)
            w = (rs.rand(B) * 4).astype(np.float32)
            T_d, codes_d, w_d, short_d = _dev(T), _dev(codes), _dev(w), _dev(short)
            for metric in hg.METRICS:
                _same(_abi(T_d, codes_d, w_d, short_d, k, metric), hg.restate(T, w, codes, short, k, metric)[:2], (two, N, metric))
                cells += 1
    assert cells == 2 * len(hg.NS) * 3 == 42


# ------------------------------------------------------------------ the public call
def test_public_call():
    import test_gpu_search as base
    m = _lib()
    rs = np.random.RandomState(10)
    case = sg.Case("shortlist_public", 4, 256, 24, 6, 300, 10)
    quant = base._quantizer(case)
    B, D = case.B, case.D
    xs = torch.from_numpy(rs.standard_normal((B, D)).astype(np.float32)).cuda()
    with torch.no_grad():
        codes = quant.encode(xs, refine_indexes_iters=2)
    xq = (xs[:6] + 0.01).reshape(2, 3, D)
    norms, rnorms = quant.code_norms(codes), quant.code_rnorms(codes)
    short = rs.randint(-1, B, size=(2, 3, 50)).astype(np.int32)
    short[1, 2] = -1                                          # a row without a candidate
    row_of = rs.permutation(B).astype(np.int64)
    s_d, r_d = torch.from_numpy(short).cuda(), torch.from_numpy(row_of).cuda()
    T = quant.search_tables(xq)
    flat = codes.cpu().numpy()
    qq = (xq.reshape(6, D) ** 2).sum(dim=1, keepdim=True)
    from quantization_amd.search import _reported
    for metric in hg.METRICS:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        for ro, ro_d in ((None, None), (row_of, r_d)):
            val, idx = quant.search_shortlist(xq, codes, s_d, 60, norms=norms, metric=metric, rnorms=rnorms, row_of=ro_d)
            assert tuple(val.shape) == tuple(idx.shape) == (2, 3, 60) and val.dtype == torch.float32 and idx.dtype == torch.int64
            ws, wi, _ = hg.restate(T.cpu().numpy(), None if w is None else w.cpu().numpy(), flat, short.reshape(6, 50), 60, metric, ro)
            assert np.array_equal(idx.cpu().numpy().reshape(6, 60), wi)
            want_v = _reported(torch.from_numpy(ws).cuda(), metric, qq)
            assert torch.equal(val.reshape(6, 60).view(torch.int32), want_v.view(torch.int32))
            assert (wi[5] == -1).all() and (wi[:5, 50:] == -1).all()
            tail = val.reshape(6, 60)[5]
            assert bool(torch.isposinf(tail).all() if metric == "l2" else torch.isneginf(tail).all())
            made = quant.search_shortlist(xq, codes, s_d, 60, metric=metric, row_of=ro_d)      # norms / rnorms made inside
            assert torch.equal(made[1], idx) and torch.equal(made[0].view(torch.int32), val.view(torch.int32))
        # a shortlist straight from search_wide, k its width: search_wide's own values and indexes
        wv, wi_ = quant.search_wide(xq, codes, 100, norms=norms, metric=metric, rnorms=rnorms)
        sv, si = quant.search_shortlist(xq, codes, wi_, 100, norms=norms, metric=metric, rnorms=rnorms)
        assert torch.equal(si, wi_) and torch.equal(sv.view(torch.int32), wv.view(torch.int32)), metric
    bias = torch.from_numpy(rs.standard_normal((2, 3, 50)).astype(np.float32)).cuda()
    val, idx = quant.search_shortlist(xq, codes, s_d, 10, norms=norms, bias=bias)
    ws, wi, _ = hg.restate(T.cpu().numpy(), norms.cpu().numpy(), flat, short.reshape(6, 50), 10, "l2", None, bias.cpu().numpy().reshape(6, 50))
    assert np.array_equal(idx.cpu().numpy().reshape(6, 10), wi)
    with pytest.raises(m.McqError):
        quant.search_shortlist(xq.cpu(), codes, s_d, 10)
    with pytest.raises(ValueError):
        quant.search_shortlist(xq, codes, s_d, 1025)
    with pytest.raises(ValueError):
        quant.search_shortlist(xq, codes, s_d, 10, metric="dot")
    with pytest.raises(ValueError):
        quant.search_shortlist(xq, codes, s_d[:1], 10)
    # two-byte codes: the int16 store of pack_codes, int64 digits narrowed, uint8 refused
    case16 = sg.Case("shortlist_public16", 4, 1024, 24, 6, 300, 10)
    q16 = base._quantizer(case16)
    digits = torch.from_numpy(rs.randint(0, 1024, size=(B, 4))).cuda()
    store = q16.pack_codes(digits)
    a = q16.search_shortlist(xq, store, s_d, 20)
    b = q16.search_shortlist(xq, digits, s_d, 20)
    assert store.dtype == torch.int16 and torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
    every = torch.arange(B, device="cuda").repeat(2, 3, 1)
    c, d = q16.search_shortlist(xq, store, every, 20), q16.search(xq, store, 20)
    assert torch.equal(c[1], d[1]) and torch.equal(c[0].view(torch.int32), d[0].view(torch.int32))
    with pytest.raises(ValueError, match="pack_codes"):
        q16.search_shortlist(xq, digits.to(torch.uint8), s_d, 20)


# ------------------------------------------------------------------ end to end
def test_end_to_end_two_stage_quantisation():
    """The coarse stage is the residual store of tests/test_gpu_search_residual.py (4 x 256 residual codes in 16 lists):
    search_lists_wide(k = 300).  The fine stage is a second synthetic Quantizer with 16 codebooks over the raw vectors, its
    codes kept in the ORIGINAL order: search_shortlist(k = 10, row_of = order).  Every reported value lies within the derived
    fp32 bound of the float64 distance to decode(fine code) at its index -- the bound of tests/test_gpu_search.py: the N table
    bounds, the norm bound and D 2^-24 |q|^2 -- and nothing is looser.  Then shortlists that contain the fine quantizer's
    exhaustive top ten (its union with random other positions): the result equals fine.search(k = 10) bit for bit, every row."""
    import test_gpu_search as base
    import test_gpu_search_residual as res
    from quantization_amd import build_lists
    quant, xq_d, codes, off, probes, bias, norms, rnorms, exact, bound, cand = res._setup()
    rs = np.random.RandomState(21)                            # the raw vectors of that recipe, drawn again
    cen = (rs.standard_normal((res.NL, res.D)) * 2.0).astype(np.float32)
    member = rs.randint(0, res.NL, size=res.B)
    x = (cen[member] + 0.5 * rs.standard_normal((res.B, res.D))).astype(np.float32)
    xq = (cen[rs.randint(0, res.NL, size=res.Q)] + 0.5 * rs.standard_normal((res.Q, res.D))).astype(np.float32)
    assert np.array_equal(xq, xq_d.cpu().numpy())
    assign = ((x.astype(np.float64)[:, None, :] - cen.astype(np.float64)[None]) ** 2).sum(2).argmin(1)
    order, off2 = build_lists(torch.from_numpy(assign).cuda(), res.NL)
    assert torch.equal(off2, off)
    fcase = sg.Case("two_stage_fine_16x256_d24", 16, 256, res.D, res.Q, res.B, 10)
    fine = base._quantizer(fcase)
    with torch.no_grad():
        fcodes = fine.encode(torch.from_numpy(x).cuda(), refine_indexes_iters=2)     # original order
    fnorms = fine.code_norms(fcodes)
    _, short = quant.search_lists_wide(xq_d, codes, off, probes, 300, norms=norms, probe_bias=bias)
    val, idx = fine.search_shortlist(xq_d, fcodes, short, 10, norms=fnorms, row_of=order)
    # bit for bit against the restatement, from the tables and norms the GPU returned
    T, t, flat = fine.search_tables(xq_d).cpu().numpy(), fnorms.cpu().numpy(), fcodes.cpu().numpy()
    short_h, order_h = short.cpu().numpy(), order.cpu().numpy()
    want_s, want_i, _ = hg.restate(T, t, flat, short_h, 10, "l2", order_h)
    assert np.array_equal(idx.cpu().numpy(), want_i) and bool((idx >= 0).all())
    from quantization_amd.search import _reported
    qq = (xq_d * xq_d).sum(dim=1, keepdim=True)
    assert torch.equal(val.view(torch.int32), _reported(torch.from_numpy(want_s).cuda(), "l2", qq).view(torch.int32))
    # within the derived bound of float64
    C = base._centers(fine)
    tb = base._check_tables(fcase, xq, C, T)
    nb = base._check_norms(fcase, C, flat, t)
    d, idx_h = val.cpu().numpy().astype(np.float64), idx.cpu().numpy()
    worst = 0.0
    for j in range(res.Q):
        rows = order_h[idx_h[j]]
        ref = ((xq[j].astype(np.float64)[None, :] - base._decode64(C, flat[rows])) ** 2).sum(1)
        bd = nb[rows] + res.D * base.EPS * float((xq[j].astype(np.float64) ** 2).sum())
        for n in range(16):
            bd = bd + tb[j, n][flat[rows, n]]
        err = np.abs(d[j] - ref)
        assert (err <= bd).all(), (j, err.max(), bd.min())
        worst = max(worst, float((err / bd).max()))
    print(f"[shortlist] two stages: largest error / bound of the reported distances = {worst:.4f}")
    # shortlists that contain the fine quantizer's exhaustive top ten
    for metric in hg.METRICS:
        top_v, top_i = fine.search(xq_d, fcodes, k=10, metric=metric, norms=fnorms)
        rows = []
        for j in range(res.Q):
            row = np.unique(np.concatenate([top_i[j].cpu().numpy(), rs.permutation(res.B)[:290]]))
            rows.append(rs.permutation(np.concatenate([row, np.full(300 - len(row), -1, dtype=np.int64)])))
        union = torch.from_numpy(np.stack(rows).astype(np.int64)).cuda()
        v, i = fine.search_shortlist(xq_d, fcodes, union, 10, norms=fnorms, metric=metric)
        assert torch.equal(i, top_i) and torch.equal(v.view(torch.int32), top_v.view(torch.int32)), metric
