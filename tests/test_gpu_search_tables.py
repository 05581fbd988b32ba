"""The first stage of every search entry on the GPU -- the per-query tables (mcq_search_tables, rule 1 of include/mcq.h), the
per-candidate norms (mcq_code_norms, rule 2) and their reciprocal roots (mcq_code_rnorms, mcq_rnorms_from_norms, rule 6) -- BIT
FOR BIT against the numpy restatement of tests/search_tables_grid.py, formed from the queries, the codes and the padded fp32
rows read out of `prepared`, never from an array the device computed.  Every comparison is one of uint32 views with no
tolerance; the one exception: where the restatement is NaN the device value must be a NaN, sign and payload free.

  tables        the case table of tests/search_tables_grid.py through the C entry, the output pre-filled with 0xA5 bytes and
                followed by a guard; a second call; Quantizer.search_tables with leading dimensions and a float64 input
  views         fp32 and fp16 queries one element into their storage
  launch        a query alone, first, last of a tile and among 33; the rows beside a NaN, +-inf or 3e38 row of their tile.  The
                non-finite row itself (rule 5 leaves it unspecified) is compared as well, and what is found is printed
  edge queries  zero, -0.0, fp32 and fp16 subnormals, +-65504, products that overflow, inf * 0, exact cancellation
  edge centers  a hand-made state (2 x 16 x 32, centers_scale 0 so that `prepared` holds the rows as given): rows of zeros, of
                +2^k, of -2^k, of +-2^k alternating, of fp32 subnormals, of 2^-126, of 2^-70 (a subnormal norm), one element of
                2^100 (a norm of +inf), and a pair C[0][5] = -C[1][1].  prepare accepts all of them; non-finite CENTERS are left
                out: mcq_prepare is specified for finite parameters only
  norms         the case table: code_norms, code_rnorms, rnorms_from_norms and the three C entries with pre-fill and guard;
                packed 16-entry codes; B = 0; t = +0 -> r = +0 and t = +inf -> r = +0 on the hand-made state
  end to end    search under the three metrics at D = 40 and D = 1,000 returns the indexes of rules 3 and 4 restated from the
                RESTATED tables and norms"""
import numpy as np
import pytest
import torch

import search_grid as sg
import search_metric_grid as mg
import search_tables_grid as tg
import test_gpu_search as base
from test_gpu_code_norms_based import _padded_centers

pytestmark = pytest.mark.gpu

GUARD = 4096                                            # bytes of 0xA5 that must survive behind every output
_STATES = {}


def _lib():
    from quantization_amd import _lib
    return _lib


def _quantizer(N, K, D):
    """(quantizer on the device in its decode-only state, its padded centers (N, K, Dp)), one per shape"""
    key = (N, K, D)
    if key not in _STATES:
        q = base._quantizer(sg.Case("tables_n%d_k%d_d%d" % key, N, K, D, 1, 1, 1))
        Cp = _padded_centers(q)
        assert q._prep.flavour == "decode" and Cp.shape == (N, K, sg.padded(D)) and not Cp[:, :, D:].any()
        if len(_STATES) >= 6:
            _STATES.clear()
        _STATES[key] = (q, Cp)
    return _STATES[key]


HAND = (2, 16, 32)


def _hand_centers():
    """the hand-made centers (N, K, D) float32"""
    N, K, D = HAND
    rs = np.random.RandomState(9)
    C = rs.standard_normal((N, K, D)).astype(np.float32)
    d = np.arange(D)
    C[0, 0] = 0.0
    C[0, 1] = 2.0 ** (d % 5)                                         # every product with a -0.0 or a +0.0 query: that zero
    C[0, 2] = -(2.0 ** (d % 7 - 3))                                  # ... and the opposite one
    C[0, 3] = (d + 1) * 2.0 ** -149                                  # fp32 subnormals
    C[0, 4] = np.where(d % 2 == 0, 1.0, -1.0) * 2.0 ** ((d // 2) % 3)   # a query of ones: the partial sums return to 0 every 2nd term
    C[0, 6] = 0.25
    C[0, 6, 3] = 2.0 ** 100                                          # its square overflows
    C[0, 7] = -(d + 1) * 2.0 ** -149
    C[0, 8] = 2.0 ** -126                                            # the smallest normal: every square underflows to +0
    C[0, 9] = 2.0 ** -70                                             # squares of 2^-140: a SUBNORMAL norm, whose root is taken
    C[1, 0] = 0.0
    C[1, 1] = -C[0, 5]                                               # an exact zero reconstruction with C[0][5]
    C[1, 2] = 0.0
    C[1, 2, ::3] = -0.0
    return C


def _hand_made():
    """the state of hand-made centers: (quantizer, Cp as `prepared` holds it, the centers as given)"""
    from quantization_amd import Quantizer
    N, K, D = HAND
    C = _hand_centers()
    key = "hand"
    if key not in _STATES:
        q = Quantizer(D, K, N)
        st = q.state_dict()
        st["centers"] = torch.from_numpy(C)
        st["centers_scale"] = torch.zeros_like(st["centers_scale"])  # exp(0) = 1: the rows reach `prepared` as they are
        st["logits_scale"] = torch.zeros_like(st["logits_scale"])
        st["to_logits.weight"] = torch.zeros_like(st["to_logits.weight"])
        st["to_logits.bias"] = torch.zeros_like(st["to_logits.bias"])
        q.load_state_dict(st)
        q = q.to("cuda:0").requires_grad_(False)
        Cp = _padded_centers(q)
        _STATES[key] = (q, Cp)
    q, Cp = _STATES[key]
    return q, Cp, C


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    """bit for bit; where the restatement is NaN, any NaN -> the number of NaN entries"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), f"{what}: {int((~np.isnan(got[nan])).sum())} entries are numbers where the rule gives NaN"
    bad = (_u32(got) != _u32(want)) & ~nan
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} entries differ, first at {tuple(np.argwhere(bad)[0])}: "
                           f"{got[bad][0]!r} ({_u32(got)[bad][0]:#010x}) against {want[bad][0]!r} ({_u32(want)[bad][0]:#010x})")
    return int(nan.sum())


def _filled(count):
    """`count` floats and the guard behind them, all 0xA5 bytes"""
    return torch.full((count * 4 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")


def _taken(buf, count, what):
    torch.cuda.synchronize()
    assert bool((buf[count * 4:] == 0xA5).all()), f"{what}: bytes past the output were written"
    return buf[:count * 4].view(torch.float32)


def _dev(a, view=False):
    """numpy -> device tensor; view: one element into its storage (the base pointer is aligned to the element alone)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not view:
        return t.cuda()
    store = torch.empty(t.numel() + 1, dtype=t.dtype, device="cuda")
    out = store[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 != 0 and out.is_contiguous()
    return out


def _abi_tables(q, xq_d):
    """mcq_search_tables on device queries (Q, D) fp32 or fp16 -> float32 (Q, N * K) device tensor"""
    m = _lib()
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    Q = xq_d.shape[0]
    assert xq_d.is_contiguous() and tuple(xq_d.shape) == (Q, D) and xq_d.dtype in (torch.float32, torch.float16)
    blob = q._prepared(any_flavour=True)
    buf = _filled(Q * N * K)
    rc = m.lib().mcq_search_tables(xq_d.data_ptr(), int(xq_d.dtype == torch.float16), Q, blob.data_ptr(), N, K, D, buf.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return _taken(buf, Q * N * K, "mcq_search_tables").reshape(Q, N * K)


def _abi_norms(q, entry, codes_d):
    """mcq_code_norms / mcq_code_rnorms on device codes (B, N) uint8 -> float32 (B,) device tensor"""
    m = _lib()
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    B = codes_d.shape[0]
    assert codes_d.is_contiguous() and codes_d.dtype == torch.uint8 and (B == 0 or codes_d.shape[1] == N)
    blob = q._prepared(any_flavour=True)
    buf = _filled(B)
    rc = getattr(m.lib(), entry)(codes_d.data_ptr(), B, blob.data_ptr(), N, K, D, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return _taken(buf, B, entry)


def _abi_rnorms_from(norms_d):
    m = _lib()
    B = norms_d.numel()
    buf = _filled(B)
    rc = m.lib().mcq_rnorms_from_norms(norms_d.data_ptr(), B, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return _taken(buf, B, "mcq_rnorms_from_norms")


def _equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _tables_of(q, Cp, x, what, view=False):
    """the device's tables of numpy queries x, checked against the restatement -> (device tensor (Q, NK), NaN entries)"""
    got = _abi_tables(q, _dev(x, view))
    return got, _same(got.cpu().numpy(), tg.restate_tables(x, Cp), what)


# ------------------------------------------------------------------ tables: the case table
@pytest.mark.parametrize("x", tg.TAB_CASES, ids=lambda x: x.name)
def test_tables_case(x):
    q, Cp = _quantizer(x.N, x.K, x.D)
    xq = tg.queries(x)
    xq_d = _dev(xq)
    got = _abi_tables(q, xq_d)
    assert _same(got.cpu().numpy(), tg.restate_tables(xq, Cp), x.name) == 0
    assert _equal(got, _abi_tables(q, xq_d)), "a second call differs"
    # the public call: the same bytes, with leading dimensions, and from a float64 input what .float() gives
    pub = q.search_tables(xq_d)
    assert pub.dtype == torch.float32 and tuple(pub.shape) == (x.Q, x.N, x.K) and _equal(pub.reshape(x.Q, -1), got)
    if x.Q % 3 == 0:
        lead = q.search_tables(xq_d.reshape(3, x.Q // 3, x.D))
        assert tuple(lead.shape) == (x.Q, x.N, x.K) and _equal(lead, pub)
    wide = xq_d.double()
    assert _equal(q.search_tables(wide), q.search_tables(wide.float()))
    if not x.fp16:
        assert _equal(q.search_tables(wide), pub)


def test_public_call_takes_leading_dimensions():
    x = next(c for c in tg.TAB_CASES if c.name == "d40_8x256_q33_h")
    q, Cp = _quantizer(x.N, x.K, x.D)
    xq = tg.queries(x)
    want = tg.restate_tables(xq, Cp).reshape(x.Q, x.N, x.K)
    for shape in ((33, 40), (3, 11, 40), (1, 33, 1, 40)):
        T = q.search_tables(_dev(xq).reshape(shape))
        assert tuple(T.shape) == (33, x.N, x.K)
        _same(T.cpu().numpy(), want, f"leading dimensions {shape[:-1]}")
    f64 = q.search_tables(_dev(xq).double().reshape(3, 11, 40))
    _same(f64.cpu().numpy(), want, "float64 queries")                 # (fp16 values widen exactly, to float64 and back to float32)


# ------------------------------------------------------------------ views
@pytest.mark.parametrize("name", ("d33_8x256_q17", "d260_8x256_q17_h", "d17_2x16_q5_h", "d31_1x16_q15"))
def test_queries_one_element_into_their_storage(name):
    x = next(c for c in tg.TAB_CASES if c.name == name)
    q, Cp = _quantizer(x.N, x.K, x.D)
    xq = tg.queries(x)
    off, _ = _tables_of(q, Cp, xq, name + " (view)", view=True)
    assert _equal(off, _abi_tables(q, _dev(xq)))
    pub = q.search_tables(_dev(xq, view=True))                        # (contiguous already: the public call hands the view on)
    assert _equal(pub.reshape(x.Q, -1), off)


# ------------------------------------------------------------------ independence of the launch
@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
def test_a_row_does_not_depend_on_its_batch(half):
    N, K, D = 2, 64, 40
    q, Cp = _quantizer(N, K, D)
    x = np.random.RandomState(21).standard_normal((33, D)).astype(np.float16 if half else np.float32)
    v = x[7:8]
    want = tg.restate_tables(v, Cp)
    for what, batch, at in (("alone", v, 0), ("first", np.concatenate([v, x[:15]]), 0), ("last of a tile", np.concatenate([x[:15], v]), 15),
                            ("among 33", np.concatenate([x[:32], v]), 32), ("first of the second tile", np.concatenate([x[:16], v]), 16)):
        got, _ = _tables_of(q, Cp, batch, what)
        assert np.array_equal(_u32(got.cpu().numpy()[at]), _u32(want[0])), what


@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
def test_a_non_finite_query_stays_in_its_row(half):
    """rows of a tile of 16 beside a NaN, +inf, -inf or 3e38 (fp16: 65504) row are unchanged.  The row itself is unspecified
    under rule 5; it is compared with the restatement all the same, a NaN matching any NaN.  Found on the MI355X: it is the
    restatement's row, NaN for NaN, in every case."""
    N, K, D = 2, 64, 40
    q, Cp = _quantizer(N, K, D)
    dt = np.float16 if half else np.float32
    x = np.random.RandomState(22).standard_normal((16, D)).astype(dt)
    clean, n = _tables_of(q, Cp, x, "clean")
    assert n == 0
    clean = clean.cpu().numpy()
    for bad, row in ((np.nan, 0), (np.inf, 5), (-np.inf, 15), (65504.0 if half else 3e38, 6)):
        xb = x.copy()
        xb[row, 3] = bad
        xb[row, D - 1] = bad                                          # (the last feature: the half chunk)
        got, nans = _tables_of(q, Cp, xb, f"a row with {bad}")
        got = got.cpu().numpy()
        keep = np.arange(16) != row
        assert np.array_equal(_u32(got[keep]), _u32(clean[keep])), f"{bad}: another row of the tile changed"
        print(f"[tables] {'fp16' if half else 'fp32'} row with {bad}: {nans} NaN entries of {N * K}, "
              f"{int(np.isinf(got[row]).sum())} infinite, the row equals the restatement")


# ------------------------------------------------------------------ edge values as queries
def _edge_queries(D, half):
    """{name: (rows, D) array} of the edge queries of one dtype"""
    dt = np.float16 if half else np.float32
    rs = np.random.RandomState(23)
    g = rs.standard_normal((4, D)).astype(dt)
    out = {"zero": np.zeros((2, D), dtype=dt), "negative_zero": np.full((2, D), -0.0, dtype=dt)}
    mixed = g.copy()
    mixed[:, ::3] = -0.0
    mixed[1, 1::3] = 0.0
    out["some_negative_zeros"] = mixed
    tiny = (g.astype(np.float64) * 2.0 ** -20).astype(dt) if half else (g.astype(np.float64) * 2.0 ** -135).astype(dt)
    assert (np.abs(tiny[tiny != 0]) < (2.0 ** -14 if half else 2.0 ** -126)).all() and (tiny != 0).sum() > D
    out["subnormals"] = tiny                                          # (subnormal in the query's own format)
    big = np.where(rs.rand(4, D) < 0.5, 65504.0, -65504.0).astype(dt)
    out["largest_fp16"] = big
    ones = np.ones((2, D), dtype=dt)
    ones[1] = 3.0
    out["ones"] = ones                                                # exact cancellation against the +-2^k row of the hand-made state
    if not half:
        huge = g.copy()
        huge[:, :4] = np.float32(3e38) * np.sign(g[:, :4])
        out["products_overflow"] = huge                               # +-inf products; inf - inf = NaN where the signs differ
        out["fp16_subnormals_as_fp32"] = (g.astype(np.float64) * 2.0 ** -20).astype(np.float16).astype(np.float32)
    inf = g.copy()
    inf[0, 2] = np.inf
    inf[1, 5] = -np.inf
    inf[2, :] = np.inf
    out["infinite"] = inf                                             # inf * 0 = NaN against a zero center element
    return out


@pytest.mark.parametrize("half", (False, True), ids=("fp32", "fp16"))
def test_edge_queries(half):
    q, Cp, C = _hand_made()
    N, K, D = HAND
    assert np.array_equal(_u32(Cp), _u32(C)), "prepare changed a hand-made row (flushed a subnormal, lost a -0.0?)"
    found = {}
    for name, x in _edge_queries(D, half).items():
        got, nans = _tables_of(q, Cp, x, name)
        got = got.cpu().numpy().reshape(len(x), N, K)
        found[name] = nans
        if name in ("zero", "negative_zero"):
            # rule 1 starts at +0 and x + (-0) = x: every entry is -2 * (+0) = -0.0, whatever the signs of the products
            assert (_u32(got) == 0x80000000).all(), f"{name}: {int((_u32(got) != 0x80000000).sum())} entries are not -0.0"
        if name == "ones":
            assert (_u32(got[:, 0, 4]) == 0x80000000).all()           # every pair of terms cancels: +0, then -0.0
        if name == "infinite":
            assert np.isnan(got[:3, 0, 0]).all() and np.isneginf(got[2, 0, 1]) and np.isposinf(got[2, 0, 2])     # inf * 0 against the row
                                                                      # of zeros; -2 * (+-inf) against the rows of one sign
        if name == "subnormals":
            assert (got != 0).sum() > N * K                           # products of subnormal queries are kept, not flushed
    print(f"[tables] edge queries {'fp16' if half else 'fp32'}: NaN entries per set {found}")
    assert found["infinite"] > 0 and (half or found["products_overflow"] > 0)
    # the same queries against random centers at a dim whose last chunk is half a one
    N2, K2, D2 = 2, 16, 48
    q2, Cp2 = _quantizer(N2, K2, D2)
    for name, x in _edge_queries(D2, half).items():
        got, _ = _tables_of(q2, Cp2, x, name + " (random centers)")
        if name in ("zero", "negative_zero"):
            assert (_u32(got.cpu().numpy()) == 0x80000000).all()


def test_edge_centers():
    """gaussian, dyadic and tiny queries against the hand-made rows; the rows the docstring of this file lists all reach
    `prepared` unchanged (asserted in test_edge_queries)"""
    q, Cp, C = _hand_made()
    N, K, D = HAND
    rs = np.random.RandomState(24)
    for half in (False, True):
        dt = np.float16 if half else np.float32
        x = rs.standard_normal((17, D)).astype(dt)
        x[1] = 2.0 ** rs.randint(-10, 10, size=D)
        x[2] = x[2].astype(np.float64) * 2.0 ** -12                   # times the subnormal rows: products far below the smallest subnormal
        got, nans = _tables_of(q, Cp, x, "hand-made centers")
        assert nans == 0
        got = got.cpu().numpy().reshape(17, N, K)
        assert (_u32(got[:, 0, 0]) == 0x80000000).all() and (_u32(got[:, 1, 0]) == 0x80000000).all()      # rows of zeros
        assert np.array_equal(_u32(got[:, 0, 5]), _u32(-got[:, 1, 1]))                # C[1][1] = -C[0][5]: the chains mirror
        assert np.isfinite(got).all() and (got[:, 0, 3] != 0).any()                   # subnormal centers are not flushed


# ------------------------------------------------------------------ norms and reciprocal roots: the case table
@pytest.mark.parametrize("x", tg.NORM_CASES, ids=lambda x: x.name)
def test_norms_case(x):
    q, Cp = _quantizer(x.N, x.K, x.D)
    codes = tg.codes(x)
    codes_d = _dev(codes)
    want_t = tg.restate_norms(Cp, codes)
    want_r = tg.restate_rnorms(want_t)
    assert np.isfinite(want_t).all() and (want_t > 0).all()
    t, r = q.code_norms(codes_d), q.code_rnorms(codes_d)
    assert t.dtype == r.dtype == torch.float32 and tuple(t.shape) == tuple(r.shape) == (x.B,)
    _same(t.cpu().numpy(), want_t, x.name + ": code_norms against rule 2")
    _same(r.cpu().numpy(), want_r, x.name + ": code_rnorms against rules 2 and 6")
    assert _equal(q.rnorms_from_norms(t), r)
    # the C entries, outputs pre-filled and guarded
    for entry, pub in (("mcq_code_norms", t), ("mcq_code_rnorms", r)):
        got = _abi_norms(q, entry, codes_d)
        assert _equal(got, pub), entry
        assert _equal(got, _abi_norms(q, entry, codes_d)), entry + ": a second call differs"
    assert _equal(_abi_rnorms_from(t), r)
    if x.codes == "bytes":                                            # the mask of rule 2: the digits are the low bits
        assert _equal(q.code_norms(_dev(codes & (x.K - 1))), t)


def test_norms_of_packed_codes_and_of_an_empty_store():
    N, K, D = 8, 16, 17
    q, Cp = _quantizer(N, K, D)
    packed = np.random.RandomState(25).randint(0, 256, size=(37, N // 2)).astype(np.uint8)
    flat = np.stack([packed & 15, packed >> 4], axis=2).reshape(37, N)                # low nibble = even codebook
    want = tg.restate_norms(Cp, flat)
    _same(q.code_norms(_dev(packed)).cpu().numpy(), want, "packed codes")
    _same(q.code_rnorms(_dev(packed)).cpu().numpy(), tg.restate_rnorms(want), "packed codes, reciprocal roots")
    _same(q.code_norms(_dev(flat)).cpu().numpy(), want, "unpacked codes")
    # B = 0: an empty result, and the C entries touch nothing
    empty = _dev(flat[:0])
    assert tuple(q.code_norms(empty).shape) == tuple(q.code_rnorms(empty).shape) == (0,)
    assert tuple(q.rnorms_from_norms(q.code_norms(empty)).shape) == (0,)
    for entry in ("mcq_code_norms", "mcq_code_rnorms"):
        assert _abi_norms(q, entry, empty).numel() == 0
    assert _abi_rnorms_from(torch.empty(0, device="cuda")).numel() == 0
    assert tuple(q.search_tables(torch.empty((0, D), device="cuda")).shape) == (0, N, K)


def test_norms_of_edge_reconstructions():
    q, Cp, C = _hand_made()
    N, K, D = HAND
    codes = np.array([[5, 1],        # C[0][5] + C[1][1] = +0 in every feature: t = +0.0, r = +0.0, never NaN
                      [0, 0],        # rows of zeros
                      [0, 2],        # zeros and -0.0
                      [6, 0],        # one element of 2^100: its square overflows, t = +inf, r = 1 / inf = +0.0
                      [6, 5],
                      [3, 0],        # fp32 subnormals: every square underflows to +0
                      [7, 0],
                      [8, 0],        # 2^-126: likewise
                      [9, 0],        # 2^-70: squares of 2^-140, a subnormal t = 2^-135 and its root 2^67.5
                      [3, 1], [1, 2], [2, 3], [4, 4], [15, 15], [5, 0], [0, 1]], dtype=np.uint8)
    want_t = tg.restate_norms(Cp, codes)
    want_r = tg.restate_rnorms(want_t)
    assert _u32(want_t)[0] == 0 and _u32(want_r)[0] == 0
    assert np.isposinf(want_t[3]) and np.isposinf(want_t[4]) and _u32(want_r)[3] == 0 and _u32(want_r)[4] == 0
    assert (_u32(want_t)[[1, 2, 5, 6, 7]] == 0).all() and (_u32(want_r)[[1, 2, 5, 6, 7]] == 0).all()
    assert 0 < want_t[8] < 2.0 ** -126 and np.isfinite(want_r[8]) and want_r[8] > 2.0 ** 67
    assert not np.isnan(want_t).any() and not np.isnan(want_r).any()
    codes_d = _dev(codes)
    t, r = q.code_norms(codes_d), q.code_rnorms(codes_d)
    _same(t.cpu().numpy(), want_t, "edge reconstructions: norms")
    _same(r.cpu().numpy(), want_r, "edge reconstructions: reciprocal roots")
    assert _equal(q.rnorms_from_norms(t), r) and _equal(_abi_rnorms_from(t), r)
    assert _equal(_abi_norms(q, "mcq_code_norms", codes_d), t) and _equal(_abi_norms(q, "mcq_code_rnorms", codes_d), r)
    # rule 6 on values no store of this state has: the smallest and largest subnormals and normals, and what gives NaN
    vals = np.array([0.0, -0.0, 2.0 ** -149, 2.0 ** -127, 2.0 ** -126, 1.0, 3.0, 2.0 ** 127, 3.4028235e38, np.inf, -1.0, np.nan],
                    dtype=np.float32)
    got = q.rnorms_from_norms(_dev(vals)).cpu().numpy()
    assert _same(got, tg.restate_rnorms(vals), "rnorms_from_norms") == 2
    assert _u32(got)[0] == 0 and _u32(got)[1] == 0                     # t == 0 of either sign: +0.0


# ------------------------------------------------------------------ end to end at the new dims
@pytest.mark.parametrize("shape", tg.END_TO_END, ids=lambda s: "n%d_k%d_d%d" % s[:3])
def test_search_from_restated_tables_and_norms(shape):
    from quantization_amd import synthetic as gen
    N, K, D, Q, B, k = shape
    q, Cp = _quantizer(N, K, D)
    flat = np.random.RandomState(26 + D).randint(0, K, size=(B, N)).astype(np.uint8)
    xq = gen.make_gaussian(27 + D, Q, D)
    T = tg.restate_tables(xq, Cp).reshape(Q, N, K)
    t = tg.restate_norms(Cp, flat)
    r = tg.restate_rnorms(t)
    xq_d, codes_d = _dev(xq), _dev(flat)
    for metric, w in (("l2", t), ("ip", None), ("cosine", r)):
        want_s, want_i = mg.restate_metric(T, w, flat, k, metric)
        assert (want_i >= 0).all()
        val, idx = q.search(xq_d, codes_d, k=k, metric=metric)
        assert np.array_equal(idx.cpu().numpy(), want_i), f"{metric}: indexes differ in rows {np.flatnonzero((idx.cpu().numpy() != want_i).any(1))[:8]}"
        # ... and the scan's scores are rule 3's over the restated arrays, bit for bit
        dev_w = None if w is None else _dev(w)
        s1, i1 = q._search_scan(_dev(T), codes_d, dev_w, k, metric=metric)
        assert np.array_equal(i1.cpu().numpy(), want_i) and np.array_equal(_u32(s1.cpu().numpy()), _u32(want_s)), metric
