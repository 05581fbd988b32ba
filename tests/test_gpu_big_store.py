"""The entries that walk a store of codes, on stores past 2^26 rows and 4 GiB of codes (the C ABI through quantization_amd._lib,
synthetic tables): launch geometry that grows with B, byte offsets past 2^31 and 2^32, positions up to 2^31 - 2.  Every
comparison is bit for bit (uint32 views of floats); the reference is tests/big_store.py -- the existing numpy restatement over
the compact store of planted rows plus the background tail -- which tests/test_big_store_host.py pins on the CPU.

    rows    N = 1,  K = 16, B = 2^26 + 321      64 MiB of codes: one wave per row is 64 * B > 2^32 threads
    bytes   N = 64, K = 16, B = 2^26 + 321      4 GiB + 20 KiB: the byte offset of a row crosses 2^31 and 2^32
    edge    N = 1,  K = 16, B = 2^31 - 1        2 GiB: positions up to 2^31 - 2, one below kNoIndex; inner product, no w

One store is alive at a time (a holder builds it on first use and the next holder frees it), so the module needs about 10 GiB;
a test skips only when less than 16 GiB of device memory are free."""
import numpy as np
import pytest
import torch

import big_store as bs
import rerank_grid as rr
import search_bias_grid as bg
import search_grid as sg
import search_mask_grid as kg
import search_metric_grid as mg
import search_tables_grid as tg
import test_gpu_search as base
from test_gpu_code_norms_based import _padded_centers

pytestmark = pytest.mark.gpu

CHUNK = 1 << 26                                     # rows of a store that an int64 temporary is formed for at a time


def _L():
    from quantization_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _ws(n):
    return torch.empty(max(int(n), 256), dtype=torch.uint8, device="cuda")


class Torch:
    """the device twin of big_store.Numpy"""

    @staticmethod
    def full(shape, value, dtype):
        dt = getattr(torch, dtype)
        return torch.zeros(shape, dtype=dt, device="cuda") if value == 0 else torch.full(shape, value, dtype=dt, device="cuda")

    @staticmethod
    def put(arr, pos, vals):
        arr[_dev(pos)] = _dev(vals)


# ------------------------------------------------------------------ one store alive at a time
class Holder:
    current = None

    def __init__(self, make):
        self.make, self.value = make, None

    def get(self):
        if self.value is None:
            if Holder.current is not None:
                Holder.current.release()
            free, _ = torch.cuda.mem_get_info()
            if free < bs.MIN_FREE:
                pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the big stores need {bs.MIN_FREE // 2 ** 30} GiB")
            self.value = self.make()
            Holder.current = self
        return self.value

    def release(self):
        self.value = None
        if Holder.current is self:
            Holder.current = None
        torch.cuda.empty_cache()


def _store(st, count, metrics, last=None):
    """a holder of (positions, codes on the device, {metric: w on the device or None})"""
    def make():
        pos = bs.planted(st, count, last)
        T = bs.tables(st)
        assert bs.separated(st, T, count), "a planted row does not precede the background: the inputs are wrong"
        codes = bs.build_codes(st, pos, Torch)
        ws = {m: bs.build_w(st, pos, m, Torch) for m in metrics}
        torch.cuda.synchronize()
        return pos, codes, ws
    return Holder(make)


def _fixture(name, st, count, metrics, last=None):
    @pytest.fixture(scope="module", name=name)
    def fx():
        h = _store(st, count, metrics, last)
        yield h
        h.release()
    return fx


rows256 = _fixture("rows256", bs.ROWS, 256, ("ip",))
bytes56 = _fixture("bytes56", bs.BYTES, 56, bs.METRICS)
bytes256 = _fixture("bytes256", bs.BYTES, 256, bs.METRICS)
edge56 = _fixture("edge56", bs.EDGE, 56, ("ip",))
edge_tail = _fixture("edge_tail", bs.EDGE, 56, ("ip",), last=(100, 40))


@pytest.fixture(scope="module", autouse=True)
def _peak():
    torch.cuda.reset_peak_memory_stats()
    yield
    if Holder.current is not None:
        Holder.current.release()
    print(f"\n[big store] peak device memory allocated by the module: {torch.cuda.max_memory_allocated() / 2 ** 30:.2f} GiB")


# ------------------------------------------------------------------ the calls
def _scan(st, T, codes, w, k, metric, mask=None, wide=False, B=None):
    L = _L()
    B = st.B if B is None else B
    Qn = T.shape[0]
    T_d = _dev(T)
    out_s = torch.full((Qn, k), -7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((Qn, k), -7, dtype=torch.int64, device="cuda")
    args = (T_d.data_ptr(), Qn, codes.data_ptr(), None if w is None else w.data_ptr(), B, st.N, st.K, k, mg.CODE[metric])
    if wide:
        ws = _ws(L.mcq_search_wide_workspace_bytes(Qn, B, st.N, st.K, k))
        rc = L.mcq_search_wide(*args, None if mask is None else mask.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                               ws.numel(), _st())
    else:
        ws = _ws(L.mcq_search_workspace_bytes(Qn, B, st.N, st.K, k))
        if mask is None:
            rc = L.mcq_search_scan_metric(*args, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), _st())
        else:
            rc = L.mcq_search_scan_masked(*args, mask.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _lists(st, T, codes, w, k, metric, off, probes, bias=None, entry="mcq_search_scan_lists"):
    L = _L()
    Qn, P = probes.shape
    T_d, off_d, pr_d = _dev(T), _dev(off), _dev(probes)
    bias_d = None if bias is None else _dev(bias)
    out_s = torch.full((Qn, k), -7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((Qn, k), -7, dtype=torch.int64, device="cuda")
    head = (T_d.data_ptr(), Qn, codes.data_ptr(), None if w is None else w.data_ptr(), st.B, st.N, st.K, k, mg.CODE[metric], None,
            off_d.data_ptr(), len(off) - 1, pr_d.data_ptr(), P)
    if entry == "mcq_search_wide_lists":
        ws = _ws(L.mcq_search_wide_lists_workspace_bytes(Qn, P, st.N, st.K, k))
    else:
        ws = _ws(L.mcq_search_lists_workspace_bytes(Qn, P, st.N, st.K, k))
    if entry != "mcq_search_scan_lists":
        head += (None if bias_d is None else bias_d.data_ptr(),)
    rc = getattr(L, entry)(*head, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_i.cpu().numpy()


def _range(st, T, codes, w, metric, thr, lists=None):
    """count, then fill -> (lims, positions, scores) as numpy"""
    L = _L()
    Qn = T.shape[0]
    T_d, thr_d = _dev(T), _dev(thr)
    lims = torch.full((Qn + 1,), -7, dtype=torch.int64, device="cuda")
    head = (T_d.data_ptr(), Qn, codes.data_ptr(), None if w is None else w.data_ptr(), st.B, st.N, st.K, mg.CODE[metric])
    if lists is None:
        ws = _ws(L.mcq_search_range_workspace_bytes(Qn, st.B, st.N, st.K))
        count, fill = L.mcq_search_range_count, L.mcq_search_range_fill
    else:
        off_d, pr_d = _dev(lists[0]), _dev(lists[1])
        head += (None, off_d.data_ptr(), len(lists[0]) - 1, pr_d.data_ptr(), lists[1].shape[1])
        ws = _ws(L.mcq_search_range_lists_workspace_bytes(Qn, lists[1].shape[1], st.N, st.K))
        count, fill = L.mcq_search_range_lists_count, L.mcq_search_range_lists_fill
    rc = count(*head, thr_d.data_ptr(), lims.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    total = int(lims[-1])
    assert 0 <= total <= 4096, f"{total} listed: the background was listed"
    out_s = torch.full((max(total, 1),), -7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((max(total, 1),), -7, dtype=torch.int64, device="cuda")
    rc = fill(*head, thr_d.data_ptr(), lims.data_ptr(), out_s.data_ptr(), out_i.data_ptr(), total, ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return lims.cpu().numpy(), out_i.cpu().numpy()[:total], out_s.cpu().numpy()[:total]


def _same_lists(got, want, what):
    (g_s, g_i), (w_s, w_i) = got, want
    assert np.array_equal(g_i, w_i), (what, "positions differ", np.argwhere(g_i != w_i)[:4].tolist(), g_i[g_i != w_i][:4], w_i[g_i != w_i][:4])
    assert np.array_equal(_u32(g_s), _u32(w_s)), (what, "scores differ", np.argwhere(_u32(g_s) != _u32(w_s))[:4].tolist())


def _same_csr(got, want, what):
    (g_l, g_p, g_v), (w_l, w_p, w_v) = got, want
    assert np.array_equal(g_l, w_l), (what, "lims differ", g_l, w_l)
    assert np.array_equal(g_p, w_p), (what, "listed positions differ")
    assert np.array_equal(_u32(g_v), _u32(w_v)), (what, "listed scores differ")


def _chunks(B):
    return [(a, min(B, a + CHUNK)) for a in range(0, B, CHUNK)]


def _third_flags(B, pos):
    """uint8 (B,) on the device: b % 3 != 0, and the planted rows"""
    flags = torch.empty(B, dtype=torch.uint8, device="cuda")
    for a, z in _chunks(B):
        flags[a:z] = (torch.arange(a, z, device="cuda") % 3 != 0).to(torch.uint8)
    flags[_dev(pos)] = 1
    return flags


def _expected_words(flags):
    """rule 10 with torch: view as (words, 64), times powers of two, summed in int64; the ragged last word apart"""
    B = flags.numel()
    full = B // 64
    pw = _dev((np.uint64(1) << np.arange(64, dtype=np.uint64)).view(np.int64))
    out = torch.zeros((B + 63) // 64, dtype=torch.int64, device="cuda")
    step = CHUNK // 64
    for a in range(0, full, step):
        z = min(full, a + step)
        out[a:z] = ((flags[a * 64:z * 64].view(z - a, 64) != 0).to(torch.int64) * pw[None, :]).sum(1)
    if B % 64:
        out[full] = ((flags[full * 64:] != 0).to(torch.int64) * pw[:B % 64]).sum()
    return out


def _check_pack(st, pos):
    L = _L()
    B = st.B
    flags = _third_flags(B, pos)
    words = (B + 63) // 64
    got = torch.full((words + 8,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    rc = L.mcq_search_pack_mask(flags.data_ptr(), B, got.data_ptr(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((got[words:] == 0x5A5A5A5A).all()), "words past the mask were written"
    assert torch.equal(got[:words], _expected_words(flags))
    first = flags[:4096].cpu().numpy() != 0
    assert np.array_equal(got[:64].cpu().numpy(), kg.pack(first))
    a = (B - 4096) // 64 * 64
    assert np.array_equal(got[a // 64:words].cpu().numpy(), kg.pack(flags[a:].cpu().numpy() != 0))
    for p in pos[[0, 1, -2, -1]]:
        assert (int(got[int(p) >> 6]) >> (int(p) & 63)) & 1 == 1


# ------------------------------------------------------------------ rows: 64 * B threads pass 2^32
def _norms_state():
    q = base._quantizer(sg.Case("big_norms", 1, 16, 4, 1, 1, 1, state="decode_only", codes="random"))
    return q, _padded_centers(q)


@pytest.mark.parametrize("entry", ("mcq_code_norms", "mcq_code_rnorms", "mcq_code_norms_based", "mcq_code_rnorms_based"))
def test_rows_code_norms(rows256, entry):
    st = bs.ROWS
    pos, codes, _ = rows256.get()
    L, B = _L(), st.B
    q, Cp = _norms_state()
    N, K, D = 1, 16, 4
    assert Cp.shape == (N, K, 16)
    blob = q._prepared(any_flavour=True)
    based, rn = entry.endswith("_based"), "rnorms" in entry
    rs = np.random.RandomState(44)
    cen = (rs.standard_normal((5, D)) * float(np.abs(Cp).max())).astype(np.float32)
    # the expected values: one per distinct (digit, assign) pair, assign = b % 7 with 5 base rows (5 and 6 name no row)
    dig = np.repeat(np.arange(K, dtype=np.uint8), 7)[:, None]
    asg = np.tile(np.arange(7, dtype=np.int32), K)
    table = bg.restate_norms_based(Cp, dig, cen, asg, D) if based else np.repeat(tg.restate_norms(Cp, np.arange(K, dtype=np.uint8)[:, None]), 7)
    if based:
        assert np.array_equal(_u32(table[5::7]), _u32(tg.restate_norms(Cp, np.arange(K, dtype=np.uint8)[:, None])))
    if rn:
        table = tg.restate_rnorms(table)
    assert len(set(_u32(table[:7 * K:7]).tolist())) == K
    out = torch.full((B + 1024,), -7.0, dtype=torch.float32, device="cuda")
    assign = torch.empty(B, dtype=torch.int32, device="cuda")
    for a, z in _chunks(B):
        assign[a:z] = (torch.arange(a, z, device="cuda") % 7).to(torch.int32)
    if based:
        cen_d = _dev(cen)
        rc = getattr(L, entry)(codes.data_ptr(), B, blob.data_ptr(), N, K, D, cen_d.data_ptr(), 5, assign.data_ptr(), out.data_ptr(), _st())
    else:
        rc = getattr(L, entry)(codes.data_ptr(), B, blob.data_ptr(), N, K, D, out.data_ptr(), _st())
    assert rc == 0, f"{entry} over {B} rows returned {rc}"
    torch.cuda.synchronize()
    assert bool((out[B:] == -7.0).all()), "floats past the output were written"
    table_d = _dev(table)
    for a, z in _chunks(B):
        want = table_d[codes[a:z, 0].to(torch.int64) * 7 + assign[a:z].to(torch.int64)]
        same = out[a:z].view(torch.int32) == want.view(torch.int32)
        assert bool(same.all()), f"{entry}: {int((~same).sum())} of rows [{a}, {z}) differ, first at {a + int(torch.nonzero(~same)[0])}"
    assert int((codes[_dev(pos), 0] != 0).sum()) == len(pos)


def test_rows_rnorms_from_norms(rows256):
    rows256.get()
    L, B = _L(), bs.ROWS.B
    vals = np.abs(np.random.RandomState(45).standard_normal(4093)).astype(np.float32) * np.float32(100)
    vals[:6] = [0.0, 2.0 ** -149, 2.0 ** -126, 1.0, 3.0, np.inf]
    norms = torch.empty(B, dtype=torch.float32, device="cuda")
    vals_d, want_d = _dev(vals), _dev(mg.restate_rnorms(vals))
    want = torch.empty(B, dtype=torch.float32, device="cuda")
    for a, z in _chunks(B):
        at = torch.arange(a, z, device="cuda") % 4093
        norms[a:z], want[a:z] = vals_d[at], want_d[at]
    out = torch.full((B + 1024,), -7.0, dtype=torch.float32, device="cuda")
    rc = L.mcq_rnorms_from_norms(norms.data_ptr(), B, out.data_ptr(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert bool((out[B:] == -7.0).all()) and torch.equal(out[:B].view(torch.int32), want.view(torch.int32))


def test_rows_pack_mask(rows256):
    pos, _, _ = rows256.get()
    _check_pack(bs.ROWS, pos)


@pytest.mark.parametrize("layout", ("one_byte", "a_byte_per_digit"))
def test_rows_decode(rows256, layout):
    """2 x 16 codebooks, D = 4: one byte per row holding both digits (the low nibble is codebook 0), and the same digits
    a byte each; the result is asserted, not which kernel the selection took (today two different ones)"""
    rows256.get()
    L, B = _L(), bs.ROWS.B
    q = base._quantizer(sg.Case("big_decode", 2, 16, 4, 1, 1, 1, state="decode_only", codes="random"))
    Cp = _padded_centers(q)
    blob = q._prepared(any_flavour=True)
    v = np.arange(256)
    table = (Cp[0, v & 15, :4] + Cp[1, v >> 4, :4]).astype(np.float32)
    codes = torch.empty(B, dtype=torch.uint8, device="cuda")
    for a, z in _chunks(B):
        codes[a:z] = (((torch.arange(a, z, device="cuda") * 2654435761) >> 11) & 255).to(torch.uint8)
    assert int(torch.bincount(codes[:1 << 20].to(torch.int64), minlength=256).min()) > 0
    out = torch.full((B + 64, 4), -7.0, dtype=torch.float32, device="cuda")
    if layout == "one_byte":
        rc = L.mcq_decode(codes.data_ptr(), 1, 1, B, blob.data_ptr(), 2, 16, 4, out.data_ptr(), _st())
    else:
        split = torch.stack([codes & 15, codes >> 4], dim=1).contiguous()
        rc = L.mcq_decode(split.data_ptr(), 1, 2, B, blob.data_ptr(), 2, 16, 4, out.data_ptr(), _st())
    assert rc == 0, f"mcq_decode over {B} rows returned {rc}"
    torch.cuda.synchronize()
    assert bool((out[B:] == -7.0).all()), "rows past the output were written"
    table_d = _dev(table)
    got = out.view(torch.int32)
    for a in range(0, B, 1 << 24):
        z = min(B, a + (1 << 24))
        want = table_d[codes[a:z].to(torch.int64)].view(torch.int32)
        if not torch.equal(got[a:z], want):
            bad = torch.nonzero((got[a:z] != want).reshape(-1))
            raise AssertionError(f"{bad.numel()} floats of rows [{a}, {z}) differ, first in row {a + int(bad[0]) // 4}")


@pytest.mark.parametrize("metric", ("ip", "l2"))
def test_rows_range_count_lists_everything(rows256, metric):
    """Q = 40 and thr = +inf: lims[q] = q * B exactly, lims[40] above 2^31.  No fill."""
    st = bs.ROWS
    pos, codes, _ = rows256.get()
    L, Qn = _L(), 40
    T_d = _dev(bs.tables(st, Qn))
    thr = torch.full((Qn,), float("inf"), device="cuda")
    w = None if metric == "ip" else torch.zeros(st.B, dtype=torch.float32, device="cuda")
    lims = torch.full((Qn + 1,), -7, dtype=torch.int64, device="cuda")
    ws = _ws(L.mcq_search_range_workspace_bytes(Qn, st.B, st.N, st.K))
    rc = L.mcq_search_range_count(T_d.data_ptr(), Qn, codes.data_ptr(), None if w is None else w.data_ptr(), st.B, st.N, st.K,
                                  mg.CODE[metric], thr.data_ptr(), lims.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert np.array_equal(lims.cpu().numpy(), np.arange(Qn + 1, dtype=np.int64) * st.B) and int(lims[-1]) > 2 ** 31


# ------------------------------------------------------------------ bytes: byte offsets cross 2^31 and 2^32
@pytest.mark.parametrize("metric", bs.METRICS)
def test_bytes_scan_with_background_tail(bytes56, metric):
    st = bs.BYTES
    pos, codes, ws = bytes56.get()
    assert codes.numel() == st.B * 64 > 2 ** 32
    T = bs.tables(st)
    want = bs.reference_topk(st, T, pos, 64, metric)
    tail = bs.tail_positions(pos, [(0, st.B)], 8)
    assert np.array_equal(want[1][:, 56:], np.tile(tail, (bs.Q, 1))) and (_u32(want[0][:, 56:]) == _u32(st.bg())).all()
    assert tail.tolist() == [2, 3, 4, 5, 6, 7, 8, 9]
    _same_lists(_scan(st, T, codes, ws[metric], 64, metric), want, f"scan {metric}")


def _cleared_mask(st, pos, kept):
    """every bit set (those past B too: rule 10 ignores them) but those of the planted rows that are not kept"""
    words = torch.full(((st.B + 63) // 64,), -1, dtype=torch.int64, device="cuda")
    for p in pos[~kept]:
        words[int(p) >> 6] &= ~(torch.ones((), dtype=torch.int64, device="cuda") << (int(p) & 63))
    return words


@pytest.mark.parametrize("metric", ("l2", "cosine"))
def test_bytes_scan_masked(bytes256, metric):
    st = bs.BYTES
    pos, codes, ws = bytes256.get()
    kept = np.arange(len(pos)) % 3 != 0
    T = bs.tables(st)
    got = _scan(st, T, codes, ws[metric], 64, metric, mask=_cleared_mask(st, pos, kept))
    _same_lists(got, bs.reference_topk(st, T, pos, 64, metric, kept=kept), f"masked scan {metric}")
    assert not np.isin(got[1], pos[~kept]).any()


@pytest.mark.parametrize("metric", bs.METRICS)
def test_bytes_scan_lists(bytes256, metric):
    st = bs.BYTES
    pos, codes, ws = bytes256.get()
    off, probes = bs.list_layout(st)
    assert {2 ** 25 - 1, 2 ** 25 + 1, 2 ** 26} <= set(off.tolist()) and off[0] == 0 and off[-1] == st.B
    T = bs.tables(st)
    want = bs.reference_lists(st, T, pos, off, probes, 64, metric)
    assert (want[1][2] == -1).all() and _u32(want[0][1, -1]) == _u32(st.bg()) and want[1][1, 0] >= 0
    _same_lists(_lists(st, T, codes, ws[metric], 64, metric, off, probes), want, f"lists {metric}")


@pytest.mark.parametrize("metric", bs.METRICS)
def test_bytes_scan_lists_bias(bytes256, metric):
    st = bs.BYTES
    pos, codes, ws = bytes256.get()
    off, probes = bs.list_layout(st)
    T = bs.tables(st)
    bias = np.random.RandomState(5).uniform(-2.0, 2.0, size=probes.shape).astype(np.float32)
    want = bs.reference_lists(st, T, pos, off, probes, 64, metric, bias=bias)
    got = _lists(st, T, codes, ws[metric], 64, metric, off, probes, bias=bias, entry="mcq_search_scan_lists_bias")
    _same_lists(got, want, f"lists with a bias {metric}")
    plain = _lists(st, T, codes, ws[metric], 64, metric, off, probes, bias=None, entry="mcq_search_scan_lists_bias")
    _same_lists(plain, bs.reference_lists(st, T, pos, off, probes, 64, metric), f"lists with a null bias {metric}")


@pytest.mark.parametrize("metric", bs.METRICS)
def test_bytes_range(bytes256, metric):
    st = bs.BYTES
    pos, codes, ws = bytes256.get()
    T = bs.tables(st)
    thr = bs.thresholds(st, T, len(pos), metric)
    want = bs.reference_range(st, T, pos, metric, thr)
    assert want[0][-1] > 10 and want[0][3] == want[0][2]                  # query 2 takes -inf
    _same_csr(_range(st, T, codes, ws[metric], metric, thr), want, f"range {metric}")
    off, probes = bs.list_layout(st)
    want = bs.reference_range_lists(st, T, pos, off, probes, metric, thr)
    assert want[0][1] > 0 and want[0][2] >= want[0][1]
    _same_csr(_range(st, T, codes, ws[metric], metric, thr, lists=(off, probes)), want, f"range list by list {metric}")


@pytest.mark.parametrize("metric", ("l2", "ip"))
def test_bytes_wide(bytes256, metric):
    """k = 300 over 256 planted rows: 44 background rows follow in ascending position"""
    st = bs.BYTES
    pos, codes, ws = bytes256.get()
    T = bs.tables(st)
    want = bs.reference_topk(st, T, pos, 300, metric)
    assert (want[1][:, 256:] == np.tile(bs.tail_positions(pos, [(0, st.B)], 44), (bs.Q, 1))).all() and (want[1] >= 0).all()
    _same_lists(_scan(st, T, codes, ws[metric], 300, metric, wide=True), want, f"wide {metric}")
    off, probes = bs.list_layout(st)
    want = bs.reference_lists(st, T, pos, off, probes, 300, metric)
    got = _lists(st, T, codes, ws[metric], 300, metric, off, probes, entry="mcq_search_wide_lists")
    _same_lists(got, want, f"wide list by list {metric}")


@pytest.fixture(scope="module")
def vectors256():
    """fp16 [B][32], 4 GiB: zeros but for the planted rows"""
    def make():
        st = bs.BYTES
        pos = bs.planted(st, 256)
        X = torch.zeros((st.B, 32), dtype=torch.float16, device="cuda")
        rows = np.random.RandomState(46).standard_normal((len(pos), 32)).astype(np.float16)
        X[_dev(pos)] = _dev(rows)
        torch.cuda.synchronize()
        return pos, X, rows
    h = Holder(make)
    yield h
    h.release()


@pytest.mark.parametrize("metric", bs.METRICS)
def test_bytes_rerank(vectors256, metric):
    st = bs.BYTES
    pos, X, rows = vectors256.get()
    L, B, D, S, k, Bs = _L(), st.B, 32, 1024, 100, 1024
    assert X.numel() * 2 > 2 ** 32
    rs = np.random.RandomState(47)
    # row_of: the planted rows, the background rows above 2^26 and beside the crossings, and random background, scrambled
    near = np.array([p for p in list(range(2 ** 26 + 2, 2 ** 26 + 300, 3)) + [2 ** 25 - 2, 2 ** 25 + 2, 2 ** 26 - 2, 2, 3] if p not in set(pos.tolist())])
    fill = rs.randint(0, B, size=Bs - len(pos) - len(near))
    row_of = rs.permutation(np.concatenate([pos, near, fill])).astype(np.int64)
    assert len(row_of) == Bs and int((row_of > 2 ** 26).sum()) > 100
    short = np.stack([rs.permutation(Bs) for _ in range(bs.Q)]).astype(np.int64)
    short[1, ::5] = -1
    short[2, 7] = Bs
    queries = rs.standard_normal((bs.Q, D)).astype(np.float32)
    gathered = X[_dev(row_of)].cpu().numpy()                              # the rows the shortlist can name, by entry of row_of
    back = {int(p): j for j, p in enumerate(pos)}
    for j, r in enumerate(row_of):
        assert np.array_equal(gathered[j], rows[back[int(r)]] if int(r) in back else np.zeros(D, dtype=np.float16))
    want_s, want_i, _ = rr.restate(queries, gathered, short, k, metric, row_of=np.arange(Bs, dtype=np.int64))
    q_d, sh_d, ro_d = _dev(queries), _dev(short), _dev(row_of)
    out_s = torch.full((bs.Q, k), -7.0, dtype=torch.float32, device="cuda")
    out_i = torch.full((bs.Q, k), -7, dtype=torch.int64, device="cuda")
    ws = _ws(L.mcq_rerank_workspace_bytes(bs.Q, S, D, k))
    rc = L.mcq_rerank(q_d.data_ptr(), 0, bs.Q, X.data_ptr(), 1, B, D, sh_d.data_ptr(), S, ro_d.data_ptr(), Bs, k, mg.CODE[metric],
                      out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _same_lists((out_s.cpu().numpy(), out_i.cpu().numpy()), (want_s, want_i), f"rerank {metric}")


# ------------------------------------------------------------------ edge: positions up to 2^31 - 2
def test_edge_scan_ip(edge56):
    st = bs.EDGE
    pos, codes, ws = edge56.get()
    assert pos[-1] == 2 ** 31 - 2 and pos[-2] == 2 ** 31 - 3 and st.B == sg.constants()["kNoIndex"]
    T = bs.tables(st)
    want = bs.reference_topk(st, T, pos, 64, "ip")
    got = _scan(st, T, codes, None, 64, "ip")
    _same_lists(got, want, "scan at the edge")
    assert (got[1] == 2 ** 31 - 2).sum() == bs.Q and (got[1] >= 0).all()


def test_edge_scan_masked_keeps_the_last_rows(edge_tail):
    """a mask that keeps the last 100 rows, 40 of them planted.  k = 64 (the most mcq_search_scan_masked takes): the 40 planted
    rows, then the 24 lowest of the 60 background rows; mcq_search_wide with k = 128: all 60, then (+inf, -1)."""
    st = bs.EDGE
    pos, codes, ws = edge_tail.get()
    B = st.B
    kept = pos >= B - 100
    assert int(kept.sum()) == 40
    words = torch.zeros((B + 63) // 64, dtype=torch.int64, device="cuda")
    keep = np.zeros(128, dtype=bool)
    a = (B - 100) // 64 * 64
    keep[B - 100 - a:B - a] = True
    words[a // 64:] = _dev(kg.pack(keep)[:len(words) - a // 64])
    T = bs.tables(st)
    want = bs.reference_topk(st, T, pos, 64, "ip", kept=kept, keep_from=B - 100)
    got = _scan(st, T, codes, None, 64, "ip", mask=words)
    _same_lists(got, want, "masked scan at the edge")
    assert (got[1][:, :40] >= B - 100).all() and (got[1] == 2 ** 31 - 2).sum() == bs.Q and (got[1] != -1).all()
    want = bs.reference_topk(st, T, pos, 128, "ip", kept=kept, keep_from=B - 100)
    assert (want[1][:, 100:] == -1).all() and (want[1][:, :100] >= B - 100).all() and np.isinf(want[0][:, 100:]).all()
    _same_lists(_scan(st, T, codes, None, 128, "ip", mask=words, wide=True), want, "masked wide scan at the edge")


def test_edge_pack_mask(edge56):
    pos, _, _ = edge56.get()
    _check_pack(bs.EDGE, pos)
