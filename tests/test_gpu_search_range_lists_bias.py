"""The range search list by list with a bias per probe slot on the GPU (mcq_search_range_lists_bias_count / _fill through
Quantizer._search_range(lists=..., bias=...), Quantizer.range_search_lists(probe_bias=...); include/mcq_residual.h rules 21 and 23),
BIT FOR BIT against the numpy restatement of tests/search_bias_grid.py.

Per case of tests/search_range_lists_grid.py x metric x mask (none, `half`), with the bias of search_bias_grid.bias_for and
the thresholds of the range grid applied to the BIASED scores (queries with no hit, some hits and all hits):
  * lims, positions and scores (as int32) equal the restatement, the slots of a row in order -- a list named twice is listed
    twice, each time under the bias of that naming's slot; count and fill agree (the fill stores lims[Q] entries and the
    sentinels behind them survive); a second call returns identical bytes;
  * some query's hits differ from the call without a bias;
  * probe_bias == NULL through the new entries is the old pair, bit for bit;
  * a fill with half the room stores the first half and nothing else.
Then every cell of launch_range_lists with a bias once, and the public call: an unsorted probe row with its bias gives the CSR of the
sorted row with the bias permuted alike."""
import numpy as np
import pytest
import torch

import search_bias_grid as bg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_lists_grid as rl
import search_selection_grid as sel
import test_gpu_search_lists_bias as tb
import test_gpu_search_range_lists as tr

pytestmark = pytest.mark.gpu

SEED = 1
SENTINEL_S, SENTINEL_I = tr.SENTINEL_S, tr.SENTINEL_I
_BIAS = {}


def _i32(t):
    return t.view(torch.int32)


def _sums(case):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes = tr._prepared(case)[:10]
    if _BIAS.get("name") != case.name:
        _BIAS.clear()
        S = mg.restate_sums(tables.cpu().numpy(), flat)
        _BIAS.update(name=case.name, v=(S, bg.bias_for(S, off, probes, SEED)))
    return _BIAS["v"]


def _direct(q, tables, flat_d, w, metric, words, off_d, probes_d, bias_d, thr_d, capacity, room, biased_entry=True):
    """count, then fill with `capacity` into buffers of `room` slots preset to the sentinels -> (lims, scores, positions);
    biased_entry False: the pair without a bias argument"""
    from quantization_amd import _lib
    L = _lib.lib()
    Q, B, N, K, P = tables.shape[0], flat_d.shape[0], q.num_codebooks, q.codebook_size, probes_d.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(L.mcq_search_range_lists_workspace_bytes(Q, P, N, K), dtype=torch.uint8, device="cuda")
    lims = torch.empty(Q + 1, dtype=torch.int64, device="cuda")
    out_s = torch.full((room,), SENTINEL_S, dtype=torch.float32, device="cuda")
    out_i = torch.full((room,), SENTINEL_I, dtype=torch.int64, device="cuda")
    args = (tables.data_ptr(), Q, flat_d.data_ptr(), None if w is None else w.data_ptr(), B, N, K, q._METRICS[metric],
            None if words is None else words.data_ptr(), off_d.data_ptr(), off_d.numel() - 1, probes_d.data_ptr(), P)
    if biased_entry:
        args += (None if bias_d is None else bias_d.data_ptr(),)
    args += (thr_d.data_ptr(), lims.data_ptr())
    count, fill = (L.mcq_search_range_lists_bias_count, L.mcq_search_range_lists_bias_fill) if biased_entry else \
        (L.mcq_search_range_lists_count, L.mcq_search_range_lists_fill)
    assert count(*args, ws.data_ptr(), ws.numel(), st) == 0
    assert fill(*args, out_s.data_ptr(), out_i.data_ptr(), capacity, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    return lims, out_s, out_i


@pytest.mark.parametrize("pattern", bg.PATTERNS, ids=lambda p: p or "nomask")
@pytest.mark.parametrize("metric", bg.METRICS)
@pytest.mark.parametrize("case", rl.CASES, ids=lambda c: c.name)
def test_range_lists_bias_case(case, metric, pattern):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tr._prepared(case)
    w, _ = tr._per_metric(case, metric)
    S, bias = _sums(case)
    Q, B = case.Q, case.B
    keep = None if pattern is None else kg.keep_for(pattern, B, SEED, case.k)
    keep_d = None if keep is None else torch.from_numpy(keep).cuda()
    words = None if keep_d is None else q.pack_mask(keep_d)
    bias_d = torch.from_numpy(bias).cuda()
    tables, flat_d = tables.contiguous(), flat_d.contiguous()
    w_h = None if w is None else w.cpu().numpy()
    s = bg.biased_scores(S, off, probes, bias, w_h, metric)

    for shift in ((0, 4) if Q == 1 else (0,)):               # (the one query of a case lists nothing at shift 0: -inf)
        thr = rl.thresholds_for(s, off, probes, keep, shift)
        thr_d = torch.from_numpy(thr).cuda()
        got = q._search_range(tables, flat_d, w, thr_d, metric, mask=keep_d, lists=(off_d, probes_d), bias=bias_d)
        want = bg.restate_range_lists_bias(S, off, probes, bias, w_h, metric, thr, keep)
        n = np.diff(want[0])
        print(f"[range lists bias] {case.name} {metric} {pattern} shift {shift}: listed per query {n.min()} .. {n.max()}, {want[0][-1]} in all")
        tr._check(got, want, "the call")
        again = q._search_range(tables, flat_d, w, thr_d, metric, mask=words, lists=(off_d, probes_d), bias=bias_d)
        assert tr._same(got, again)

    # the bias decides something: under the same thresholds the call without one lists other hits
    plain = q._search_range(tables, flat_d, w, thr_d, metric, mask=keep_d, lists=(off_d, probes_d))
    if bg.rows_with_two_lists(off, probes) and int(got[0][-1]) > 0:
        assert not tr._same(got, plain), "the bias changed nothing"

    # count and fill agree: exactly lims[Q] entries are stored; and NULL through the new pair is the old pair
    total = int(got[0][-1])
    lims, out_s, out_i = _direct(q, tables, flat_d, w, metric, words, off_d, probes_d, bias_d, thr_d, total + 64, total + 64)
    assert torch.equal(lims, got[0]) and torch.equal(out_i[:total], got[2]) and torch.equal(_i32(out_s[:total]), _i32(got[1]))
    assert bool((out_i[total:] == SENTINEL_I).all()) and bool((out_s[total:] == SENTINEL_S).all()), "fill stored more than count counted"
    ptotal = int(plain[0][-1])
    a = _direct(q, tables, flat_d, w, metric, words, off_d, probes_d, None, thr_d, ptotal, ptotal + 64)
    b = _direct(q, tables, flat_d, w, metric, words, off_d, probes_d, None, thr_d, ptotal, ptotal + 64, biased_entry=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(_i32(a[1]), _i32(b[1]))
    assert torch.equal(a[0], plain[0]) and torch.equal(a[2][:ptotal], plain[2]) and torch.equal(_i32(a[1][:ptotal]), _i32(plain[1]))

    # a fill with half the room: the first half is right and nothing else is written
    cap = total // 2
    lims, out_s, out_i = _direct(q, tables, flat_d, w, metric, words, off_d, probes_d, bias_d, thr_d, cap, total + 64)
    assert torch.equal(lims, got[0])
    assert torch.equal(out_i[:cap], got[2][:cap]) and torch.equal(_i32(out_s[:cap]), _i32(got[1][:cap]))
    assert bool((out_i[cap:] == SENTINEL_I).all()) and bool((out_s[cap:] == SENTINEL_S).all()), "stored past the capacity"


@pytest.mark.parametrize("N", bg.CELL_NS)
def test_every_cell_of_launch_range_lists_bias(N):
    case, q, flat, flat_d, tables, norms, rnorms, off, probes, S, bias = tb._cell(N)
    off_d, probes_d, bias_d = torch.from_numpy(off).cuda(), torch.from_numpy(probes).cuda(), torch.from_numpy(bias).cuda()
    keep, words = sel.mask_for(case.B)
    words_d = torch.from_numpy(words).cuda()
    tables = tables.contiguous()
    for metric in bg.METRICS:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        w_h = None if w is None else w.cpu().numpy()
        s = bg.biased_scores(S, off, probes, bias, w_h, metric)
        for masked in bg.CELL_MASKS:
            k_ = keep if masked else None
            thr = rl.thresholds_for(s, off, probes, k_, shift=2)             # about 1 %, about half, everything
            want = bg.restate_range_lists_bias(S, off, probes, bias, w_h, metric, thr, k_)
            assert (np.diff(want[0]) > 0).all()
            total = int(want[0][-1])
            lims, out_s, out_i = _direct(q, tables, flat_d, w, metric, words_d if masked else None, off_d, probes_d, bias_d,
                                         torch.from_numpy(thr).cuda(), total, total + 8)      # both sweeps: count, then fill
            tr._check((lims, out_s[:total], out_i[:total]), want, (N, metric, masked))
            assert bool((out_i[total:] == SENTINEL_I).all())


@pytest.mark.parametrize("metric", bg.METRICS)
def test_public_call_permutes_the_bias_with_the_row(metric):
    case = rl.CASES[1]                                       # rows that do not ascend, padding, a row of padding only
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tr._prepared(case)
    S, bias = _sums(case)
    Q, L = case.Q, len(off) - 1
    bias_d = torch.from_numpy(bias).cuda()
    assert any(row.tolist() != sorted(row.tolist()) for row in probes)
    # the sorted rows, and the bias of each entry travelling with it (entries that name no list: any order among themselves)
    clean = np.where((probes >= 0) & (probes < L), probes, -1).astype(np.int32)
    perm = np.argsort(clean, axis=1, kind="stable")
    asc, asc_bias = np.take_along_axis(clean, perm, axis=1), np.take_along_axis(bias, perm, axis=1)
    assert np.array_equal(asc, rl.sorted_rows(probes, L))
    asc_d, asc_bias_d = torch.from_numpy(asc).cuda(), torch.from_numpy(asc_bias).cuda()
    val10 = q.search_lists(xq, kept, off_d, probes_d, k=10, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias_d)[0][:, 9]
    radius = torch.where(torch.isfinite(val10), val10, torch.zeros_like(val10))
    a = q.range_search_lists(xq, kept, off_d, probes_d, radius, norms=norms, metric=metric, rnorms=rnorms, probe_bias=bias_d)
    b = q.range_search_lists(xq, kept, off_d, asc_d, radius, norms=norms, metric=metric, rnorms=rnorms, probe_bias=asc_bias_d)
    assert int(a[0][-1]) > Q and tr._same(a, b)
    # int64 probes with an entry past int32, leading dimensions on all three
    far = probes_d.to(torch.int64)
    far[far < 0] = 1 << 40
    c = q.range_search_lists(xq.reshape(1, Q, case.D), kept, off_d, far.reshape(1, Q, case.P), radius, norms=norms, metric=metric,
                             rnorms=rnorms, probe_bias=bias_d.reshape(1, Q, case.P))
    assert tr._same(a, c)
    # against the C entry with the sorted rows: the reported values are _reported's of its scores, the positions its own
    w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
    qq = (xq.float() * xq.float()).sum(dim=1)
    thr = radius - qq if metric == "l2" else (radius * -2.0 if metric == "ip" else radius * -2.0 * qq.sqrt())
    d = q._search_range(tables, flat_d, w, thr, metric, lists=(off_d, asc_d), bias=asc_bias_d)
    assert torch.equal(d[0], a[0]) and torch.equal(d[2], a[2])
