"""The search list by list with a bias per probe slot on the GPU (mcq_search_scan_lists_bias through
Quantizer._search_scan(lists=..., bias=...); include/mcq_residual.h rules 21 and 23), BIT FOR BIT against the numpy restatement of
tests/search_bias_grid.py.

Per case of tests/search_lists_grid.py x metric x mask (none, `half` of tests/search_mask_grid.py), with the bias of
search_bias_grid.bias_for (normal values scaled to the spread of the case's table sums, zeros, negatives and one -0.0):
  * scores (as int32) and positions of EVERY query equal the restatement: per query each candidate's table sum plus the bias
    of the one slot whose list holds it, the metric's finish, then rule 4 over the candidates;
  * for at least one query that probes two lists the result differs from the call without a bias (else the case shows nothing);
  * a second call returns identical bytes;
  * bias = None through the new entry is the old entry, bit for bit.
Then every cell of launch_lists with a bias once (the lists cells of tests/search_selection_grid.py), and the calls without a
candidate."""
import numpy as np
import pytest
import torch

import search_bias_grid as bg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_selection_grid as sel
import test_gpu_search as base
import test_gpu_search_lists as tl

pytestmark = pytest.mark.gpu

SEED = 1
_BIAS = {}


def _i32(t):
    return t.view(torch.int32)


def _sums(case):
    """(S of rule 3 for the whole store, the bias of the case): once per case, from the tables the device returned"""
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes = tl._prepared(case)[:10]
    if _BIAS.get("name") != case.name:
        _BIAS.clear()
        S = mg.restate_sums(tables.cpu().numpy(), flat)
        _BIAS.update(name=case.name, v=(S, bg.bias_for(S, off, probes, SEED)))
    return _BIAS["v"]


def _direct(q, tables, flat_d, w, k, metric, words, off_d, probes_d, bias_d, entry):
    """one call of a top-k entry list by list: `entry` with a bias argument (None: NULL), or the entry without one"""
    from quantization_amd import _lib
    L = _lib.lib()
    Q, B, N, K, P = tables.shape[0], flat_d.shape[0], q.num_codebooks, q.codebook_size, probes_d.shape[1]
    ws = torch.empty(L.mcq_search_lists_workspace_bytes(Q, P, N, K, k), dtype=torch.uint8, device="cuda")
    out_s = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    out_i = torch.empty((Q, k), dtype=torch.int64, device="cuda")
    args = (tables.data_ptr(), Q, flat_d.data_ptr(), None if w is None else w.data_ptr(), B, N, K, k, q._METRICS[metric],
            None if words is None else words.data_ptr(), off_d.data_ptr(), off_d.numel() - 1, probes_d.data_ptr(), P)
    if entry == "mcq_search_scan_lists_bias":
        args += (None if bias_d is None else bias_d.data_ptr(),)
    rc = getattr(L, entry)(*args, out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, (entry, rc)
    torch.cuda.synchronize()
    return out_s, out_i


@pytest.mark.parametrize("pattern", bg.PATTERNS, ids=lambda p: p or "nomask")
@pytest.mark.parametrize("metric", bg.METRICS)
@pytest.mark.parametrize("case", lg.CASES, ids=lambda c: c.name)
def test_lists_bias_case(case, metric, pattern):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tl._prepared(case)
    w, _ = tl._per_metric(case, metric)
    S, bias = _sums(case)
    Q, B, k = case.Q, case.B, case.k
    keep = None if pattern is None else kg.keep_for(pattern, B, SEED, k)
    keep_d = None if keep is None else torch.from_numpy(keep).cuda()
    bias_d = torch.from_numpy(bias).cuda()
    tables, flat_d = tables.contiguous(), flat_d.contiguous()

    gs, gi = q._search_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d), bias=bias_d)
    assert gs.dtype == torch.float32 and gi.dtype == torch.int64 and tuple(gs.shape) == tuple(gi.shape) == (Q, k)
    s = bg.biased_scores(S, off, probes, bias, None if w is None else w.cpu().numpy(), metric)
    want_s, want_i = lg.restate_lists(s, off, probes, k, keep)
    assert torch.equal(gi, torch.from_numpy(want_i).cuda()), "positions differ from rules 4, 13 and 21"
    assert torch.equal(_i32(gs), _i32(torch.from_numpy(want_s).cuda())), "scores differ from rule 21"

    # the bias decides something: some query with two lists differs from the call without one
    ps, pi = q._search_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d))
    two = bg.rows_with_two_lists(off, probes)
    if two:
        rows = torch.tensor(two, device="cuda")
        assert not (torch.equal(gi[rows], pi[rows]) and torch.equal(_i32(gs[rows]), _i32(ps[rows]))), "the bias changed nothing"
        print(f"[lists bias] {case.name} {metric} {pattern}: {int((gi[rows] != pi[rows]).any(dim=1).sum())} of {len(two)} rows "
              f"with two lists list other positions under the bias")

    # a second call: identical bytes; a float64 bias is narrowed to the same float32
    s2, i2 = q._search_scan(tables, flat_d, w, k, metric=metric, mask=None if keep_d is None else q.pack_mask(keep_d),
                            lists=(off_d, probes_d), bias=bias_d.to(torch.float64))
    assert torch.equal(_i32(gs), _i32(s2)) and torch.equal(gi, i2)

    # probe_bias == NULL through the new entry is the entry without a bias, bit for bit
    words = None if keep_d is None else q.pack_mask(keep_d)
    n_s, n_i = _direct(q, tables, flat_d, w, k, metric, words, off_d, probes_d, None, "mcq_search_scan_lists_bias")
    o_s, o_i = _direct(q, tables, flat_d, w, k, metric, words, off_d, probes_d, None, "mcq_search_scan_lists")
    assert torch.equal(n_i, o_i) and torch.equal(_i32(n_s), _i32(o_s)) and torch.equal(o_i, pi) and torch.equal(_i32(o_s), _i32(ps))
    d_s, d_i = _direct(q, tables, flat_d, w, k, metric, words, off_d, probes_d, bias_d, "mcq_search_scan_lists_bias")
    assert torch.equal(d_i, gi) and torch.equal(_i32(d_s), _i32(gs))


# ------------------------------------------------------------------ every cell of launch_lists with a bias, one N per test
_CELL = {}


def _cell(N):
    if _CELL.get("N") != N:
        _CELL.clear()
        case = sel.lists_case(N)
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, _ = base._queries(case, q, kept)
        tables, norms = q.search_tables(xq), q.code_norms(kept)
        off, probes = sel.lists_layout()
        S = mg.restate_sums(tables.cpu().numpy(), flat)
        _CELL.update(N=N, v=(case, q, flat, torch.from_numpy(flat).cuda(), tables, norms, q.rnorms_from_norms(norms), off, probes,
                             S, bg.bias_for(S, off, probes, SEED)))
    return _CELL["v"]


@pytest.mark.parametrize("N", bg.CELL_NS)
def test_every_cell_of_launch_lists_bias(N):
    case, q, flat, flat_d, tables, norms, rnorms, off, probes, S, bias = _cell(N)
    off_d, probes_d, bias_d = torch.from_numpy(off).cuda(), torch.from_numpy(probes).cuda(), torch.from_numpy(bias).cuda()
    keep, words = sel.mask_for(case.B)
    words_d = torch.from_numpy(words).cuda()
    for metric in bg.METRICS:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        s = bg.biased_scores(S, off, probes, bias, None if w is None else w.cpu().numpy(), metric)
        for masked in bg.CELL_MASKS:
            gs, gi = q._search_scan(tables, flat_d, w, case.k, metric=metric, mask=words_d if masked else None,
                                    lists=(off_d, probes_d), bias=bias_d)
            want_s, want_i = lg.restate_lists(s, off, probes, case.k, keep if masked else None)
            assert torch.equal(gi, torch.from_numpy(want_i).cuda()), (N, metric, masked)
            assert torch.equal(_i32(gs), _i32(torch.from_numpy(want_s).cuda())), (N, metric, masked)
            assert bool((gi >= 0).all())


def test_calls_without_a_candidate_read_no_bias():
    from quantization_amd._lib import McqError
    case = lg.CASES[1]
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = tl._prepared(case)
    k, Q = case.k, case.Q
    bias_d = torch.from_numpy(_sums(case)[1]).cuda()
    nan = torch.full_like(bias_d, float("nan"))
    none = [q._search_scan(tables, flat_d, norms, k, lists=(off_d, probes_d[:, :0]), bias=bias_d[:, :0]),          # P == 0
            q._search_scan(tables, flat_d, norms, k, lists=(off_d[:1], probes_d), bias=bias_d),                    # L == 0
            q._search_scan(tables, flat_d[:0], norms[:0], k, lists=(off_d, probes_d), bias=bias_d),                # B == 0
            q._search_scan(tables, flat_d, norms, k, lists=(off_d, torch.full_like(probes_d, -1)), bias=nan)]      # padding only
    for s, i in none:
        assert tuple(s.shape) == (Q, k) and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s > 0).all())
    # the value of a slot that names no list (or an empty one) is never read: NaN there changes nothing
    L = len(off) - 1
    unread = torch.from_numpy(np.array([[not (0 <= int(l) < L and off[int(l) + 1] > off[int(l)]) for l in row] for row in probes])).cuda()
    assert bool(unread.any())
    a = q._search_scan(tables, flat_d, norms, k, lists=(off_d, probes_d), bias=bias_d)
    b = q._search_scan(tables, flat_d, norms, k, lists=(off_d, probes_d), bias=torch.where(unread, nan, bias_d))
    assert torch.equal(a[1], b[1]) and torch.equal(_i32(a[0]), _i32(b[0]))
    with pytest.raises(McqError):
        q._search_scan(tables, flat_d, norms, k, lists=(off_d, probes_d), bias=bias_d.cpu())
    with pytest.raises(ValueError, match="probe_bias"):
        q._search_scan(tables, flat_d, norms, k, lists=(off_d, probes_d), bias=bias_d[:, :-1])
