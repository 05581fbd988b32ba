"""Every cell of the kernel-selection tables of the search over stored codes (launch_scan, launch_range, launch_lists of
quantization_amd/csrc/mcq_api.hip), launched once on the GPU and compared BIT FOR BIT with the numpy restatement of the
contract (include/mcq.h).  The cells, and what each reaches, are the table of tests/search_selection_grid.py;
tests/test_search_selection_host.py checks them against the pick<...> lists of the source and the mirrors of the launch
arithmetic.  No tolerance appears in this file: the restatement is tied to float64 by tests/test_gpu_search_metric_definition.py.

Per (QT, N) cell and per capped cell (one test each; the inputs are those of tests/test_gpu_search.py for a decode-only state
and random codes):
  scan    k_search_scan<QT, N, M, MASKED>: the three metrics, each without a mask and under the mask of the grid (about half
          the bits, one whole word zero inside a slice, the bits past B of the last word set: rule 10 ignores them), scores as
          uint32 and positions against search_grid.restate (L2), search_metric_grid.restate_metric (the other two) and
          search_mask_grid.compact_topk (rule 11).  Then one metric (it rotates with the cell) under a mask of k - 1
          candidates: the tail is (+inf, -1), rule 4.
  sweeps  k_range_sweep<QT, CH, FILL, MASKED>: the metric is a runtime value there, so one per cell, rotating; without and
          under the mask; each query's threshold is its 10th smallest restated score (among the candidates), so that the
          inclusive comparison of rule 7 decides a real borderline candidate; lims, scores and positions against
          search_range_grid.restate and search_mask_grid.restate_range_masked.  A call runs the count and the fill.
Per N (one test each): k_search_lists<N, M, MASKED>, three metrics x mask or none, against search_lists_grid.restate_lists and,
per rule 14, against row 0 of the masked scan called with the union mask of each query."""
import numpy as np
import pytest
import torch

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg
import search_selection_grid as ss
import test_gpu_search as base

pytestmark = pytest.mark.gpu

_STORES = {}


def _store(case):
    """the quantizer, the store and its per-candidate arrays: shared by the cells of one N x K (they differ in Q alone)"""
    key = (case.N, case.K, case.B)
    if key not in _STORES:
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        norms = q.code_norms(kept)
        rnorms = q.rnorms_from_norms(norms)
        _STORES[key] = (q, flat, torch.from_numpy(flat).cuda(), {"l2": norms, "ip": None, "cosine": rnorms},
                        {"l2": norms.cpu().numpy(), "ip": None, "cosine": rnorms.cpu().numpy()})
    return _STORES[key]


def _inputs(case):
    q, flat, flat_d, w_d, w_h = _store(case)
    xq, _ = base._queries(case, q, None)
    tables = q.search_tables(xq)
    assert tables.dtype == torch.float32 and tuple(tables.shape) == (case.Q, case.N, case.K)
    return q, flat, flat_d, w_d, w_h, tables, tables.cpu().numpy()


def _same_lists(got, want, what):
    (gs, gi), (want_s, want_i) = got, want
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    assert gs.dtype == np.float32 and gi.dtype == np.int64 and gs.shape == gi.shape == want_i.shape
    assert np.array_equal(gi, want_i), f"{what}: positions differ from rule 4 in rows {np.flatnonzero((gi != want_i).any(1))[:8]}"
    assert np.array_equal(gs.view(np.uint32), want_s.view(np.uint32)), f"{what}: scores differ from rule 3"
    tail = want_i == -1
    assert (gi[tail] == -1).all() and np.isposinf(gs[tail]).all(), f"{what}: the tail is not (+inf, -1)"
    return int(tail.sum())


@pytest.mark.parametrize("cell", ss.CELLS, ids=lambda c: c.name)
def test_scan_and_sweep_cell(cell):
    case, at = cell.case(), ss.CELLS.index(cell)
    q, flat, flat_d, w_d, w_h, tables, T = _inputs(case)
    B, k, Q = cell.B, cell.k, cell.Q
    keep, words = ss.mask_for(B)
    words_d = torch.from_numpy(words).cuda()

    # the scan: <QT, N> x three metrics x mask or none
    for metric in ss.METRICS:
        w, wh = w_d[metric], w_h[metric]
        want = sg.restate(T, wh, flat, k) if metric == "l2" else mg.restate_metric(T, wh, flat, k, metric)
        assert _same_lists(q._search_scan(tables, flat_d, w, k, metric=metric), want, f"{cell.name} {metric}") == 0
        want = kg.compact_topk(T, wh, flat, k, metric, keep)
        got = q._search_scan(tables, flat_d, w, k, metric=metric, mask=words_d)
        assert _same_lists(got, want, f"{cell.name} {metric} masked") == 0
        assert bool(torch.from_numpy(keep).cuda()[got[1]].all())
    metric = ss.METRICS[at % 3]
    few, few_words = ss.few_for(B)
    got = q._search_scan(tables, flat_d, w_d[metric], k, metric=metric, mask=torch.from_numpy(few_words).cuda())
    assert _same_lists(got, kg.compact_topk(T, w_h[metric], flat, k, metric, few), f"{cell.name} {metric} few") == Q

    # the sweeps: <QT, CH, FILL, MASKED>, count and fill in one call
    s = mg.restate_metric_scores(T, w_h[metric], flat, metric)
    for masked in (False, True):
        top_s, _ = kg.restate_topk_masked(s, keep, k) if masked else sg.restate_topk(s, k)
        thr = np.ascontiguousarray(top_s[:, k - 1])
        assert np.isfinite(thr).all()
        if masked:
            want_lims, want_pos, want_val = kg.restate_range_masked(s, keep, thr)
        else:
            _, want_lims, want_pos, want_val = rg.restate(T, w_h[metric], flat, metric, thr=thr)
        assert (np.diff(want_lims) >= k).all() and want_lims[-1] < Q * B // 4          # the borderline candidate is listed
        lims, val, pos = q._search_range(tables, flat_d, w_d[metric], torch.from_numpy(thr).cuda(), metric,
                                         mask=words_d if masked else None)
        what = f"{cell.name} {metric} sweep{' masked' if masked else ''}"
        assert lims.dtype == torch.int64 and pos.dtype == torch.int64 and val.dtype == torch.float32
        assert np.array_equal(lims.cpu().numpy(), want_lims), f"{what}: lims differ from rules 7 and 8"
        assert np.array_equal(pos.cpu().numpy(), want_pos), f"{what}: positions differ from rule 8"
        assert np.array_equal(val.cpu().numpy().view(np.uint32), want_val.view(np.uint32)), f"{what}: scores differ from rule 3'"


@pytest.mark.parametrize("N", ss.NS)
def test_lists_cell(N):
    case = ss.lists_case(N)
    q, flat, flat_d, w_d, w_h, tables, T = _inputs(case)
    B, k, Q = case.B, case.k, case.Q
    off, probes = ss.lists_layout()
    off_d, probes_d = torch.from_numpy(off).cuda(), torch.from_numpy(probes).cuda()
    keep, words = ss.mask_for(B)
    words_d = torch.from_numpy(words).cuda()
    for metric in ss.METRICS:
        w = w_d[metric]
        s = mg.restate_metric_scores(T, w_h[metric], flat, metric)
        for masked in (False, True):
            what = f"lists {N} x {case.K} {metric}{' masked' if masked else ''}"
            gs, gi = q._search_scan(tables, flat_d, w, k, metric=metric, mask=words_d if masked else None, lists=(off_d, probes_d))
            assert _same_lists((gs, gi), lg.restate_lists(s, off, probes, k, keep if masked else None), what) == 0
            # rule 14: row 0 of the masked scan with this one query and the union mask of its lists
            for j in range(Q):
                union = torch.from_numpy(lg.union_mask(off, probes[j], B, keep if masked else None)).cuda()
                ms, mi = q._search_scan(tables[j:j + 1], flat_d, w, k, metric=metric, mask=union)
                assert torch.equal(mi[0], gi[j]) and torch.equal(ms[0].view(torch.int32), gs[j].view(torch.int32)), \
                    f"{what}: query {j} differs from mcq_search_scan_masked under the union mask"
