"""The search list by list on the GPU (mcq_search_scan_lists through Quantizer._search_scan(lists=...), Quantizer.search_lists;
include/mcq.h rules 13-16), BIT FOR BIT against the numpy restatement of tests/search_lists_grid.py and against the existing
scans.

Per case of its table x metric x mask (none, `half`, `sparse` of tests/search_mask_grid.py):
  * scores (as uint32) and positions of EVERY query equal the restatement formed from the tables and the per-candidate array
    the device returned;
  * the first queries equal row 0 of mcq_search_scan_masked with that one query and the union mask of its lists (rule 14);
  * with every list probed, each row scrambled in its own way, and lists that cover the store, every query equals the scan
    of the whole store (mcq_search_scan_metric, or mcq_search_scan_masked under the mask);
  * a second call returns identical bytes.
Then the calls that have no candidate anywhere, the public call against Quantizer.search(mask=union) per query, and
build_lists + probe_lists end to end."""
import numpy as np
import pytest
import torch

import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import test_gpu_search as base

pytestmark = pytest.mark.gpu

RULE14 = 3                          # queries per case checked against the masked scan, one call each
SEED = 1
_CACHE = {}


def _i32(t):
    return t.view(torch.int32)


def _prepared(case):
    """the store, the queries, the lists and what the device made of them, shared by the metrics and masks of one case"""
    if _CACHE.get("name") != case.name:
        _CACHE.clear()
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, _ = base._queries(case, q, kept)
        tables, norms = q.search_tables(xq), q.code_norms(kept)
        off, probes = lg.layout(case)
        _CACHE.update(name=case.name, metric={},
                      v=(q, kept, flat, torch.from_numpy(flat).cuda(), xq, tables, norms, q.rnorms_from_norms(norms), off, probes,
                         torch.from_numpy(off).cuda(), torch.from_numpy(probes).cuda()))
    return _CACHE["v"]


def _per_metric(case, metric):
    """(w, the scores of the whole store for every query): once per (case, metric)"""
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)[:8]
    if metric not in _CACHE["metric"]:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        s = mg.restate_metric_scores(tables.cpu().numpy(), None if w is None else w.cpu().numpy(), flat, metric)
        _CACHE["metric"][metric] = (w, s)
    return _CACHE["metric"][metric]


@pytest.mark.parametrize("pattern", lg.PATTERNS, ids=lambda p: p or "nomask")
@pytest.mark.parametrize("metric", lg.METRICS)
@pytest.mark.parametrize("case", lg.CASES, ids=lambda c: c.name)
def test_lists_case(case, metric, pattern):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    w, s = _per_metric(case, metric)
    Q, B, k = case.Q, case.B, case.k
    keep = None if pattern is None else kg.keep_for(pattern, B, SEED, k)
    keep_d = None if keep is None else torch.from_numpy(keep).cuda()

    gs, gi = q._search_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, probes_d))
    assert gs.dtype == torch.float32 and gi.dtype == torch.int64 and tuple(gs.shape) == tuple(gi.shape) == (Q, k)
    want_s, want_i = lg.restate_lists(s, off, probes, k, keep)
    n_cand = [len(lg.candidates(off, row, keep)) for row in probes]
    print(f"[lists] {case.name} {metric} {pattern}: candidates per query {min(n_cand)} .. {max(n_cand)} of {B}")
    assert torch.equal(gi, torch.from_numpy(want_i).cuda()), "positions differ from rules 4, 13 and 14"
    assert torch.equal(_i32(gs), _i32(torch.from_numpy(want_s).cuda())), "scores differ from rule 3'"

    # a second call: identical bytes; packed mask words are the bool mask
    s2, i2 = q._search_scan(tables, flat_d, w, k, metric=metric, mask=None if keep_d is None else q.pack_mask(keep_d),
                            lists=(off_d, probes_d))
    assert torch.equal(_i32(gs), _i32(s2)) and torch.equal(gi, i2)

    # rule 14: row 0 of the masked scan with this one query and the union mask of its lists
    for j in range(min(Q, RULE14)):
        union = torch.from_numpy(lg.union_mask(off, probes[j], B, keep)).cuda()
        ms, mi = q._search_scan(tables[j:j + 1], flat_d, w, k, metric=metric, mask=union)
        assert torch.equal(mi[0], gi[j]) and torch.equal(_i32(ms[0]), _i32(gs[j])), (j, "differs from mcq_search_scan_masked")

    # every list probed, in scrambled order, over lists that cover the store: the scan of the whole store
    if case.covering:
        every = torch.from_numpy(lg.all_probes(case, len(off) - 1)).cuda()
        a_s, a_i = q._search_scan(tables, flat_d, w, k, metric=metric, mask=keep_d, lists=(off_d, every))
        u_s, u_i = q._search_scan(tables, flat_d, w, k, metric=metric, mask=keep_d)
        assert torch.equal(a_i, u_i) and torch.equal(_i32(a_s), _i32(u_s)), "all lists probed differs from the scan"


@pytest.mark.parametrize("metric", lg.METRICS)
def test_public_call_against_search_under_the_union_mask(metric):
    case = lg.CASES[1]
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    k = case.k
    for keep in (None, kg.keep_for("half", case.B, SEED, k)):
        keep_d = None if keep is None else torch.from_numpy(keep).cuda()
        val, idx = q.search_lists(xq, kept, off_d, probes_d, k=k, norms=norms, metric=metric, rnorms=rnorms, mask=keep_d)
        assert tuple(val.shape) == tuple(idx.shape) == (case.Q, k) and idx.dtype == torch.int64
        wide = q.search_lists(xq.reshape(1, case.Q, case.D), kept, off_d, probes_d.to(torch.int64).reshape(1, case.Q, case.P), k=k,
                              metric=metric, mask=keep_d)             # leading dimensions, int64 probes, norms formed by the call
        assert tuple(wide[0].shape) == (1, case.Q, k) and torch.equal(wide[1][0], idx) and torch.equal(_i32(wide[0][0]), _i32(val))
        for j in range(5):
            union = torch.from_numpy(lg.union_mask(off, probes[j], case.B, keep)).cuda()
            u_val, u_idx = q.search(xq[j:j + 1], kept, k=k, norms=norms, metric=metric, rnorms=rnorms, mask=union)
            assert torch.equal(u_idx[0], idx[j]) and torch.equal(_i32(u_val[0]), _i32(val[j])), j
    # an int64 entry past the int32 range names no list
    far = probes_d.to(torch.int64)
    far[far < 0] = 1 << 40
    v2, i2 = q.search_lists(xq, kept, off_d, far, k=k, norms=norms, metric=metric, rnorms=rnorms)
    v1, i1 = q.search_lists(xq, kept, off_d, probes_d, k=k, norms=norms, metric=metric, rnorms=rnorms)
    assert torch.equal(i1, i2) and torch.equal(_i32(v1), _i32(v2))


def test_calls_without_a_candidate_fill_the_outputs():
    from quantization_amd._lib import McqError
    case = lg.CASES[1]
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    k, Q = case.k, case.Q
    none = [q._search_scan(tables, flat_d, norms, k, lists=(off_d, probes_d[:, :0])),                      # P == 0
            q._search_scan(tables, flat_d, norms, k, lists=(off_d[:1], probes_d)),                         # L == 0
            q._search_scan(tables, flat_d[:0], norms[:0], k, lists=(off_d, probes_d)),                     # B == 0
            q._search_scan(tables, flat_d, norms, k, lists=(off_d, torch.full_like(probes_d, -1)))]        # padding only
    for s, i in none:
        assert tuple(s.shape) == (Q, k) and bool((i == -1).all()) and bool(torch.isinf(s).all()) and bool((s > 0).all())
    val, idx = q.search_lists(xq, kept, off_d, torch.full_like(probes_d, -1), k=k, metric="ip")
    assert bool((idx == -1).all()) and bool(torch.isinf(val).all()) and bool((val < 0).all())              # similarities: -inf
    with pytest.raises(McqError, match="unsupported"):
        q._search_scan(tables, flat_d, norms, k, lists=(off_d, torch.zeros(Q, 4097, dtype=torch.int32, device="cuda")))
    with pytest.raises(McqError):
        q.search_lists(xq, kept, off_d.cpu(), probes_d)
    with pytest.raises(ValueError):
        q.search_lists(xq, kept, off_d, probes_d[:-1])


@pytest.mark.parametrize("metric", lg.METRICS)
def test_build_lists_and_probe_lists_end_to_end(metric):
    from quantization_amd import build_lists, probe_lists
    case = lg.CASES[2]                                       # 8 x 256, 20,000 encoded vectors
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)[:8]
    B, k, nl = case.B, case.k, 48
    with torch.no_grad():
        cen = q.decode(kept[torch.from_numpy(np.random.RandomState(5).choice(B, nl, replace=False)).cuda()])
        x = q.decode(kept)
        assign = torch.cdist(x, cen).argmin(dim=1)
    order, off = build_lists(assign, nl)
    assert bool((assign[order][1:] >= assign[order][:-1]).all()) and int(off[-1]) == B
    store, n_o, r_o = kept[order].contiguous(), norms[order].contiguous(), rnorms[order].contiguous()
    full_val, full_idx = q.search(xq, kept, k=k, norms=norms, metric=metric, rnorms=rnorms)
    hits = {}
    for nprobe in (1, 4, nl):
        probes = probe_lists(xq, cen, nprobe, metric=metric)
        assert probes.dtype == torch.int32 and tuple(probes.shape) == (case.Q, nprobe) and probes.is_cuda
        val, idx = q.search_lists(xq, store, off, probes, k=k, norms=n_o, metric=metric, rnorms=r_o)
        off_h, probes_h = off.cpu().numpy(), probes.cpu().numpy()
        for j in range(3):
            union = torch.from_numpy(lg.union_mask(off_h, probes_h[j], B)).cuda()
            u_val, u_idx = q.search(xq[j:j + 1], store, k=k, norms=n_o, metric=metric, rnorms=r_o, mask=union)
            assert torch.equal(u_idx[0], idx[j]) and torch.equal(_i32(u_val[0]), _i32(val[j]))
        back = torch.where(idx >= 0, order[idx.clamp(min=0)], idx)
        hits[nprobe] = float((back[:, :, None] == full_idx[:, None, :]).any(dim=2).float().mean())
        if nprobe == nl:                                     # every list: the search of the whole store, mapped back through order
            assert torch.equal(_i32(val), _i32(full_val))
            distinct = (val[:, 1:] != val[:, :-1]).all(dim=1)
            assert torch.equal(back[distinct], full_idx[distinct])
    print(f"[lists] {metric}: recall@{k} against the whole store by nprobe: {hits}")
    assert hits[nl] >= hits[4] >= hits[1] and hits[nl] > 0.999
