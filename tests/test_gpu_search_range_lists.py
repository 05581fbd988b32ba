"""The range search list by list on the GPU (mcq_search_range_lists_count / _fill through Quantizer._search_range(lists=...),
Quantizer.range_search_lists; include/mcq.h rules 17-20), BIT FOR BIT against the numpy restatement of
tests/search_range_lists_grid.py and against the existing range searches.

Per case of its table x metric x mask (none, `half`, `sparse` of tests/search_mask_grid.py), with the thresholds of the grid:
  * lims, positions and scores (as int32) equal the restatement formed from the tables and the per-candidate array the
    device returned; a second call returns identical bytes, and packed mask words give what the bool mask gave;
  * rule 18, ascending rows: the first queries with their row sorted equal mcq_search_range_count_masked / _fill_masked
    called with that one query and the union mask of its lists;
  * rule 18, covering lists: with every list named ascending the result is the range search of the whole store;
  * scrambled rows: every list named in an order of the row's own returns the same set of hits, list by list in the row's
    order and ascending inside each list;
  * a fill with half the room stores the first half and nothing else.
Then the empty calls, max_results, the public call against Quantizer.range_search(mask=union), the top-k search list by list
as a prefix, and build_lists + probe_lists end to end."""
import numpy as np
import pytest
import torch

import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_lists_grid as rl
import test_gpu_search as base

pytestmark = pytest.mark.gpu

RULE18 = 3                          # queries per case checked against the masked range search, one call each
SEED = 1
SENTINEL_S, SENTINEL_I = -12345.5, -777
_CACHE = {}


def _i32(t):
    return t.view(torch.int32)


def _same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(_i32(a[1]), _i32(b[1]))


def _prepared(case):
    """the store, the queries, the lists and what the device made of them, shared by the metrics and masks of one case"""
    if _CACHE.get("name") != case.name:
        _CACHE.clear()
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, _ = base._queries(case, q, kept)
        tables, norms = q.search_tables(xq), q.code_norms(kept)
        off, probes = rl.layout(case)
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


def _check(got, want, what):
    lims, pos, val = want
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.float32 and got[2].dtype == torch.int64
    assert torch.equal(got[0], torch.from_numpy(lims).cuda()), f"{what}: lims differ from rules 17 and 18"
    assert torch.equal(got[2], torch.from_numpy(pos).cuda()), f"{what}: positions differ from rules 17 and 18"
    assert torch.equal(_i32(got[1]), _i32(torch.from_numpy(val).cuda())), f"{what}: scores differ from rule 3'"


def _direct_fill(q, tables, flat_d, w, metric, words, off_d, probes_d, thr_d, capacity, room):
    """count, then fill with `capacity` into buffers of `room` slots preset to the sentinels -> (lims, scores, positions)"""
    from quantization_amd import _lib
    L = _lib.lib()
    Q, B, N, K, P = tables.shape[0], flat_d.shape[0], q.num_codebooks, q.codebook_size, probes_d.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.empty(L.mcq_search_range_lists_workspace_bytes(Q, P, N, K), dtype=torch.uint8, device="cuda")
    lims = torch.empty(Q + 1, dtype=torch.int64, device="cuda")
    out_s = torch.full((room,), SENTINEL_S, dtype=torch.float32, device="cuda")
    out_i = torch.full((room,), SENTINEL_I, dtype=torch.int64, device="cuda")
    args = (tables.data_ptr(), Q, flat_d.data_ptr(), None if w is None else w.data_ptr(), B, N, K, q._METRICS[metric],
            None if words is None else words.data_ptr(), off_d.data_ptr(), off_d.numel() - 1, probes_d.data_ptr(), P, thr_d.data_ptr(),
            lims.data_ptr())
    assert L.mcq_search_range_lists_count(*args, ws.data_ptr(), ws.numel(), st) == 0
    assert L.mcq_search_range_lists_fill(*args, out_s.data_ptr(), out_i.data_ptr(), capacity, ws.data_ptr(), ws.numel(), st) == 0
    torch.cuda.synchronize()
    return lims, out_s, out_i


@pytest.mark.parametrize("pattern", rl.PATTERNS, ids=lambda p: p or "nomask")
@pytest.mark.parametrize("metric", rl.METRICS)
@pytest.mark.parametrize("case", rl.CASES, ids=lambda c: c.name)
def test_range_lists_case(case, metric, pattern):
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    w, s = _per_metric(case, metric)
    Q, B, L = case.Q, case.B, len(off) - 1
    keep = None if pattern is None else kg.keep_for(pattern, B, SEED, case.k)
    keep_d = None if keep is None else torch.from_numpy(keep).cuda()
    tables, flat_d = tables.contiguous(), flat_d.contiguous()

    for shift in ((0, 4) if Q == 1 else (0,)):               # (the one query of a case lists nothing at shift 0: -inf)
        thr = rl.thresholds_for(s, off, probes, keep, shift)
        thr_d = torch.from_numpy(thr).cuda()
        got = q._search_range(tables, flat_d, w, thr_d, metric, mask=keep_d, lists=(off_d, probes_d))
        want = rl.restate_range_lists(s, off, probes, thr, keep)
        n = np.diff(want[0])
        print(f"[range lists] {case.name} {metric} {pattern} shift {shift}: listed per query {n.min()} .. {n.max()}, {want[0][-1]} in all")
        _check(got, want, "the call")
        # a second call: identical bytes; packed mask words are the bool mask
        again = q._search_range(tables, flat_d, w, thr_d, metric, mask=None if keep_d is None else q.pack_mask(keep_d),
                                lists=(off_d, probes_d))
        assert _same(got, again)

    # rule 18: an ascending row equals the masked range search of that one query under the union mask of its lists
    asc = rl.sorted_rows(probes, L)
    asc_d = torch.from_numpy(asc).cuda()
    head = min(Q, RULE18)
    a = q._search_range(tables[:head], flat_d, w, thr_d[:head], metric, mask=keep_d, lists=(off_d, asc_d[:head]))
    for j in range(head):
        if not rl.distinct(off, asc[j]):
            continue
        union = torch.from_numpy(lg.union_mask(off, asc[j], B, keep)).cuda()
        u = q._search_range(tables[j:j + 1], flat_d, w, thr_d[j:j + 1], metric, mask=union)
        lo, hi = int(a[0][j]), int(a[0][j + 1])
        assert hi - lo == int(u[0][1]) and torch.equal(a[2][lo:hi], u[2]) and torch.equal(_i32(a[1][lo:hi]), _i32(u[1])), \
            (j, "differs from mcq_search_range_count_masked / _fill_masked")

    # every list named: ascending (over covering lists the range search of the whole store), and scrambled row by row
    every = torch.from_numpy(rl.all_ascending(case, L)).cuda()
    e = q._search_range(tables, flat_d, w, thr_d, metric, mask=keep_d, lists=(off_d, every))
    if case.covering:
        assert _same(e, q._search_range(tables, flat_d, w, thr_d, metric, mask=keep_d)), "all lists named differs from the sweep"
    scr = lg.all_probes(case, L)
    g = q._search_range(tables, flat_d, w, thr_d, metric, mask=keep_d, lists=(off_d, torch.from_numpy(scr).cuda()))
    assert torch.equal(g[0], e[0])
    g_l, g_s, g_i, e_s, e_i = g[0].cpu().numpy(), _i32(g[1]).cpu().numpy(), g[2].cpu().numpy(), _i32(e[1]).cpu().numpy(), e[2].cpu().numpy()
    for j in range(Q):
        lo, hi = g_l[j], g_l[j + 1]
        order = np.argsort(g_i[lo:hi], kind="stable")
        assert np.array_equal(g_i[lo:hi][order], e_i[lo:hi]) and np.array_equal(g_s[lo:hi][order], e_s[lo:hi]), (j, "another set of hits")
        rank = np.empty(L, dtype=np.int64)
        rank[scr[j]] = np.arange(L)
        of = np.searchsorted(off, g_i[lo:hi], side="right") - 1
        key = rank[of] * (B + 1) + g_i[lo:hi]                # the row's order of the lists, ascending position inside one
        assert (np.diff(key) > 0).all(), (j, "not list by list in the row's order")

    # a fill with half the room: the first half is right and nothing else is written
    total = int(got[0][-1])
    cap = total // 2
    words = None if keep_d is None else q.pack_mask(keep_d)
    lims, out_s, out_i = _direct_fill(q, tables, flat_d, w, metric, words, off_d, probes_d, thr_d, cap, total + 64)
    assert torch.equal(lims, got[0])
    assert torch.equal(out_i[:cap], got[2][:cap]) and torch.equal(_i32(out_s[:cap]), _i32(got[1][:cap]))
    assert bool((out_i[cap:] == SENTINEL_I).all()) and bool((out_s[cap:] == SENTINEL_S).all()), "stored past the capacity"


def test_calls_without_a_candidate_give_zero_lims():
    from quantization_amd._lib import McqError
    case = rl.CASES[1]
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    Q = case.Q
    thr = torch.full((Q,), float("inf"), device="cuda")
    none = [q._search_range(tables, flat_d, norms, thr, lists=(off_d, probes_d[:, :0])),                    # P == 0
            q._search_range(tables, flat_d, norms, thr, lists=(off_d[:1], probes_d)),                       # L == 0
            q._search_range(tables, flat_d[:0], norms[:0], thr, lists=(off_d, probes_d)),                   # B == 0
            q._search_range(tables[:0], flat_d, norms, thr[:0], lists=(off_d, probes_d[:0])),               # Q == 0
            q._search_range(tables, flat_d, norms, thr, lists=(off_d, torch.full_like(probes_d, -1)))]      # padding only
    for lims, s, i in none:
        assert lims.numel() in (Q + 1, 1) and not bool(lims.any()) and s.numel() == 0 and i.numel() == 0
    lims, val, idx = q.range_search_lists(xq, kept, off_d, torch.full_like(probes_d, -1), 1e30, metric="ip")
    assert not bool(lims.any()) and val.numel() == 0
    with pytest.raises(McqError, match="unsupported"):
        q._search_range(tables, flat_d, norms, thr, lists=(off_d, torch.zeros(Q, 4097, dtype=torch.int32, device="cuda")))
    with pytest.raises(McqError):
        q.range_search_lists(xq, kept, off_d.cpu(), probes_d, 1.0)
    with pytest.raises(ValueError):
        q.range_search_lists(xq, kept, off_d, probes_d[:-1], 1.0)


def test_max_results_names_the_count():
    from quantization_amd._lib import McqError
    case = rl.CASES[1]
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    thr = torch.full((case.Q,), float("inf"), device="cuda")
    total = int(q._search_range(tables, flat_d, norms, thr, lists=(off_d, probes_d))[0][-1])
    assert total == sum(len(rl.row_positions(off, row)) for row in probes) > 10
    assert int(q._search_range(tables, flat_d, norms, thr, max_results=total, lists=(off_d, probes_d))[0][-1]) == total
    with pytest.raises(McqError, match=str(total)):
        q._search_range(tables, flat_d, norms, thr, max_results=total - 1, lists=(off_d, probes_d))
    with pytest.raises(McqError, match=str(total)):
        q.range_search_lists(xq, kept, off_d, probes_d, 1e30, norms=norms, max_results=total - 1)


@pytest.mark.parametrize("metric", rl.METRICS)
def test_public_call_against_range_search_under_the_union_mask(metric):
    case = rl.CASES[1]
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    Q, B, L = case.Q, case.B, len(off) - 1
    xq = xq.clone()
    xq[3] = 0                                                # a zero query: under the cosine every similarity is 0
    # radii per query: the 40th value of the top-k search list by list (the 40 nearest of its lists, and their ties)
    val40 = q.search_lists(xq, kept, off_d, probes_d, k=40, norms=norms, metric=metric, rnorms=rnorms)[0][:, 39]
    radius = torch.where(torch.isfinite(val40), val40, torch.zeros_like(val40))
    for keep in (None, kg.keep_for("half", B, SEED, case.k)):
        keep_d = None if keep is None else torch.from_numpy(keep).cuda()
        lims, val, idx = q.range_search_lists(xq, kept, off_d, probes_d, radius, norms=norms, metric=metric, rnorms=rnorms, mask=keep_d)
        assert tuple(lims.shape) == (Q + 1,) and lims.dtype == idx.dtype == torch.int64 and val.dtype == torch.float32
        assert int(lims[-1]) == val.numel() == idx.numel() > 0
        # leading dimensions on queries and probes, int64 probes with an entry past int32, norms formed by the call
        far = probes_d.to(torch.int64)
        far[far < 0] = 1 << 40
        wide = q.range_search_lists(xq.reshape(1, Q, case.D), kept, off_d, far.reshape(1, Q, case.P), radius, metric=metric, mask=keep_d)
        assert _same((lims, val, idx), wide)
        for j in range(5):
            union = torch.from_numpy(lg.union_mask(off, probes[j], B, keep)).cuda()
            u = q.range_search(xq[j:j + 1], kept, radius[j:j + 1], norms=norms, metric=metric, rnorms=rnorms, mask=union)
            lo, hi = int(lims[j]), int(lims[j + 1])
            assert hi - lo == int(u[0][1]) and torch.equal(idx[lo:hi], u[2]) and torch.equal(_i32(val[lo:hi]), _i32(u[1])), j
            mine = idx[lo:hi]
            assert bool((mine[1:] > mine[:-1]).all())                            # ascending position, whatever the row's order
        # a float radius is the tensor of that value
        r0 = float(radius[1])
        one = q.range_search_lists(xq, kept, off_d, probes_d, r0, norms=norms, metric=metric, rnorms=rnorms, mask=keep_d)
        assert _same(one, q.range_search_lists(xq, kept, off_d, probes_d, torch.full((Q,), r0, device="cuda"), norms=norms,
                                               metric=metric, rnorms=rnorms, mask=keep_d))
    if metric == "cosine":                                   # the zero query: everything it probes at radius <= 0, else nothing
        n3 = len(lg.candidates(off, probes[3]))
        assert n3 > 0
        for r, n in ((0.0, n3), (-0.5, n3), (1e-6, 0)):
            lims = q.range_search_lists(xq, kept, off_d, probes_d, r, rnorms=rnorms, metric="cosine")[0]
            assert int(lims[4] - lims[3]) == n, (r, n)


@pytest.mark.parametrize("metric", rl.METRICS)
def test_the_top_k_list_by_list_is_a_prefix(metric):
    case = rl.CASES[2]                                       # 8 x 256, 20,000 encoded vectors, k = 10
    q, kept, flat, flat_d, xq, tables, norms, rnorms, off, probes, off_d, probes_d = _prepared(case)
    w, _ = _per_metric(case, metric)
    k = case.k
    ts, ti = q._search_scan(tables, flat_d, w, k, metric=metric, lists=(off_d, probes_d))
    assert bool((ti >= 0).all())
    lims, s, i = q._search_range(tables, flat_d, w, ts[:, k - 1].contiguous(), metric, lists=(off_d, probes_d))
    lims, s, i = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy()
    for j in range(case.Q):
        lo, hi = lims[j], lims[j + 1]
        assert hi - lo >= k
        order = np.lexsort((i[lo:hi], s[lo:hi]))[:k]         # by (score, position)
        assert np.array_equal(i[lo:hi][order], ti[j].cpu().numpy())
        assert np.array_equal(s[lo:hi][order].view(np.int32), ts[j].cpu().numpy().view(np.int32))


@pytest.mark.parametrize("metric", rl.METRICS)
def test_build_lists_and_probe_lists_end_to_end(metric):
    from quantization_amd import build_lists, probe_lists
    case = rl.CASES[2]                                       # 8 x 256, 20,000 encoded vectors
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)[:8]
    B, Q, nl = case.B, case.Q, 48
    with torch.no_grad():
        cen = q.decode(kept[torch.from_numpy(np.random.RandomState(5).choice(B, nl, replace=False)).cuda()])
        assign = torch.cdist(q.decode(kept), cen).argmin(dim=1)
    order, off = build_lists(assign, nl)
    store, n_o, r_o = kept[order].contiguous(), norms[order].contiguous(), rnorms[order].contiguous()
    radius = q.search(xq, kept, k=50, norms=norms, metric=metric, rnorms=rnorms)[0][:, 49].contiguous()
    f_lims, f_val, f_idx = q.range_search(xq, kept, radius, norms=norms, metric=metric, rnorms=rnorms)
    assert int(f_lims[-1]) > 10 * Q                          # (about 50 per query; the rounding of |q|^2 may drop the 50th)
    listed = {}
    for nprobe in (4, nl):
        probes = probe_lists(xq, cen, nprobe, metric=metric)
        lims, val, idx = q.range_search_lists(xq, store, off, probes, radius, norms=n_o, metric=metric, rnorms=r_o)
        listed[nprobe] = int(lims[-1])
        off_h, probes_h = off.cpu().numpy(), probes.cpu().numpy()
        for j in range(3):
            union = torch.from_numpy(lg.union_mask(off_h, probes_h[j], B)).cuda()
            u = q.range_search(xq[j:j + 1], store, radius[j:j + 1], norms=n_o, metric=metric, rnorms=r_o, mask=union)
            lo, hi = int(lims[j]), int(lims[j + 1])
            assert hi - lo == int(u[0][1]) and torch.equal(idx[lo:hi], u[2]) and torch.equal(_i32(val[lo:hi]), _i32(u[1]))
        if nprobe == nl:                                     # every list: the range search of the unordered store, as a set
            assert torch.equal(lims, f_lims)
            back = order[idx]
            for j in range(Q):
                lo, hi = int(lims[j]), int(lims[j + 1])
                by = torch.argsort(back[lo:hi])
                assert torch.equal(back[lo:hi][by], f_idx[lo:hi]) and torch.equal(_i32(val[lo:hi][by]), _i32(f_val[lo:hi])), j
    print(f"[range lists] {metric}: listed by nprobe {listed} of {int(f_lims[-1])}")
    assert 0 < listed[4] <= listed[nl] == int(f_lims[-1])
