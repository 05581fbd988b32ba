"""The search over stored codes under a mask on the GPU (Quantizer.pack_mask, search(mask=...), range_search(mask=...);
include/mcq.h rules 10-12), BIT FOR BIT against the numpy restatement of tests/search_mask_grid.py and against the existing
unmasked search over the compacted store.

Per case of its table x mask pattern x metric, for the top-k scan and for the range search, with the mask handed in as packed
words and as a bool tensor (packed by mcq_search_pack_mask):
  * scores (as uint32), positions and lims EQUAL the restatement formed from the tables and the per-candidate array the device
    returned.  At most RESTATED queries of a case are restated (all of them except in the case of 200 queries, where they are
    spread over its tiles); the long-run case is not restated at all;
  * for EVERY query they equal the unmasked _search_scan / _search_range over codes[keep], w[keep] with positions mapped
    through nonzero(keep) (rule 11);
  * pattern `all` equals the call without a mask (rule 12).
The thresholds of the range search are inputs, taken per query (by q mod 4) from the unmasked top-k of the whole store: its k-th
score (a score that occurs), -inf, +inf, its score of rank (k + 1) // 2.
Then pack_mask against numpy.packbits, NaN behind cleared bits, and the public calls."""
import numpy as np
import pytest
import torch

import search_mask_grid as kg
import search_metric_grid as mg
import test_gpu_search as base

pytestmark = pytest.mark.gpu

RESTATED = 24
SEED = 1
_CACHE = {}


def _i32(t):
    return t.view(torch.int32)


def _prepared(case):
    """the store, the queries and what the device made of them, shared by the patterns and metrics of one case"""
    if _CACHE.get("name") != case.name:
        _CACHE.clear()
        q = base._quantizer(case)
        kept, flat = base._store(case, q)
        xq, _ = base._queries(case, q, kept)
        tables, norms = q.search_tables(xq), q.code_norms(kept)
        _CACHE.update(name=case.name, v=(q, kept, flat, torch.from_numpy(flat).cuda(), xq, tables, norms, q.rnorms_from_norms(norms)),
                      metric={})
    return _CACHE["v"]


def _per_metric(case, metric):
    """(w, restated rows, their scores of the whole store or None, thresholds on the device): once per (case, metric)"""
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)
    if metric not in _CACHE["metric"]:
        w = None if metric == "ip" else (norms if metric == "l2" else rnorms)
        rows = np.unique(np.linspace(0, case.Q - 1, min(case.Q, RESTATED)).astype(np.int64))
        s = None
        if case.restate:
            s = mg.restate_metric_scores(tables[torch.from_numpy(rows).cuda()].cpu().numpy(), None if w is None else w.cpu().numpy(),
                                         flat, metric)
        m = min(case.k, case.B)
        top, _ = q._search_scan(tables, flat_d, w, m, metric=metric)
        thr = top[:, m - 1].clone()
        qi = torch.arange(case.Q, device="cuda")
        thr[qi % 4 == 1] = float("-inf")
        thr[qi % 4 == 2] = float("inf")
        thr[qi % 4 == 3] = top[:, (m + 1) // 2 - 1][qi % 4 == 3]
        _CACHE["metric"][metric] = (w, rows, s, thr.contiguous())
    return _CACHE["metric"][metric]


def _compacted(q, tables, flat_d, w, k, metric, keep_d, thr):
    """rule 11's other side on the device: the UNMASKED calls over the compacted store, positions mapped back"""
    pos = torch.nonzero(keep_d)[:, 0]
    Q = tables.shape[0]
    if pos.numel() == 0:
        return (torch.full((Q, k), float("inf"), device="cuda"), torch.full((Q, k), -1, dtype=torch.int64, device="cuda"),
                torch.zeros(Q + 1, dtype=torch.int64, device="cuda"), torch.zeros(0, device="cuda"),
                torch.zeros(0, dtype=torch.int64, device="cuda"))
    sub, wsub = flat_d[pos].contiguous(), None if w is None else w[pos].contiguous()
    s, i = q._search_scan(tables, sub, wsub, k, metric=metric)
    i = torch.where(i >= 0, pos[i.clamp(min=0)], i)
    lims, val, p = q._search_range(tables, sub, wsub, thr, metric)
    return s, i, lims, val, pos[p]


@pytest.mark.parametrize("pattern", kg.PATTERNS)
@pytest.mark.parametrize("metric", kg.METRICS)
@pytest.mark.parametrize("case", kg.CASES, ids=lambda c: c.name)
def test_mask_case(case, metric, pattern):
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)
    w, rows, s, thr = _per_metric(case, metric)
    Q, B, k = case.Q, case.B, case.k
    keep, words = kg.words_for(pattern, B, SEED, k)
    keep_d, words_d = torch.from_numpy(keep).cuda(), torch.from_numpy(words).cuda()

    # the two ways to hand a mask in agree (garbage_tail: the bits past B are ignored, so its candidates are the bool's)
    ts, ti = q._search_scan(tables, flat_d, w, k, metric=metric, mask=words_d)
    bs, bi = q._search_scan(tables, flat_d, w, k, metric=metric, mask=keep_d)
    assert ts.dtype == torch.float32 and ti.dtype == torch.int64 and tuple(ts.shape) == tuple(ti.shape) == (Q, k)
    assert torch.equal(_i32(ts), _i32(bs)) and torch.equal(ti, bi)
    lims, val, pos = q._search_range(tables, flat_d, w, thr, metric, mask=words_d)
    b_lims, b_val, b_pos = q._search_range(tables, flat_d, w, thr, metric, mask=keep_d)
    assert torch.equal(lims, b_lims) and torch.equal(_i32(val), _i32(b_val)) and torch.equal(pos, b_pos)
    assert bool(keep_d[pos].all()) and bool(keep_d[ti[ti >= 0]].all())
    print(f"[mask] {case.name} {metric} {pattern}: {int(keep.sum())} candidates, {int(lims[-1])} listed")

    # rule 11 against the unmasked calls over the compacted store: every query
    c_s, c_i, c_lims, c_val, c_pos = _compacted(q, tables, flat_d, w, k, metric, keep_d, thr)
    assert torch.equal(ti, c_i), "positions differ from the search over the compacted store"
    assert torch.equal(_i32(ts), _i32(c_s)), "scores differ from the search over the compacted store"
    assert torch.equal(lims, c_lims) and torch.equal(pos, c_pos) and torch.equal(_i32(val), _i32(c_val))
    if keep.sum() < k:
        assert bool((ti[:, int(keep.sum()):] == -1).all()) and bool(torch.isinf(ts[:, int(keep.sum()):]).all())

    # rules 10 and 11 against the restatement: the restated queries
    if case.restate:
        want_s, want_i = kg.restate_topk_masked(s, keep, k)
        rows_d = torch.from_numpy(rows).cuda()
        assert torch.equal(ti[rows_d], torch.from_numpy(want_i).cuda()), "positions differ from rules 4 and 11"
        assert torch.equal(_i32(ts[rows_d]), _i32(torch.from_numpy(want_s).cuda())), "scores differ from rule 3'"
        w_lims, w_pos, w_val = kg.restate_range_masked(s, keep, thr[rows_d].cpu().numpy())
        l_h, p_h, v_h = lims.cpu().numpy(), pos.cpu().numpy(), val.cpu().numpy()
        for j, qi in enumerate(rows):
            got, want = slice(l_h[qi], l_h[qi + 1]), slice(w_lims[j], w_lims[j + 1])
            assert np.array_equal(p_h[got], w_pos[want]), (qi, "listed positions differ from rules 7, 8 and 11")
            assert np.array_equal(v_h[got].view(np.uint32), w_val[want].view(np.uint32)), qi

    # rule 12: every bit set is no mask at all
    if pattern == "all":
        u_s, u_i = q._search_scan(tables, flat_d, w, k, metric=metric)
        u_lims, u_val, u_pos = q._search_range(tables, flat_d, w, thr, metric)
        assert torch.equal(_i32(ts), _i32(u_s)) and torch.equal(ti, u_i)
        assert torch.equal(lims, u_lims) and torch.equal(_i32(val), _i32(u_val)) and torch.equal(pos, u_pos)

    # the public calls (packed 16-entry codes included: B counts stored vectors): a search over codes[keep], mapped back
    if pattern == "half":
        kpos = torch.nonzero(keep_d)[:, 0]
        a_val, a_idx = q.search(xq, kept, k=k, norms=norms, metric=metric, rnorms=rnorms, mask=keep_d)
        p_val, p_idx = q.search(xq, kept, k=k, norms=norms, metric=metric, rnorms=rnorms, mask=q.pack_mask(keep_d))
        assert torch.equal(_i32(a_val), _i32(p_val)) and torch.equal(a_idx, p_idx)
        sub = dict(norms=norms[kpos], rnorms=rnorms[kpos], metric=metric)
        if kpos.numel():
            c_val, c_idx = q.search(xq, kept[kpos], k=k, **sub)
            assert torch.equal(_i32(a_val), _i32(c_val)) and torch.equal(a_idx, torch.where(c_idx >= 0, kpos[c_idx.clamp(min=0)], c_idx))
            m = min(k, int(kpos.numel()))
            edge = a_val[:, m - 1]
            radius = edge * (1 + 1e-3) + 1e-3 if metric == "l2" else edge - edge.abs() * 1e-3 - 1e-3
            r_lims, r_val, r_idx = q.range_search(xq, kept, radius, norms=norms, metric=metric, rnorms=rnorms, mask=keep_d)
            s_lims, s_val, s_idx = q.range_search(xq, kept[kpos], radius, **sub)
            assert torch.equal(r_lims, s_lims) and torch.equal(_i32(r_val), _i32(s_val)) and torch.equal(r_idx, kpos[s_idx])
            assert int(r_lims[-1]) >= Q * m


@pytest.mark.parametrize("B", (1, 63, 64, 65, 4099))
def test_pack_mask_is_numpy_packbits(B):
    q = base._quantizer(kg.CASES[1])
    rs = np.random.RandomState(B)
    for flags in (rs.rand(B) < 0.5, np.ones(B, bool), np.zeros(B, bool), rs.choice([0, 0, 1, 2, 128, 255], size=B).astype(np.uint8)):
        got = q.pack_mask(torch.from_numpy(flags).cuda())
        assert got.dtype == torch.int64 and tuple(got.shape) == ((B + 63) // 64,)
        want = kg.pack(flags != 0)
        assert np.array_equal(got.cpu().numpy(), want)
        raw = np.packbits(flags != 0, bitorder="little")
        assert np.array_equal(got.cpu().numpy().view(np.uint8)[:len(raw)], raw)
    assert q.pack_mask(torch.zeros(0, dtype=torch.bool, device="cuda")).numel() == 0


@pytest.mark.parametrize("pattern", ("half", "sparse", "blocks", "run", "one_last", "none"))
def test_nan_behind_cleared_bits(pattern):
    """rule 12: norms and rnorms that are NaN wherever the bit is cleared give the results of finite ones"""
    case = kg.CASES[4]
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)
    keep_d = torch.from_numpy(kg.keep_for(pattern, case.B, SEED, case.k)).cuda()
    nan = torch.full_like(norms, float("nan"))
    for metric, w in (("l2", norms), ("cosine", rnorms)):
        _, _, _, thr = _per_metric(case, metric)
        bad = torch.where(keep_d, w, nan)
        s, i = q._search_scan(tables, flat_d, w, case.k, metric=metric, mask=keep_d)
        bs, bi = q._search_scan(tables, flat_d, bad, case.k, metric=metric, mask=keep_d)
        assert torch.equal(_i32(s), _i32(bs)) and torch.equal(i, bi)
        lims, val, pos = q._search_range(tables, flat_d, w, thr, metric, mask=keep_d)
        b_lims, b_val, b_pos = q._search_range(tables, flat_d, bad, thr, metric, mask=keep_d)
        assert torch.equal(lims, b_lims) and torch.equal(_i32(val), _i32(b_val)) and torch.equal(pos, b_pos)
        assert bool(torch.isfinite(b_val).all())


def test_mask_interface():
    from quantization_amd._lib import McqError
    case = kg.CASES[4]
    q, kept, flat, flat_d, xq, tables, norms, rnorms = _prepared(case)
    keep = torch.from_numpy(kg.keep_for("half", case.B, SEED, case.k)).cuda()
    words = q.pack_mask(keep)
    a = q.search(xq, kept, k=5, mask=keep)
    b = q.search(xq.reshape(1, case.Q, case.D), kept, k=5, mask=words)          # leading dimensions, a reused packed mask
    assert tuple(b[0].shape) == (1, case.Q, 5) and torch.equal(a[1], b[1][0]) and torch.equal(_i32(a[0]), _i32(b[0][0]))
    assert bool(keep[a[1]].all())
    with pytest.raises(ValueError, match=str(case.B)):
        q.search(xq, kept, mask=keep[:-1])
    with pytest.raises(ValueError, match=str(case.B)):
        q.range_search(xq, kept, 1.0, mask=words[:-1])
    with pytest.raises(ValueError):
        q.search(xq, kept, mask=keep.to(torch.uint8))
    with pytest.raises(McqError):
        q.search(xq, kept, mask=keep.cpu())
    with pytest.raises(McqError):
        q.range_search(xq, kept, 1.0, mask=words.cpu())
    # a delete is one cleared bit of the packed words the store keeps
    gone = int(a[1][0, 0])
    words2 = words.clone()
    words2[gone >> 6] &= ~(torch.ones((), dtype=torch.int64, device="cuda") << (gone & 63))
    c = q.search(xq, kept, k=5, mask=words2)
    assert gone not in c[1][0].tolist() and c[1][0, :4].tolist() == a[1][0, 1:].tolist()
