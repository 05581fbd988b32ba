"""Host-side check of the launch plans of the search (no GPU): every workspace size query of the search entries --
mcq_search_workspace_bytes, mcq_search_lists_workspace_bytes, mcq_search_range_workspace_bytes,
mcq_search_range_lists_workspace_bytes, mcq_search_wide_workspace_bytes, mcq_search_wide_lists_workspace_bytes,
mcq_rerank_workspace_bytes, mcq_search_topk_u16_workspace_bytes, mcq_search_range_u16_workspace_bytes and
mcq_search_shortlist_workspace_bytes -- is held against the Python mirror of its plan (scan_plan, lists_plan, range_plan,
range_lists_plan, wide_plan, rerank_plan, short_plan of tests/*_grid.py) over ONE grid.

The plans of mcq_api.hip share their arithmetic (part_count: max(1, min(target / Q, cap, steps))); the mirrors do not, each
restates its own.  The grid crosses every clamp of every plan -- the target over Q on both sides of 256 / Q and 1,024 / Q, the
slice cap, the merge cap at both halves of wide_half, parts > steps -- and both code widths.  A size depends on the parts of a
query, so a plan whose clamp moved gives another size.  An argument list outside an entry's domain answers 256."""
import itertools

import rerank_grid as rr
import search_grid as sg
import search_lists_grid as lg
import search_range_grid as rg
import search_range_lists_grid as rl
import search_shortlist_grid as hg
import search_wide_grid as wg

QS = (1, 3, 4, 5, 8, 9, 16, 17, 255, 256, 257, 1023, 1024, 1025, 5000)
BS = (1, 64, 65, 4096)
PS = (1, 7, 4096)
SS = (1, 16, 17, 64, 65, 1000, 100000)
DS = (1, 100, 16384)
KS = (1, 64, 65, 512, 513, 1024)
SHAPES = ((1, 16), (8, 256), (64, 256), (16, 1024))          # (N, K); the last one: two-byte codes
NARROW_MAX_K = 64                                           # rule 5 of include/mcq.h
BIG = (1 << 31) - 1
OUTSIDE = 256                                               # what every size query answers outside its domain


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib.lib()


def _hold(entry, mirror, grid, inside):
    """entry(*args) == mirror(*args) for every argument list of the grid that `inside` admits, 256 for every other one
    -> the number of lists inside"""
    n = 0
    for args in grid:
        want = mirror(*args) if inside(*args) else OUTSIDE
        assert entry(*args) == want, (entry.__name__, args, entry(*args), want)
        n += inside(*args)
    return n


def test_size_queries_equal_the_mirrors_over_the_grid():
    L = _lib()
    c = hg.constants()                                      # every constant the mirrors below read, and kRange*Waves
    c.update(rl.constants())
    c.update(rg.constants())
    c.update(rr.constants())
    wide_k, max_p, max_d = c["kWideMaxK"], c["kListMaxProbes"], c["kRerankMaxD"]
    assert max(KS) == wide_k and max(PS) == max_p and max(DS) == max_d
    one = lambda K: K <= 256
    qbnk = [(Q, B, N, K) for Q, B, (N, K) in itertools.product(QS, BS, SHAPES)]
    qpnk = [(Q, P, N, K) for Q, P, (N, K) in itertools.product(QS, PS, SHAPES)]
    with_k = lambda rows: [r + (k,) for r in rows for k in KS]
    seen = 0
    # the scan and the sweeps over the whole store
    seen += _hold(L.mcq_search_workspace_bytes, lambda Q, B, N, K, k: sg.scan_plan(Q, B, N, K, k, c).ws_bytes, with_k(qbnk),
                  lambda Q, B, N, K, k: one(K) and k <= NARROW_MAX_K)
    seen += _hold(L.mcq_search_range_workspace_bytes, lambda Q, B, N, K: rg.range_plan(Q, B, N, K, c).ws_bytes, qbnk,
                  lambda Q, B, N, K: one(K))
    # list by list
    seen += _hold(L.mcq_search_lists_workspace_bytes, lambda Q, P, N, K, k: lg.lists_plan(Q, P, N, K, k, c).ws_bytes, with_k(qpnk),
                  lambda Q, P, N, K, k: one(K) and k <= NARROW_MAX_K)
    seen += _hold(L.mcq_search_range_lists_workspace_bytes, lambda Q, P, N, K: rl.range_lists_plan(Q, P, N, K, c).ws_bytes, qpnk,
                  lambda Q, P, N, K: one(K))
    # past 64 neighbours: the whole store is one list
    seen += _hold(L.mcq_search_wide_workspace_bytes, lambda Q, B, N, K, k: wg.wide_plan(Q, 1, N, K, k, c).ws_bytes, with_k(qbnk),
                  lambda Q, B, N, K, k: one(K))
    seen += _hold(L.mcq_search_wide_lists_workspace_bytes, lambda Q, P, N, K, k: wg.wide_plan(Q, P, N, K, k, c).ws_bytes,
                  with_k(qpnk), lambda Q, P, N, K, k: one(K))
    # two-byte codes: every shape of the library
    seen += _hold(L.mcq_search_topk_u16_workspace_bytes, lambda Q, P, N, K, k: wg.wide_plan(Q, P, N, K, k, c).ws_bytes,
                  with_k(qpnk), lambda *a: True)
    seen += _hold(L.mcq_search_range_u16_workspace_bytes, lambda Q, P, N, K: rl.range_lists_plan(Q, P, N, K, c).ws_bytes, qpnk,
                  lambda *a: True)
    # shortlists
    seen += _hold(L.mcq_rerank_workspace_bytes, lambda Q, S, D, k: rr.rerank_plan(Q, S, D, k, c).ws_bytes,
                  list(itertools.product(QS, SS, DS, KS)), lambda *a: True)
    seen += _hold(L.mcq_search_shortlist_workspace_bytes, lambda Q, S, N, K, k: hg.short_plan(Q, S, N, K, k, c).ws_bytes,
                  with_k([(Q, S, N, K) for Q, S, (N, K) in itertools.product(QS, SS, SHAPES)]), lambda *a: True)
    assert seen == 8505                                     # the lists inside a domain: one that shrank shows here


def test_every_clamp_of_every_plan_is_crossed():
    """the grid reaches what the docstring says it reaches, by the mirrors"""
    c = hg.constants()
    c.update(rr.constants())
    lists = {lg.lists_plan(Q, 1, 8, 256, 1, c).parts for Q in QS}
    assert {1, c["kScanMaxSlices"]} <= lists and len(lists) > 4                               # the target over Q; the slice cap
    for k in KS:
        cap = c["kWideMergeEntries"] // wg.wide_half(k, c)
        wide = {wg.wide_plan(Q, 1, 8, 256, k, c).parts for Q in QS}
        assert max(wide) == cap < c["kScanMaxSlices"] and 1 in wide and len(wide) > 2            # the merge cap, both halves over KS
        for plan, target in ((lambda Q, S: rr.rerank_plan(Q, S, 100, k, c), c["kRerankTargetBlocks"]),
                             (lambda Q, S: hg.short_plan(Q, S, 8, 256, k, c), c["kShortTargetBlocks"])):
            got = [(plan(Q, S), target // Q) for Q in QS for S in SS]
            assert any(p.parts == p.steps < min(cap, t) for p, t in got)                        # parts > steps: the steps decide
            assert any(p.parts == cap < min(p.steps, t) for p, t in got)                        # the merge cap decides
            assert any(p.parts == t < min(cap, p.steps) for p, t in got)                        # the target over Q decides
            assert any(p.parts == 1 and t == 0 for p, t in got)                                 # the floor of one part
    assert {wg.wide_half(k, c) for k in KS} == {c["half_small"], c["half_large"]}
    tiles = [sg.scan_plan(Q, B, N, K, 1, c) for Q in QS for B in BS for N, K in SHAPES[:3]]
    assert {p.qt for p in tiles} == {1, 2, 4, 8, 16} and min(p.slices for p in tiles) == 1 < max(p.slices for p in tiles)


def test_outside_the_domain_every_size_query_answers_256():
    L = _lib()
    bad = {
        "mcq_search_workspace_bytes": [(0, 64, 8, 256, 10), (4, 0, 8, 256, 10), (4, 64, 8, 256, 65), (4, 64, 8, 256, 0),
                                       (4, 64, 8, 512, 10), (4, 64, 3, 256, 10), (BIG + 1, 64, 8, 256, 10), (4, BIG + 1, 8, 256, 10)],
        "mcq_search_range_workspace_bytes": [(0, 64, 8, 256), (4, 0, 8, 256), (4, 64, 16, 1024), (4, 64, 8, 100),
                                             (BIG + 1, 64, 8, 256), (4, BIG + 1, 8, 256)],
        "mcq_search_lists_workspace_bytes": [(0, 7, 8, 256, 10), (4, 0, 8, 256, 10), (4, 4097, 8, 256, 10), (4, 7, 8, 256, 65),
                                             (4, 7, 8, 256, 0), (4, 7, 16, 1024, 10), (BIG + 1, 7, 8, 256, 10)],
        "mcq_search_range_lists_workspace_bytes": [(0, 7, 8, 256), (4, 0, 8, 256), (4, 4097, 8, 256), (4, 7, 16, 1024),
                                                   (BIG + 1, 7, 8, 256)],
        "mcq_search_wide_workspace_bytes": [(0, 64, 8, 256, 100), (4, 0, 8, 256, 100), (4, 64, 8, 256, 1025), (4, 64, 8, 256, 0),
                                            (4, 64, 16, 1024, 100), (BIG + 1, 64, 8, 256, 100), (4, BIG + 1, 8, 256, 100)],
        "mcq_search_wide_lists_workspace_bytes": [(0, 7, 8, 256, 100), (4, 0, 8, 256, 100), (4, 4097, 8, 256, 100),
                                                  (4, 7, 8, 256, 1025), (4, 7, 16, 1024, 100), (BIG + 1, 7, 8, 256, 100)],
        "mcq_rerank_workspace_bytes": [(0, 100, 100, 10), (4, 0, 100, 10), (4, 100, 0, 10), (4, 100, 16385, 10), (4, 100, 100, 1025),
                                       (4, 100, 100, 0), (BIG, 100, 100, 10), (4, BIG, 100, 10)],
        "mcq_search_topk_u16_workspace_bytes": [(0, 7, 16, 1024, 100), (4, 0, 16, 1024, 100), (4, 4097, 16, 1024, 100),
                                                (4, 7, 16, 1024, 1025), (4, 7, 32, 1024, 100), (4, 7, 16, 2048, 100),
                                                (BIG + 1, 7, 16, 1024, 100)],
        "mcq_search_range_u16_workspace_bytes": [(0, 7, 16, 1024), (4, 0, 16, 1024), (4, 4097, 16, 1024), (4, 7, 32, 1024),
                                                 (BIG + 1, 7, 16, 1024)],
        "mcq_search_shortlist_workspace_bytes": [(0, 100, 8, 256, 10), (4, 0, 8, 256, 10), (4, 100, 8, 256, 1025), (4, 100, 8, 256, 0),
                                                 (4, 100, 32, 1024, 10), (BIG, 100, 8, 256, 10), (4, BIG, 8, 256, 10)],
    }
    for name, rows in bad.items():
        for args in rows:
            assert getattr(L, name)(*args) == OUTSIDE, (name, args)
    # the last size inside: the scans and lists admit 2^31 - 1 queries, the shortlists stop one short of it
    assert L.mcq_search_lists_workspace_bytes(BIG, 7, 8, 256, 10) > OUTSIDE
    assert L.mcq_rerank_workspace_bytes(BIG - 1, 100, 100, 10) > OUTSIDE
