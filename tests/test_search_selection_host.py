"""Host-side checks of the kernel-selection cells of the search and of the decode (no GPU): the pick<...> lists read from
quantization_amd/csrc/mcq_api.hip against the cell table of tests/search_selection_grid.py -- a value added to a list, or a
dispatcher that moved, fails here -- and every claim of a cell (the tile reached, the tiles, the slices, the partial last step,
the padding query, the regime of the LDS size, what the mask and the lists hold) against the mirrors of the launch arithmetic
(search_grid.scan_plan, search_range_grid.range_plan, search_lists_grid.lists_plan)."""
import os
import re

import numpy as np
import pytest

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_range_grid as rg
import search_selection_grid as ss


def test_cells_cover_the_product_of_every_pick_list():
    n = ss.coverage()
    assert n == {"launch_scan": 210, "launch_range": 80, "launch_lists": 42, "launch_decode_sliced": 30, "launch_decode_blk": 6}
    assert len(ss.CELLS) == 41 and len({c.name for c in ss.CELLS}) == 41
    assert not any(ss.UNREACHABLE.values())                 # (an entry belongs in DESIGN.md section 4 as well)


def _doctored(tmp_path, launcher, old, new):
    """a copy of mcq_api.hip with one pick<...> list of one dispatcher changed"""
    with open(ss.API) as f:
        src = f.read()
    at = re.search(r"^int\s+" + launcher + r"\s*\(", src, re.M).end()
    assert src.count(old, at, src.find("\n}\n", at)) == 1, (launcher, old)
    path = os.path.join(str(tmp_path), "mcq_api.hip")
    with open(path, "w") as f:
        f.write(src[:at] + src[at:].replace(old, new, 1))
    return path


@pytest.mark.parametrize("launcher,old,new", [
    ("launch_scan", "pick<1, 2, 4, 8, 16>(", "pick<1, 2, 4, 8, 16, 32>("),
    ("launch_scan", "pick<1, 2, 4, 8, 16, 32, 64>(", "pick<1, 2, 4, 8, 16, 32, 64, 128>("),
    ("launch_scan", "pick<kMetricL2, kMetricIP, kMetricCos>(", "pick<kMetricL2, kMetricIP, kMetricCos, 3>("),
    ("launch_range", "pick<1, 2, 4, 8>(", "pick<1, 2, 4, 8, 16>("),
    ("launch_range", "pick<1, 2, 4, 8, 16>(", "pick<1, 2, 4, 8>("),
    ("launch_lists", "pick<1, 2, 4, 8, 16, 32, 64>(", "pick<1, 2, 4, 8, 16, 32, 64, 128>("),
    ("launch_decode_sliced", "pick<4, 8, 16, 32, 64>(", "pick<4, 8, 16, 32, 64, 128>("),
    ("launch_decode_sliced", "pick<4, 8, 16>(", "pick<4, 8, 16, 32>("),
    ("launch_decode_blk", "pick<4, 2>(", "pick<4, 2, 1>("),
    ("launch_decode_blk", "pick<4, 8, 16>(", "pick<4, 8, 16, 32>("),
    ("launch_lists", "pick_bool(mask != nullptr,", "pick_flag(mask != nullptr,"),
    ("launch_lists", "pick_bool(li.bias != nullptr,", "pick_flag(li.bias != nullptr,"),
    ("launch_scan", "launch_rc();", "pick<1, 2>(0, [](auto) { return 0; });"),
])
def test_a_changed_pick_list_fails_the_coverage(tmp_path, launcher, old, new):
    with pytest.raises(AssertionError, match="search_selection_grid"):
        ss.coverage(_doctored(tmp_path, launcher, old, new))


def test_a_moved_dispatcher_names_this_module(tmp_path):
    with open(ss.API) as f:
        src = f.read()
    path = os.path.join(str(tmp_path), "mcq_api.hip")
    with open(path, "w") as f:
        f.write(src.replace("int launch_lists(", "int launch_by_lists("))
    with pytest.raises(AssertionError, match="launch_lists moved .* tests/search_selection_grid.py"):
        ss.pick_lists("launch_lists", path)


@pytest.mark.parametrize("cell", ss.CELLS, ids=lambda c: c.name)
def test_cell_reaches_what_it_claims(cell):
    c = rg.constants()
    scan = sg.scan_plan(cell.Q, cell.B, cell.N, cell.K, cell.k, c)
    sweep = rg.range_plan(cell.Q, cell.B, cell.N, cell.K, c)
    keep, words = ss.mask_for(cell.B)
    for p in (scan, sweep):
        assert p.qt == cell.qt and p.qtiles == cell.tiles, (cell.name, p)
        assert p.slices > 1 and p.last_step_partial(cell.B), (cell.name, p)
        assert (cell.Q % p.qt != 0) == cell.padded, cell.name
        # the cleared word lies inside a slice, with live steps of the same slice on both sides
        s = 64 * ss.ZERO_WORD // p.per_slice
        part = keep[s * p.per_slice:min(cell.B, (s + 1) * p.per_slice)]
        at = 64 * ss.ZERO_WORD - s * p.per_slice
        assert part[:at].any() and part[at + 64:].any() and not part[at:at + 64].any()
    assert scan.slices == 3 and cell.B - (scan.slices - 1) * scan.per_slice < scan.per_slice
    tab, lists = cell.qt * cell.N * cell.K * 4, cell.qt * c["kScanWaves"] * 64 * 8
    assert scan.lds == max(tab, lists) and scan.lds <= c["kScanTableLds"]
    assert (tab == c["kScanTableLds"]) == cell.capped and (tab <= lists) == (not cell.capped)
    assert 2 * cell.qt * cell.N * cell.K * 4 > c["kScanTableLds"] or cell.qt == c["kScanQTMax"] or cell.Q <= cell.qt
    case = cell.case()
    assert (case.N, case.K, case.D, case.Q, case.B, case.k) == (cell.N, cell.K, 24, cell.Q, 1061, 10)
    assert case.state == "decode_only" and case.codes == "random" and not case.packed


def test_cell_table_is_the_one_the_kernels_need():
    c = rg.constants()
    base = [x for x in ss.CELLS if not x.capped]
    assert {(x.qt, x.N) for x in base} == {(qt, N) for qt in (1, 2, 4, 8, 16) for N in (1, 2, 4, 8, 16, 32, 64)}
    assert all(x.K == 16 and x.tiles == 1 and x.Q == {1: 1, 2: 2, 4: 3, 8: 6, 16: 11}[x.qt] for x in base)
    capped = [x for x in ss.CELLS if x.capped]
    assert {(x.qt, x.N, x.K) for x in capped} == {(2, 64, 256), (4, 32, 256), (4, 64, 128), (8, 16, 256), (8, 32, 128), (8, 64, 64)}
    assert all(x.Q == 2 * x.qt + 1 and x.tiles == 3 for x in capped)
    # every (QT, N) the tile plan can produce with the tables at the cap has its capped cell
    full = {(qt, N) for qt, N in ss.reachable_tiles(ss.NS, c) if 1 < qt < c["kScanQTMax"]
            and any(qt * N * K * 4 == c["kScanTableLds"] for K in (16, 32, 64, 128, 256))}
    assert full == {(x.qt, x.N) for x in capped}
    assert {(x.B, x.k, x.D) for x in ss.CELLS} == {(1061, 10, 24)}


def test_masks_hold_what_the_cells_need():
    for B in (ss.B, ss.LISTS_B):
        keep, words = ss.mask_for(B)
        assert 0.4 * B < keep.sum() < 0.6 * B and keep.sum() >= ss.KTOP
        assert words.dtype == np.int64 and len(words) == kg.words_of(B) and words[ss.ZERO_WORD] == 0
        assert np.array_equal(kg.unpack(words, B), keep)                        # below B the words are the candidates,
        tail = np.unpackbits(words[-1:].view(np.uint8), bitorder="little")[B % 64:]
        assert B % 64 and tail.all()                                            # and every bit past B is set
        assert not np.array_equal(words, kg.pack(keep))
        few, few_words = ss.few_for(B)
        assert few.sum() == ss.KTOP - 1 and np.array_equal(kg.unpack(few_words, B), few)
    p = sg.scan_plan(1, ss.B, 8, 16, ss.KTOP)
    few, _ = ss.few_for(ss.B)
    assert len({int(b) // p.per_slice for b in np.flatnonzero(few)}) == p.slices    # the short result is merged from every slice


def test_lists_cells_reach_what_they_claim():
    c = lg.constants()
    off, probes = ss.lists_layout()
    L = len(off) - 1
    lens = np.diff(off)
    assert L == 9 and probes.shape == (ss.LISTS_Q, ss.LISTS_P) == (3, 3) and probes.dtype == np.int32 and off.dtype == np.int64
    assert off[0] > 0 and off[-1] < ss.LISTS_B == 1500 and ss.LISTS_K == 16
    assert len(set(lens.tolist())) == L and (lens[lens > 0] % 64 != 0).all()
    assert (lens == 0).sum() == 1 and ((lens > 0) & (lens < 64)).any() and (lens > 128).any()
    named = [[l for l in row.tolist() if 0 <= l < L] for row in probes]
    assert all(len(r) == len(set(r)) for r in named)                             # rule 13: a row holds distinct lists
    assert sum((row == -1).any() for row in probes) == 1 and all(len(r) >= 2 for r in named)
    probed = {l for r in named for l in r}
    assert {int(np.argmax(lens)), int(np.flatnonzero(lens == 0)[0]), int(np.flatnonzero((lens > 0) & (lens < 64))[0])} <= probed
    keep, _ = ss.mask_for(ss.LISTS_B)
    for row in probes:
        assert len(lg.candidates(off, row, keep)) >= ss.KTOP
    for N in ss.NS:
        case = ss.lists_case(N)
        assert (case.N, case.K, case.D, case.Q, case.B, case.k) == (N, 16, 24, 3, 1500, 10)
        plan = lg.lists_plan(case.Q, ss.LISTS_P, N, case.K, case.k, c)
        assert plan.parts > 1
        # a part boundary falls inside a list: some probe's steps lie in more than one part
        cut = False
        for row in probes:
            rng, pre = lg.step_space(off, row, case.B)
            for lo, hi in lg.part_steps(int(pre[-1]), plan.parts):
                cut |= any(pre[p] < lo < pre[p + 1] for p in range(len(row)))
        assert cut, N


def test_decode_cells_reach_what_they_claim():
    for dim, lpv in ss.SLICED_DIMS.items():
        assert ss.decode_sliced_lpv(dim) == lpv and dim % 16 != 0
        assert 8 * lpv * 4 >= sg.padded(dim) > 8 * (lpv // 2) * 4 or lpv == 4
    assert sorted(ss.SLICED_DIMS.values()) == [4, 8, 16, 32, 64] and sorted(ss.SLICED_DIMS) == [100, 200, 300, 1000, 1100]
    assert {ss.decode_sliced_ch(N) for N in ss.SLICED_NS} == {4, 8, 16} and ss.SLICED_NS == (1, 2, 4, 8, 16, 32, 64)
    assert ss.SLICED_B == 4099 >= 4096 and ss.SLICED_K == 32                    # decode_sliced_applies: B >= 4096, K >= 32,
    assert ss.SLICED_B < 16384                                                 # below the LDS-resident kernels' batch size
    assert ss.BLK_CELLS == {(4, 1024): (4, 2), (8, 512): (8, 2)}
    assert ss.BLK_B == 4355 >= ss.BLK_LDS_MIN == 4096 and ss.BLK_D == 72 and ss.BLK_D % 4 == 0
    # the k_decode_blk cells left to tests/test_gpu_parity.py are cases of its tables
    with open(os.path.join(sg.ROOT, "tests", "test_gpu_parity.py")) as f:
        src = f.read()
    m = re.search(r'parametrize\("D,K,N,B", \[([^\]]*)\]\)\s*def test_block_staged_decode_whole_and_partial_blocks', src)
    assert m, "test_block_staged_decode_whole_and_partial_blocks moved: update tests/search_selection_grid.py (BLK_ELSEWHERE)"
    cases = {(int(N), int(K)) for _, K, N, Bn in re.findall(r"\((\d+), (\d+), (\d+), (\d+)\)", m.group(1)) if int(Bn) >= 16384}
    assert re.search(r"def test_decode_of_sixteen_big_codebooks_uses_32_byte_slices\(D\):.*?synthetic_state\(33, D, 256, 16\)", src, re.S)
    assert set(ss.BLK_ELSEWHERE) <= cases | {(16, 256)}
    # packed digits: every rep the entry point accepts; 16 digits of 4 bits fit an int64 only with the top digit below 8
    assert {r for r, _ in ss.PACKED_REPS} == {2, 4, 8, 16} and ss.PACKED_K ** 16 > np.iinfo(np.int64).max >= 8 * ss.PACKED_K ** 15 - 1
    idx = np.random.RandomState(0).randint(0, 16, size=(5, 16))
    idx[:, 15] %= 8
    for rep, dtype in ss.PACKED_REPS:
        got = ss.pack_digits(idx, rep, 16, np.dtype(dtype))
        assert got.shape == (5, 16 // rep) and got.dtype == np.dtype(dtype)
        assert got[0, 0] == sum(int(idx[0, r]) * 16 ** r for r in range(rep))    # least significant digit first
