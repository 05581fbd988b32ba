"""Every cell of the host's kernel-selection tables of the search over stored codes and of the decode (the pick<...> lists of
launch_scan, launch_range, launch_lists, launch_decode_sliced and launch_decode_blk in quantization_amd/csrc/mcq_api.hip): the
table of the shapes that reach each cell once, what each shape CLAIMS to reach, and the value lists read from the source.

The case tables of the other search grids were chosen for paths (tiles, slices, partial steps, ties); this one is chosen for
template arguments.  Nothing here is new launch arithmetic: the (QT, tiles, slices) of a cell come from search_grid.tile_plan
through scan_plan and search_range_grid.range_plan, the parts of a lists cell from search_lists_grid.lists_plan.  The value
lists are read from mcq_api.hip by regex (as search_grid.constants() reads its constants), and coverage() asserts that the
product of the lists of every dispatcher is what the cells below -- and, for the decode, the named cells of other tests --
launch, so that a value added to a pick<...> list fails tests/test_search_selection_host.py until it gets a cell.  The lists of
launch_range_lists, and the cells of both list launchers with a bias, are held against tests/search_bias_grid.py.

  scan, sweeps   base cells: all 35 (QT, N), K = 16 (the tile cap is 16 at every N), Q = 1, 2, 3, 6, 11 for QT = 1, 2, 4, 8, 16:
                 every tile of QT >= 4 has a padding query; the waves' lists fill the LDS (lds = max(tables, lists))
                 capped cells: QT 2 at 64 x 256, QT 4 at 32 x 256 and 64 x 128, QT 8 at 16 x 256, 32 x 128 and 64 x 64,
                 Q = 2 QT + 1: three tiles, the last ragged, the tables fill kScanTableLds
                 B = 1,061 (several slices, a last step of 37 candidates), k = 10, D = 24
  lists          7 values of N, K = 16, Q = 3, B = 1,500, k = 10, P = 3, 9 lists of uneven lengths
  decode         k_decode_sliced: N in 1 .. 64 x dims 100, 200, 300, 1,000, 1,100 (LPV 4 .. 64), K = 32, 4,099 vectors
                 k_decode_blk<4, 2>, <8, 2>: 4 x 1,024 and 8 x 512 with one-byte codes, 4,355 vectors, D = 72
                 k_decode with packed digits: 16 x 16, rep 2, 4, 8, 16 (tests/test_gpu_selection_grid.py runs the three)"""
import itertools
import os
import re
from dataclasses import dataclass

import numpy as np

import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg

API = os.path.join(sg.ROOT, "quantization_amd", "csrc", "mcq_api.hip")
ME = "tests/search_selection_grid.py"

# dispatcher -> (what each of its pick<...> lists selects, in the order they are written; the number of pick_bool calls)
DISPATCHERS = {
    "launch_scan": (("metric", "QT", "N"), 1),
    "launch_range": (("QT", "CH"), 1),
    "launch_lists": (("metric", "N"), 2),                 # masked or not, with a bias or without
    "launch_range_lists": (("CH",), 2),
    "launch_decode_sliced": (("CH", "LPV"), 0),
    "launch_decode_blk": (("N", "LPV"), 0),
}


def pick_lists(launcher, path=API):
    """the value lists of the pick<...> calls inside `launcher`, in source order, as a dict by what they select"""
    with open(path) as f:
        src = f.read()
    with open(sg.HDR) as f:
        names = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr\s+int\s+(kMetric\w+)\s*=\s*([0-9]+);", f.read())}
    m = re.search(r"^int\s+" + launcher + r"\s*\(", src, re.M)
    assert m, f"{launcher} moved out of mcq_api.hip or was renamed: update {ME}"
    end = src.find("\n}\n", m.end())
    assert end > 0, f"{launcher}: no end of the function found: update {ME}"
    body = src[m.end():end]
    what, bools = DISPATCHERS[launcher]
    lists = re.findall(r"\bpick<([^<>]*)>\s*\(", body)
    assert len(lists) == len(what) and len(re.findall(r"\bpick_bool\s*\(", body)) == bools, \
        f"{launcher} no longer selects {what} and {bools} flag(s): update {ME}"
    out = {}
    for name, text in zip(what, lists):
        vals = []
        for tok in text.split(","):
            tok = tok.strip()
            assert re.fullmatch(r"[0-9]+", tok) or tok in names, f"{launcher}: value {tok!r} of pick<{text}>: update {ME}"
            vals.append(names[tok] if tok in names else int(tok))
        assert len(set(vals)) == len(vals), f"{launcher}: pick<{text}> repeats a value"
        out[name] = tuple(vals)
    return out


# ------------------------------------------------------------------ the scan and the sweeps
D, B, KTOP = 24, 1061, 10
NS = (1, 2, 4, 8, 16, 32, 64)
Q_OF_QT = {1: 1, 2: 2, 4: 3, 8: 6, 16: 11}              # the smallest Q that reaches the tile; QT >= 4: a padding query
CAPPED = ((2, 64, 256), (4, 32, 256), (4, 64, 128), (8, 16, 256), (8, 32, 128), (8, 64, 64))      # (QT, N, K): N * K * QT * 4 = kScanTableLds
METRICS = rg.METRICS
SEED = 1
ZERO_WORD = 2                                           # the mask word cleared whole: positions 128 .. 191


@dataclass(frozen=True)
class Cell:
    N: int
    K: int
    Q: int
    qt: int                         # claims: the tile of the scan and of the sweeps,
    tiles: int                      # the number of query tiles,
    capped: bool                    # the tables fill kScanTableLds (else: the waves' lists decide the LDS of the scan)
    D: int = D
    B: int = B
    k: int = KTOP

    @property
    def name(self):
        return f"qt{self.qt}_n{self.N}_k{self.K}"

    @property
    def padded(self):
        """claims a query past the end of the call in the last tile, which tile_stage stages as zeros"""
        return self.qt >= 4 or self.capped

    def case(self):
        """the case of tests/search_grid.py whose machinery (test_gpu_search._quantizer, _store, _queries) makes the inputs:
        a decode-only state, random bytes below K as codes, gaussian queries"""
        return sg.Case(self.name, self.N, self.K, self.D, self.Q, self.B, self.k, state="decode_only", codes="random")


CELLS = [Cell(N, 16, Q_OF_QT[qt], qt, 1, False) for qt in Q_OF_QT for N in NS] + \
        [Cell(N, K, 2 * qt + 1, qt, 3, True) for qt, N, K in CAPPED]


def range_chunk_cap(path=API, launcher="launch_range"):
    """the largest chunk of the sweeps, read from the value `launcher` picks on: a.N < cap ? a.N : cap"""
    with open(path) as f:
        src = f.read()
    m = re.search(r"^int\s+" + launcher + r"\s*\(", src, re.M)
    assert m, f"{launcher} moved out of mcq_api.hip or was renamed: update {ME}"
    body = src[m.end():src.find("\n}\n", m.end())]
    m = re.search(r"\(\s*a\.N\s*<\s*([0-9]+)\s*\?\s*a\.N\s*:\s*([0-9]+)\s*,", body)
    assert m and m.group(1) == m.group(2), f"{launcher} no longer picks its chunk as min(N, cap): update {ME}"
    return int(m.group(1))


def range_ch(N, cap):
    """the chunk of the sweeps: the digits of a candidate arrive min(N, cap) at a time"""
    return min(N, cap)


def mask_for(B, k=KTOP, seed=SEED):
    """the mask of the cells: (keep bool (B,), int64 words) -- about half the bits set, word ZERO_WORD all zero, the bits of
    the last word at positions >= B set (rule 10 ignores them; only hand-packed words can say so)"""
    keep, words = kg.words_for("garbage_tail", B, seed, k)
    keep = keep.copy()
    keep[64 * ZERO_WORD:64 * (ZERO_WORD + 1)] = False
    words = words.copy()
    words[ZERO_WORD] = 0
    return keep, words


def few_for(B, k=KTOP, seed=SEED):
    """k - 1 candidates spread over the store: rule 4 gives a tail of one (+inf, -1)"""
    keep = kg.keep_for("few", B, seed, k)
    return keep, kg.pack(keep)


def reachable_tiles(ns, c):
    """the (QT, N) tile_plan can produce inside the domain of the search (16 <= K <= 256)"""
    return {(sg.tile_plan(Q, B, N, K, c["kScanWaves"], c)[0], N)
            for N in ns for K in (16, 32, 64, 128, 256) for Q in range(1, 2 * c["kScanQTMax"] + 2)}


# ------------------------------------------------------------------ the lists kernel
LISTS_K, LISTS_Q, LISTS_B, LISTS_P = 16, 3, 1500, 3
LISTS_START = 11
LISTS_LENS = (200, 0, 37, 333, 65, 129, 190, 301, 100)   # none a multiple of 64, one empty, one below a step, some above two
LISTS_PROBES = ((3, 1, 2), (7, -1, 0), (6, 5, 4))        # the long, the empty and the short list; a padded row; three more


def lists_case(N):
    return sg.Case(f"lists_n{N}_k{LISTS_K}", N, LISTS_K, D, LISTS_Q, LISTS_B, KTOP, state="decode_only", codes="random")


def lists_layout():
    """(list_offsets int64 (10,), probes int32 (3, 3))"""
    off = LISTS_START + np.concatenate([[0], np.cumsum(LISTS_LENS)]).astype(np.int64)
    return off, np.array(LISTS_PROBES, dtype=np.int32)


# ------------------------------------------------------------------ the decode
SLICED_K, SLICED_B = 32, 4099
SLICED_NS = NS
SLICED_DIMS = {100: 4, 200: 8, 300: 16, 1000: 32, 1100: 64}          # dim -> the LPV it claims; none a multiple of 16
SLICED_TYPES = ("uint8", "int64")
BLK_CELLS = {(4, 1024): (4, 2), (8, 512): (8, 2)}                    # (N, K) -> the k_decode_blk<N, LPV> it claims
BLK_B, BLK_D, BLK_LDS_MIN = 4355, 72, 4096
# k_decode_blk cells that tests/test_gpu_parity.py launches (test_block_staged_decode_whole_and_partial_blocks,
# test_decode_of_sixteen_big_codebooks_uses_32_byte_slices): (N, K) -> <N, LPV>
BLK_ELSEWHERE = {(4, 256): (4, 4), (8, 256): (8, 4), (16, 128): (16, 4), (16, 256): (16, 2)}
PACKED_N, PACKED_K, PACKED_B = 16, 16, 5
PACKED_REPS = ((2, "int64"), (4, "int64"), (8, "int64"), (16, "int64"), (2, "uint8"))
PACKED_DIMS = (20, 300)


def decode_sliced_lpv(dim):
    """decode_sliced_lpv of mcq_api.hip: 8 slices x lpv lanes x 4 floats cover the padded dim"""
    lpv = 4
    while lpv * 32 < sg.padded(dim):
        lpv *= 2
    return lpv


def decode_sliced_ch(N):
    return 4 if N <= 4 else (8 if N <= 8 else 16)


def decode_blk_lpv(N, K):
    """decode_blk_lpv of mcq_api.hip: 64-byte slices of all rows beside two 16 KB code buffers in 160 KB of LDS, else 32-byte"""
    for lpv in (4, 2):
        if N * K * 16 * lpv + 2 * 16384 <= 160 * 1024:
            return lpv
    return 0


def pack_digits(idx, rep, K, dtype):
    """_maybe_separate_indexes of quantization_amd/quantizer.py backwards: (B, N) digits below K -> (B, N / rep) codes, `rep`
    digits per code, least significant first"""
    Bn, N = idx.shape
    d = idx.astype(np.int64).reshape(Bn, N // rep, rep)
    out = np.zeros((Bn, N // rep), dtype=np.int64)
    for r in range(rep):
        out += d[:, :, r] * (K ** r)
    assert out.min() >= 0 and out.max() <= np.iinfo(dtype).max
    back = (out[:, :, None] // (K ** np.arange(rep, dtype=np.int64))[None, None, :]) % K
    assert np.array_equal(back.reshape(Bn, N), idx)
    return out.astype(dtype)


# ------------------------------------------------------------------ the cells against the lists of the source
UNREACHABLE = {name: set() for name in DISPATCHERS}       # instantiated cells that no call can reach: none


def coverage(path=API):
    """Assert, dispatcher by dispatcher, that the product of its pick<...> lists is exactly what the cells of this module
    launch plus what UNREACHABLE names, and that nothing UNREACHABLE can be produced.  -> the number of cells per dispatcher."""
    c = rg.constants()
    lc = lg.constants()
    out = {}

    scan = pick_lists("launch_scan", path)
    assert set(scan["metric"]) == {mg.CODE[m] for m in METRICS}, f"launch_scan: metrics {scan['metric']}: update {ME}"
    got = {(sg.scan_plan(x.Q, x.B, x.N, x.K, x.k, c).qt, x.N) for x in CELLS}
    want = set(itertools.product(scan["QT"], scan["N"]))
    assert want == got | UNREACHABLE["launch_scan"], \
        f"launch_scan: (QT, N) without a cell {sorted(want - got)}, cells without an instantiation {sorted(got - want)}: update {ME}"
    assert not UNREACHABLE["launch_scan"] & reachable_tiles(scan["N"], c)
    assert got <= reachable_tiles(scan["N"], c)
    out["launch_scan"] = len(want) * len(scan["metric"]) * 2

    sweep = pick_lists("launch_range", path)
    cap = range_chunk_cap(path)
    got = {(rg.range_plan(x.Q, x.B, x.N, x.K, c).qt, range_ch(x.N, cap)) for x in CELLS}
    want = set(itertools.product(sweep["QT"], sweep["CH"]))
    assert want == got | UNREACHABLE["launch_range"], \
        f"launch_range: (QT, CH) without a cell {sorted(want - got)}, cells without an instantiation {sorted(got - want)}: update {ME}"
    assert not UNREACHABLE["launch_range"] & {(qt, range_ch(N, cap)) for qt, N in reachable_tiles(NS, c)}
    out["launch_range"] = len(want) * 2 * 2

    lists = pick_lists("launch_lists", path)
    assert set(lists["metric"]) == {mg.CODE[m] for m in METRICS}, f"launch_lists: metrics {lists['metric']}: update {ME}"
    assert set(lists["N"]) == set(NS) | UNREACHABLE["launch_lists"], f"launch_lists: N {lists['N']} against the cells {NS}: update {ME}"
    assert lg.lists_plan(LISTS_Q, LISTS_P, max(NS), LISTS_K, KTOP, lc).parts >= 1
    out["launch_lists"] = len(lists["N"]) * len(lists["metric"]) * 2        # without a bias; with one: tests/search_bias_grid.py

    sliced = pick_lists("launch_decode_sliced", path)
    got = {(decode_sliced_ch(N), decode_sliced_lpv(dim)) for N in SLICED_NS for dim in SLICED_DIMS}
    want = set(itertools.product(sliced["CH"], sliced["LPV"]))
    assert want == got | UNREACHABLE["launch_decode_sliced"], \
        f"launch_decode_sliced: (CH, LPV) without a cell {sorted(want - got)}, cells without an instantiation {sorted(got - want)}: update {ME}"
    out["launch_decode_sliced"] = len(want) * len(SLICED_TYPES)

    blk = pick_lists("launch_decode_blk", path)
    here = {decode_blk_lpv(N, K) and (N, decode_blk_lpv(N, K)) for N, K in BLK_CELLS}
    there = {decode_blk_lpv(N, K) and (N, decode_blk_lpv(N, K)) for N, K in BLK_ELSEWHERE}
    assert here == set(BLK_CELLS.values()) and there == set(BLK_ELSEWHERE.values())
    want = set(itertools.product(blk["N"], blk["LPV"]))
    assert want == here | there | UNREACHABLE["launch_decode_blk"], \
        f"launch_decode_blk: <N, LPV> without a cell {sorted(want - here - there)}, cells without an instantiation " \
        f"{sorted((here | there) - want)}: update {ME}"
    out["launch_decode_blk"] = len(want)
    return out
