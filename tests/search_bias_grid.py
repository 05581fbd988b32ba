"""Residual codes list by list (mcq_search_scan_lists_bias, mcq_search_range_lists_bias_count / _fill, mcq_code_norms_based;
include/mcq_residual.h rules 21-23): the numpy restatement of the biased score and of the based norms, the bias of a GPU case, and
the cells of the two list launchers that carry a bias (their value lists are read from quantization_amd/csrc/mcq_api.hip by
tests/search_selection_grid.py).

    score[q][b] = finish((S[q][b] + bias[q][p]), w[b])     p: the slot of row q whose list holds b
                  S: restate_sums of tests/search_metric_grid.py (rule 3's chain); then ONE float32 addition; then
                  finish = (.. + w[b]) under l2, nothing under ip, (.. * w[b]) under cosine, each one float32 operation
    norms[b]    = sum_d (base[assign[b]][d] + sum_n C[n][code[b][n]][d])^2: rows n ascending, then the base element, then
                  the lane chains and the butterfly of rule 2 (restate_norms_based spells them out)

The top-k restatement is lists_grid.restate_lists over the matrix biased_scores() gives (rows hold distinct lists, so every
candidate has ONE slot); the range restatement walks the slots of a row in order, as rule 18 lists them, so a list named twice
is listed twice, each time with the bias of that naming's slot.

The GPU cases are the case tables of tests/search_lists_grid.py and tests/search_range_lists_grid.py themselves: whatever
those tables claim to reach (cut lists, list boundaries inside a wave's run, empty parts, padding rows, 4,096 probes) is
checked against the launch arithmetic by their own host tests, and that arithmetic does not depend on a bias."""
import numpy as np

import search_lists_grid as lg
import search_metric_grid as mg
import search_selection_grid as sel
import search_tables_grid as tg

ME = "tests/search_bias_grid.py"
METRICS = lg.METRICS
PATTERNS = (None, "half")                       # the masks of the GPU cases: none, and `half` of tests/search_mask_grid.py


# ------------------------------------------------------------------ rule 21 in numpy
def finish(Sb, w, metric):
    """the metric's finishing operation of rule 3' on float32 (S + bias): one float32 operation, none under ip"""
    Sb = np.asarray(Sb, dtype=np.float32)
    if metric == "ip":
        return Sb
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.asarray(w, dtype=np.float32)
        return (Sb + w).astype(np.float32) if metric == "l2" else (Sb * w).astype(np.float32)


def slot_scores(S_row, list_offsets, row, bias_row, w, metric):
    """per slot of one query's row, in the row's order: (positions of the named list, their biased scores); a slot that
    names no list has none"""
    L = len(list_offsets) - 1
    out = []
    for p, l in enumerate(row):
        if not 0 <= int(l) < L:
            continue
        pos = np.arange(list_offsets[int(l)], list_offsets[int(l) + 1], dtype=np.int64)
        Sb = (S_row[pos] + np.float32(bias_row[p])).astype(np.float32)
        out.append((pos, finish(Sb, None if w is None else w[pos], metric)))
    return out


def biased_scores(S, list_offsets, probes, bias, w, metric):
    """(Q, B) float32: at the candidates of query q their biased scores (of the LAST slot naming their list, where a row
    names one twice), NaN everywhere else -- the matrix lists_grid.restate_lists and range_lists_grid.thresholds_for take"""
    out = np.full(S.shape, np.nan, dtype=np.float32)
    for q, row in enumerate(probes):
        for pos, val in slot_scores(S[q], list_offsets, row, bias[q], w, metric):
            out[q, pos] = val
    return out


def restate_range_lists_bias(S, list_offsets, probes, bias, w, metric, thr, keep=None):
    """rules 17, 18 and 21: -> (lims int64 (Q + 1,), positions int64, scores float32), the slots of a row in order"""
    thr = np.asarray(thr, dtype=np.float32)
    lims = np.zeros(len(probes) + 1, dtype=np.int64)
    pos_out, val_out = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    for q, row in enumerate(probes):
        n = 0
        for pos, val in slot_scores(S[q], list_offsets, row, bias[q], w, metric):
            with np.errstate(invalid="ignore"):
                hit = val <= thr[q]                                  # a NaN compares false
            if keep is not None:
                hit &= keep[pos]
            pos_out.append(pos[hit])
            val_out.append(val[hit])
            n += int(hit.sum())
        lims[q + 1] = lims[q] + n
    return lims, np.concatenate(pos_out), np.concatenate(val_out)


def named_slots(list_offsets, probes):
    """the (q, p) whose entry names a list that is not empty: the slots whose bias some candidate takes"""
    L = len(list_offsets) - 1
    return [(q, p) for q, row in enumerate(probes) for p, l in enumerate(row)
            if 0 <= int(l) < L and list_offsets[int(l) + 1] > list_offsets[int(l)]]


def bias_for(S, list_offsets, probes, seed=1):
    """the bias of a GPU case, float32 with the shape of probes: fixed-seed normal values scaled to the spread of the case's
    table sums (so that a bias reorders candidates of different lists without drowning the sums); of the slots that name a
    list that is not empty every fifth holds +0.0 and the last -0.0; negatives occur by themselves (asserted)"""
    rs = np.random.RandomState(seed + 7 * probes.shape[1])
    spread = float(np.std(S.astype(np.float64))) or 1.0
    bias = (rs.standard_normal(probes.shape) * spread).astype(np.float32)
    named = named_slots(list_offsets, probes)
    for q, p in named[::5]:
        bias[q, p] = 0.0
    if len(named) > 1:
        bias[named[-1]] = -0.0
    if len(named) > 2:
        bias[named[1]] = -abs(bias[named[1]]) - np.float32(spread)
    return bias


def rows_with_two_lists(list_offsets, probes):
    """the queries whose row names two or more lists that are not empty: where a bias can change the ORDER of the result"""
    count = {}
    for q, _ in named_slots(list_offsets, probes):
        count[q] = count.get(q, 0) + 1
    return [q for q, n in count.items() if n >= 2]


# ------------------------------------------------------------------ rule 22 in numpy
def restate_norms_based(C, codes, base, assign, D):
    """C (N, K, Dp) float32 -- the PADDED rows of `prepared` --, codes (B, N), base (L, D) float32, assign (B,) integer ->
    float32 (B,).  base None: rule 2 itself, restate_norms of tests/search_tables_grid.py, whose row sums and lane chains these
    are: the base row goes in between them."""
    if base is None:
        return tg.restate_norms(C, codes)
    B = codes.shape[0]
    v = tg.row_sums(C, codes)
    ok = (assign >= 0) & (assign < len(base))
    add = np.zeros((B, D), dtype=np.float32)
    add[ok] = base[assign[ok]]
    head = (v[:, :D] + add).astype(np.float32)
    v[:, :D] = np.where(ok[:, None], head, v[:, :D])                 # (no row: nothing is added, not even a zero)
    return tg.lane_sums(v)


# ------------------------------------------------------------------ the launchers' cells with a bias
# launch_lists and launch_range_lists select a kernel with a bias by one more flag over the value lists of the calls without
# one (search_selection_grid.pick_lists reads them, and counts the flags).  The cells tests/test_gpu_search_lists_bias.py and
# test_gpu_search_range_lists_bias.py launch: the layout and the shapes of the lists cells of tests/search_selection_grid.py
# (K = 16, one N per test), three metrics, mask or none; the range kernel at every N as well, count and fill
CELL_NS = sel.NS
CELL_MASKS = (False, True)
CELL_SWEEPS = ("count", "fill")


def coverage(path=sel.API):
    """assert that the product of each launcher's value lists is exactly what the cells above launch -> the cells with a
    bias per launcher"""
    top = sel.pick_lists("launch_lists", path)
    assert set(top["metric"]) == {mg.CODE[m] for m in METRICS}, f"launch_lists: metrics {top['metric']}: update {ME}"
    assert set(top["N"]) == set(CELL_NS), f"launch_lists: N {top['N']} against the cells {CELL_NS}: update {ME}"
    rng = sel.pick_lists("launch_range_lists", path)
    cap = sel.range_chunk_cap(path, "launch_range_lists")
    assert set(rng["CH"]) == {min(N, cap) for N in CELL_NS}, f"launch_range_lists: CH {rng['CH']} against the cells {CELL_NS}: update {ME}"
    return {"launch_lists": len(top["N"]) * len(top["metric"]) * len(CELL_MASKS),
            "launch_range_lists": len(rng["CH"]) * len(CELL_SWEEPS) * len(CELL_MASKS)}
