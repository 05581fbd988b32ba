"""The reference side of the candidate-list tests (no device): what OracleQuantizer.refine_trace says the workspace of one
refinement pass must hold, level by level, and the states that put exact ties on the boundary of a shortlist.

refine_trace(x, idx) gives, for one vector and one pass (oracle/mcq_oracle.c, refine_one_table): E, R, the stage-0 scores S0[N][K],
every combine's kin * kin scores (`comb`, group by group, ladder step by ladder step) and what every selection kept (`sel_pos`,
`sel_val`: stage 0 first -- N lists of `first` -- then the groups of each ladder step).  The device holds the same objects in
the arrays of TfLists (quantization_amd/csrc/mcq_tf_kernels.h):

  level 0        ent[n][j] = sel_pos (a codebook entry), S[0][n][j] = sel_val
  level v >= 1   ladder step v - 1, lists of kin in and kout out: pos[v][g][j] = (p // kin, p % kin) -- the positions in the two
                 halves' lists --, S[v][g][j] = sel_val
  the result     the last ladder step keeps one pair; lane n walks down the position tree from it to an entry of ent[n]

DESIGN.md section 2(d): a list is the kout smallest by (value, position), lowest position on equal values, in ASCENDING POSITION.
"""
import numpy as np

from golden import gen

D = 32
PASSES = 3

# (N, K) -> vectors.  Batches cross the four-vector workgroup of stage 0 and a wave's worth of vectors; fewer for 32 and 64
# codebooks, whose per-vector trace costs more
SHAPES = [(2, 16), (2, 64), (4, 16), (4, 64), (8, 16), (8, 256), (16, 16), (16, 32), (32, 16), (32, 32), (64, 16), (64, 32),
          (2, 512), (4, 512), (8, 512), (4, 1024)]
STATES = ("plain", "ties", "degenerate")
# the period the center rows of the tie state repeat with: it does not divide the list length (8 for 16 entries, else 16), so
# a run of equal scores straddles the end of a list
PERIODS = {16: 5, 32: 11, 64: 22, 256: 100, 512: 200, 1024: 400}


def batches(N):
    return (1, 5, 67) if N <= 16 else (1, 5, 21)


def make_state(name, N, K, seed=None):
    """plain: gen.synthetic_state.  ties: its center rows repeat with PERIODS[K].  degenerate: every center row is the same"""
    sd = gen.synthetic_state(3100 + N + K if seed is None else seed, D, K, N)
    c = sd["centers"]
    if name == "ties":
        p = PERIODS[K]
        c[:, :] = c[:, np.arange(K) % p]
    elif name == "degenerate":
        c[:, :] = c[0, 0]
    else:
        assert name == "plain"
    return sd


def make_frames(name, N, K, B):
    if name == "degenerate":
        return np.zeros((B, D), np.float32)
    return gen.make_gaussian(3200 + N + K, B, D)


def oracle_of(sd):
    from oracle.oracle import OracleQuantizer
    return OracleQuantizer(sd["centers"], float(sd["centers_scale"]), sd["to_logits.weight"], sd["to_logits.bias"],
                           float(sd["logits_scale"]))


def ladder(N, K):
    from oracle import oracle as O
    return O.ladder(N, K)


def blocks(t, N, K):
    """the selections of a trace, in its order: (level of the list written, group, scores, kin, kout, sel_pos, sel_val).
    Level 0: the stage-0 row of codebook `group` (kin = 0); level v >= 1: the combine of the siblings 2 g, 2 g + 1 of level
    v - 1; the last one (kout == 1) writes no list but the result"""
    first, lad = ladder(N, K)
    sp, sv, comb = t["sel_pos"], t["sel_val"], t["comb"]
    off = 0
    for n in range(N):
        yield 0, n, t["S0"][n], 0, first, sp[off:off + first], sv[off:off + first]
        off += first
    groups, co = N, 0
    for li, (kin, kout) in enumerate(lad):
        groups //= 2
        for g in range(groups):
            yield li + 1, g, comb[co:co + kin * kin], kin, kout, sp[off:off + kout], sv[off:off + kout]
            co += kin * kin
            off += kout
    assert off == sp.size and (co == comb.size or N == 1)


def lists_of(t, N, K):
    """the arrays the device must hold after the pass of trace `t`: {"E", "R", "ent", "S0", "pos1", "S1", ..., "idx"} --
    scores as uint32, ent / idx as uint16, pos[v] as uint8 [groups][kc][2]"""
    out = {"E": t["E"].view(np.uint32).copy(), "R": t["R"].view(np.uint32).copy()}
    ent, levels, win = [], {}, None
    for v, g, _, kin, kout, pos, val in blocks(t, N, K):
        if v == 0:
            ent.append(pos.astype(np.uint16))
            levels.setdefault(0, []).append(val.view(np.uint32))
        elif kout == 1:
            win = (int(pos[0]), kin)
        else:
            levels.setdefault(v, []).append((np.stack([pos // kin, pos % kin], axis=1).astype(np.uint8), val.view(np.uint32)))
    out["ent"] = np.stack(ent)
    out["S0"] = np.stack(levels.pop(0))
    for v, rows in levels.items():
        out[f"pos{v}"] = np.stack([r[0] for r in rows])
        out[f"S{v}"] = np.stack([r[1] for r in rows])
    nlev = 1 + len(levels)
    # the position tree (tf_emit): the winner is the pair (a, b) of positions in the two top-level lists
    idx = np.empty(N, np.uint16)
    for n in range(N):
        v = nlev - 1
        p = win[0] % win[1] if (n >> v) & 1 else win[0] // win[1]
        while v > 0:
            p = int(out[f"pos{v}"][n >> v, p, (n >> (v - 1)) & 1])
            v -= 1
        idx[n] = out["ent"][n, p]
    out["idx"] = idx
    return out


def boundary_ties(t, N, K):
    """per level that holds a list: (lists whose largest kept value also occurs outside the list, lists)"""
    ties, total = {}, {}
    for v, _, scores, _, kout, pos, val in blocks(t, N, K):
        if v > 0 and kout == 1:
            continue
        rest = np.delete(scores, pos)
        total[v] = total.get(v, 0) + 1
        ties[v] = ties.get(v, 0) + int(rest.size > 0 and bool((rest == val.max()).any()))
    return [(ties[v], total[v]) for v in sorted(total)]


_REF = {}
KEPT_TRACES = 5


def reference(N, K, name):
    """Once per (shape, state): the state, max(batches(N)) frames, the arg max of the oracle's logits as start, and PASSES
    passes of the oracle: passes[p] = the lists of every vector stacked ({"E": [B], "ent": [B][N][kc0], ...}), ties[p] =
    boundary_ties summed over the vectors, traces = the raw traces of the first KEPT_TRACES vectors of every pass.  Vectors are
    independent: a smaller batch is a prefix."""
    key = (N, K, name)
    if key in _REF:
        return _REF[key]
    B = max(batches(N))
    sd = make_state(name, N, K)
    x = make_frames(name, N, K, B)
    o = oracle_of(sd)
    start = o.compute_indexes(x, 0).astype(np.uint16)
    idx, passes, ties = start.copy(), [], []
    traces = []
    for _ in range(PASSES):
        per, tie = [], None
        for b in range(B):
            t = o.refine_trace(x[b], idx[b])
            if b < KEPT_TRACES:
                traces.append(t)
            want = lists_of(t, N, K)
            assert np.array_equal(want["idx"], t["idx"]), (N, K, name, b)      # the position tree gives the oracle's own codes
            per.append(want)
            bt = np.array(boundary_ties(t, N, K))
            tie = bt if tie is None else tie + bt
            idx[b] = t["idx"]
        stacked = {k: np.stack([w[k] for w in per]) for k in per[0]}
        stacked["E"] = stacked["E"].reshape(B)
        passes.append(stacked)
        ties.append(tie)
    _REF[key] = dict(state=sd, x=x, start=start, passes=passes, ties=ties, traces=traces)
    return _REF[key]


# ------------------------------------------------------------------------------- the workspace of a pass (mcq_test_pass_layout)
ARRAYS = ("idx", "idxB", "idxC", "final_idx", "map0", "map1", "cnt", "E", "R", "xx", "gterms", "XC", "xf", "xe", "ent",
          "pos1", "pos2", "pos3", "pos4", "pos5", "S0", "S1", "S2", "S3", "S4", "S5", "tabs0", "tabs1")
LIST_ARRAYS = ARRAYS[ARRAYS.index("ent"):ARRAYS.index("tabs0")]
# the order they lie in (carve lays out a level's positions and scores together)
CARVE_ORDER = ARRAYS[:ARRAYS.index("ent")] + ("ent", "S0") + tuple(f"{a}{v}" for v in range(1, 6) for a in ("pos", "S")) + ("tabs0", "tabs1")
assert sorted(CARVE_ORDER) == sorted(ARRAYS)
LAYOUT_VALUES = 2 * len(ARRAYS) + 6 + 2


def layout(L, B, N, K):
    """mcq_test_pass_layout as {"at": {array: (offset, bytes)}, "kc": [6], "cw": code width, "total": bytes of the chunk}"""
    import ctypes
    out = (ctypes.c_size_t * LAYOUT_VALUES)()
    n = L.mcq_test_pass_layout(B, N, K, D, out, LAYOUT_VALUES)
    assert n == LAYOUT_VALUES, n
    v = list(out)
    at = {name: (v[2 * i], v[2 * i + 1]) for i, name in enumerate(ARRAYS)}
    return dict(at=at, kc=v[2 * len(ARRAYS):2 * len(ARRAYS) + 6], cw=v[-2], total=v[-1])
