"""The reference side of the masked cousin tables (no device): which entries of a level-1 cousin table T_1[X][Y] the later readers
of a pass reach, and the masks tf_table1<USED2> (quantization_amd/csrc/mcq_tf_kernels.h) derives from the level-2 lists.

Two views of the same pass, kept apart on purpose:

  masks_of        what the DEVICE computes, with its own flat index arithmetic on the list bytes: lane c of a half-wave reads
                  pos[2][((b G2 + (Z >> 1)) kc2 + c) 2 + (Z & 1)] and the half-wave ORs 1 << byte (usedX, usedY); quarter w, lane
                  c adds level-0 position pos[1][((b G1 + Z) 16 + c) 2 + (w & 1)] to its codebook's set only if candidate c is used
  reads_of        what the READERS index, written as they do (tf_up: entry (px[2 i + a], py[2 j + c]) of the table of the halves
                  a, c, for all kc x kc pairs (i, j) of the two level-2 lists): the sibling combine of level 2 (k_tf_comb) and,
                  with 16 codebooks and more, the level-2 tables of the cousins of every level above (k_tf_up / k_tf_comb3 build
                  them over every pair of level-2 candidates -- a superset of what a higher list then reads through them)
"""
import numpy as np

import pass_lists as pl
from golden import gen

PASSES = 3
# (N, K, D) of tests/test_gpu_lazy_tables.py: lists of 16 (K >= 32), 8 and 16 codebooks, dimensions that are no multiple of 16 / 32
SHAPES = [(8, 32, 24), (8, 64, 32), (8, 256, 32), (16, 32, 16), (16, 256, 32)]
BATCHES = (1, 5, 67, 259)
STATES = ("plain", "ties")
# 32 and 64 codebooks (and 16 below the chunk threshold): the mask sits on their k_tf_table1 launches above level 2
UPPER_SHAPES = [(16, 32, 16), (32, 32, 16), (64, 32, 16)]
UPPER_BATCH = 5


def make_state(name, N, K, D):
    """pass_lists.make_state at any dimension"""
    sd = gen.synthetic_state(3100 + N + K + D, D, K, N)
    c = sd["centers"]
    if name == "ties":
        c[:, :] = c[:, np.arange(K) % pl.PERIODS[K]]
    elif name == "degenerate":
        c[:, :] = c[0, 0]
    else:
        assert name == "plain"
    return sd


def make_frames(name, N, K, D, B):
    return np.zeros((B, D), np.float32) if name == "degenerate" else gen.make_gaussian(3200 + N + K + D, B, D)


_REF = {}


def reference(N, K, D, name, B=max(BATCHES)):
    """Once per (shape, state, batch): state, frames, start codes and PASSES passes of the oracle, each {"E", "R", "ent", "S0",
    "pos1", "S1", ..., "idx"} stacked over the vectors (pass_lists.lists_of).  A smaller batch is a prefix."""
    key = (N, K, D, name, B)
    if key in _REF:
        return _REF[key]
    sd, x = make_state(name, N, K, D), make_frames(name, N, K, D, B)
    o = pl.oracle_of(sd)
    start = o.compute_indexes(x, 0).astype(np.uint16)
    idx, passes = start.copy(), []
    for _ in range(PASSES):
        per = []
        for b in range(B):
            want = pl.lists_of(o.refine_trace(x[b], idx[b]), N, K)
            per.append(want)
            idx[b] = want["idx"]
        stacked = {k: np.stack([w[k] for w in per]) for k in per[0]}
        stacked["E"] = stacked["E"].reshape(B)
        passes.append(stacked)
    _REF[key] = dict(state=sd, x=x, start=start, passes=passes)
    return _REF[key]


def cousin_tables(N):
    """(X, Y) of every level-1 cousin table a pass of N codebooks builds, in the device's order: t = (g per + a) per + c under
    sibling pair g of level v, X = 2 g per + a, Y = (2 g + 1) per + c, per = 2^(v - 1); level 2 first, then level 3"""
    out = []
    for v in range(2, N.bit_length() - 1):
        per = 1 << (v - 1)
        for g in range(N >> (v + 1)):
            for a in range(per):
                for c in range(per):
                    out.append((2 * g * per + a, (2 * g + 1) * per + c))
    return out


def masks_of(pos1, pos2, N, b, X, Y):
    """the device's masks of table (X, Y) of vector b, from the FLAT list bytes: (usedX, usedY, [position set of codebooks
    2X, 2X+1, 2Y, 2Y+1])"""
    p1, p2 = pos1.reshape(-1), pos2.reshape(-1)
    G1, G2, kc2 = N >> 1, N >> 2, 32
    assert pos2.shape[-2] == kc2 and pos1.shape[-2] == 16
    used = []
    for Z in (X, Y):
        u = 0
        for c in range(32):
            u |= 1 << int(p2[((b * G2 + (Z >> 1)) * kc2 + c) * 2 + (Z & 1)])
        used.append(u)
    sets = []
    for w in range(4):
        Z, m = (X if w < 2 else Y), 0
        for c in range(16):
            if (used[w >> 1] >> c) & 1:
                m |= 1 << int(p1[((b * G1 + Z) * 16 + c) * 2 + (w & 1)])
        sets.append(m)
    return used[0], used[1], sets


def reads_of(pos2, N, b):
    """{(X, Y): set of (i0, jj0)} -- the entries of the level-1 cousin tables the readers of vector b's pass index"""
    out = {}
    pairs = []
    for v in range(2, N.bit_length() - 1):      # v = 2: the siblings of level 2 (k_tf_comb); above: the level-2 cousins under the
        per2 = 1 << (v - 2)                     # siblings of level v, whose T_2 k_tf_up / k_tf_comb3 build over all pairs of candidates
        for g in range(N >> (v + 1)):
            pairs += [(2 * g * per2 + a, (2 * g + 1) * per2 + c) for a in range(per2) for c in range(per2)]
    for X2, Y2 in pairs:
        px, py = pos2[b, X2], pos2[b, Y2]                                   # [kc2][2]
        for a in range(2):
            for c in range(2):
                s = out.setdefault((2 * X2 + a, 2 * Y2 + c), set())
                for i in range(px.shape[0]):
                    for j in range(py.shape[0]):
                        s.add((int(px[i, a]), int(py[j, c])))
    return out


def bits(m):
    return [i for i in range(32) if (m >> i) & 1]


def counts_of(pos1, pos2, N, b):
    """the figures of the issue's table for vector b (8 codebooks): per level-1 group the candidates a level-2 list names, per
    codebook the distinct level-0 positions over all 16 candidates and over the named ones, per cousin LEAF table the core gathers
    today and masked, per cousin table the share of entries named"""
    G1 = N >> 1
    named = [set(int(p) for p in pos2[b, h >> 1, :, h & 1]) for h in range(G1)]
    allp = [set(int(p) for p in pos1[b, n >> 1, :, n & 1]) for n in range(N)]
    usedp = [set(int(pos1[b, n >> 1, c, n & 1]) for c in named[n >> 1]) for n in range(N)]
    core_all, core_used, share = [], [], []
    for X, Y in cousin_tables(N):
        share.append(len(named[X]) * len(named[Y]) / 256.0)
        for a in range(2):
            for c in range(2):
                core_all.append(len(allp[2 * X + a]) * len(allp[2 * Y + c]))
                core_used.append(len(usedp[2 * X + a]) * len(usedp[2 * Y + c]))
    return dict(named=[len(s) for s in named], pos_all=[len(s) for s in allp], pos_used=[len(s) for s in usedp], core_all=core_all,
                core_used=core_used, share=share)


# ---------------------------------------------------------------------------------------------------------- the bench state
BENCH = dict(seed=103, D=512, K=256, N=8, vectors=300, frames_seed=0)


def bench_counts(start_passes, vectors=BENCH["vectors"]):
    """the means of counts_of over one pass of `vectors` Gaussian frames on the bench state, started from the codes after
    `start_passes` passes"""
    import torch
    D, K, N = BENCH["D"], BENCH["K"], BENCH["N"]
    o = pl.oracle_of(gen.synthetic_state(BENCH["seed"], D, K, N))
    g = torch.Generator()
    g.manual_seed(BENCH["frames_seed"])
    x = torch.randn(BENCH["vectors"], D, generator=g).numpy().astype(np.float32)[:vectors]
    idx = o.compute_indexes(x, start_passes)
    acc = {}
    for b in range(vectors):
        w = pl.lists_of(o.refine_trace(x[b], idx[b]), N, K)
        for k, v in counts_of(w["pos1"][None], w["pos2"][None], N, 0).items():
            acc.setdefault(k, []).extend(v)
    return {k: float(np.mean(v)) for k, v in acc.items()}
