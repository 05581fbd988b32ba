"""Host mirror of the launch arithmetic of the search over stored codes (tile_plan and scan_plan in
quantization_amd/csrc/mcq_api.hip, the constants of mcq_search_kernels.h), the numpy restatement of rules 3 and 4 of its
contract (include/mcq.h), and the case table of tests/test_gpu_search.py.

The constants are read from the source, so that a moved tile size or cap makes tests/test_search_host.py fail instead of
leaving the GPU cases covering nothing: each case below CLAIMS which paths it reaches (more than one query tile, more than
one slice of the store, a partial last step of 64 candidates, a store shorter than k) and the host test checks the claims
against the mirror, and the mirror's workspace size against the library's."""
import os
import re
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "quantization_amd", "csrc", "mcq_search_kernels.h")

NAMES = ("kTabRows", "kTabQueries", "kTabChunk", "kNormWaves", "kPieceRows", "kScanWaves", "kScanQTMax", "kScanTableLds",
         "kScanTargetBlocks", "kScanMaxSlices", "kNoIndex")


def constants(path=HDR):
    with open(path) as f:
        src = f.read()
    out = {}
    for name in NAMES:
        m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([0-9a-fx* ]+);", src)
        assert m, f"{name} moved out of mcq_search_kernels.h: update tests/search_grid.py"
        out[name] = int(eval(m.group(1), {"__builtins__": {}}))
    return out


def padded(D):
    return (D + 15) & ~15


def align256(v):
    return (v + 255) & ~255


@dataclass(frozen=True)
class Plan:
    qt: int
    qtiles: int
    slices: int
    per_slice: int
    lds: int
    ws_bytes: int

    def last_step_partial(self, B):
        """some slice ends in a step of fewer than 64 candidates"""
        return any((min(B, (s + 1) * self.per_slice) - s * self.per_slice) % 64 != 0 for s in range(self.slices))


def tile_plan(Q, B, N, K, waves, c):
    """tile_plan of mcq_api.hip, shared by the scan and by the sweeps of the range search -> (qt, qtiles, slices, per_slice)"""
    cap = c["kScanQTMax"]
    while cap > 1 and cap * N * K * 4 > c["kScanTableLds"]:
        cap //= 2
    qt = 1
    while qt < cap and qt < Q:
        qt *= 2
    qtiles = (Q + qt - 1) // qt
    cap_slices = min(max(c["kScanTargetBlocks"] // max(qtiles, 1), 1), c["kScanMaxSlices"])
    steps = (B + 63) // 64
    want = min(max((steps + waves - 1) // waves, 1), cap_slices)
    per = max((((B + want - 1) // want) + 63) // 64 * 64, 64)
    return qt, qtiles, (B + per - 1) // per, per


def scan_plan(Q, B, N, K, k, c=None):
    c = c or constants()
    qt, qtiles, slices, per = tile_plan(Q, B, N, K, c["kScanWaves"], c)
    lds = max(qt * N * K * 4, qt * c["kScanWaves"] * 64 * 8)
    return Plan(qt, qtiles, slices, per, lds, 2 * align256(Q * slices * k * 4))


def tables_grid(Q, N, K, c=None):
    c = c or constants()
    return ((Q + c["kTabQueries"] - 1) // c["kTabQueries"], (N * K + c["kTabRows"] - 1) // c["kTabRows"])


def tables_chain(D):
    """additions of the one chain of a table entry: the padded dim (pad columns add zeros)"""
    return padded(D)


def norms_chains(N, D):
    """(row additions per component, additions of a lane's chain plus the butterfly)"""
    groups = padded(D) // 4
    return max(N - 1, 1), 4 * ((groups + 63) // 64) + 6


# ------------------------------------------------------------------ rules 3 and 4 in numpy
def restate_scores(T, t, codes):
    """rule 3: s[q][b] = (((T[q][0][c_0] + T[q][1][c_1]) + ...) + T[q][N-1][c_{N-1}]) + t[b], float32 additions in this order"""
    T = np.asarray(T, dtype=np.float32)
    t = np.asarray(t, dtype=np.float32)
    Q, N, K = T.shape
    B = codes.shape[0]
    s = np.empty((Q, B), dtype=np.float32)
    cols = [codes[:, n].astype(np.int64) & (K - 1) for n in range(N)]
    for q in range(Q):
        acc = T[q, 0][cols[0]]
        for n in range(1, N):
            acc = (acc + T[q, n][cols[n]]).astype(np.float32)
        s[q] = (acc + t).astype(np.float32)
    return s


def restate_topk(s, k):
    """rule 4: per query the k candidates smallest under (s, b) ascending, in that order; the tail is (+inf, -1)"""
    Q, B = s.shape
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    m = min(k, B)
    for q in range(Q):
        if B > 4 * k:
            # candidates: everything not above the k-th smallest score (ties included), then the stable order decides
            kth = np.partition(s[q], m - 1)[m - 1]
            cand = np.flatnonzero(s[q] <= kth)
        else:
            cand = np.arange(B)
        order = cand[np.argsort(s[q][cand], kind="stable")][:m]      # stable: equal scores stay in ascending position
        out_s[q, :m] = s[q][order]
        out_i[q, :m] = order
    return out_s, out_i


def restate(T, t, codes, k, qchunk=8):
    """rules 3 and 4 for all queries, a few at a time (the score matrix of a large store is not held whole)"""
    Q = T.shape[0]
    out_s = np.full((Q, k), np.inf, dtype=np.float32)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    if codes.shape[0] == 0:
        return out_s, out_i
    for a in range(0, Q, qchunk):
        s = restate_scores(T[a:a + qchunk], t, codes)
        out_s[a:a + qchunk], out_i[a:a + qchunk] = restate_topk(s, k)
    return out_s, out_i


# ------------------------------------------------------------------ the GPU cases
@dataclass(frozen=True)
class Case:
    name: str
    N: int
    K: int
    D: int
    Q: int
    B: int
    k: int
    state: str = "synthetic"        # "synthetic" | "trained" (tests/golden/trained_d512_b8_p2.npz) | "decode_only"
    codes: str = "encode"           # "encode" (Quantizer.encode of seeded frames) | "random" | "dup16" (16 distinct codes)
    queries: str = "gaussian"       # "gaussian" | "fp16" | "stored" (decodes of stored vectors: distance 0 occurs)
    packed: bool = False            # the store keeps encode's packed 16-entry codes
    tiles: bool = False             # claims: more than one query tile,
    sliced: bool = False            # more than one slice,
    partial: bool = False           # a last step of fewer than 64 candidates,
    short: bool = False             # fewer than k stored vectors,
    strided: bool = False           # a wave takes more than one step of its slice (its steps are kScanWaves apart, so the order
                                    # in which candidates reach the lists is no longer the order of their positions)


BIG = 1_048_576 + 17
CASES = [
    Case("trained_8x256_d512", 8, 256, 512, 200, 100_003, 10, state="trained", strided=True, tiles=True, sliced=True, partial=True),
    Case("big_8x256_d24_k64", 8, 256, 24, 17, BIG, 64, strided=True, tiles=True, sliced=True, partial=True),
    Case("n1_k16_one", 1, 16, 24, 1, 1, 1, partial=True),
    Case("n2_k64_b63", 2, 64, 24, 17, 63, 10, tiles=True, partial=True),
    Case("n2_k256_b63_k64", 2, 256, 24, 1, 63, 64, partial=True, short=True),          # B = k - 1
    Case("n16_k16_packed_b65", 16, 16, 512, 17, 65, 64, packed=True, tiles=True, partial=True),
    Case("n16_k64_short", 16, 64, 512, 200, 9, 10, tiles=True, partial=True, short=True),  # B = k - 1
    Case("n64_k256_decode_only", 64, 256, 24, 17, 100_003, 10, state="decode_only", codes="random", strided=True, tiles=True,
         sliced=True, partial=True),
    Case("n64_k16_b64", 64, 16, 24, 1, 64, 1, packed=True),
    Case("n1_k256_b64_k1", 1, 256, 512, 17, 64, 1, tiles=True),
    Case("dup16_k64", 8, 256, 24, 17, 4096, 64, codes="dup16", tiles=True, sliced=True),
    Case("dup16_strided_k64", 8, 256, 24, 200, 40_000, 64, codes="dup16", tiles=True, sliced=True, strided=True),
    Case("fp16_queries", 8, 64, 24, 17, 4099, 10, queries="fp16", tiles=True, sliced=True, partial=True),
    Case("decode_only_8x256", 8, 256, 512, 17, 4099, 10, state="decode_only", codes="random", tiles=True, sliced=True,
         partial=True),
    Case("stored_queries_clamp", 8, 16, 24, 17, 1000, 10, queries="stored", packed=True, tiles=True, sliced=True, partial=True),
    Case("n8_k256_q1_k1", 8, 256, 512, 1, 100_003, 1, sliced=True, partial=True),
    # dims whose padded dim is no multiple of kTabChunk (40 -> 48, 1000 -> 1008): the last chunk of k_search_tables is half a one
    Case("n8_k256_d40", 8, 256, 40, 17, 4099, 10, state="decode_only", codes="random", tiles=True, sliced=True, partial=True),
    Case("n2_k64_d1000", 2, 64, 1000, 5, 300, 10, partial=True),
]
