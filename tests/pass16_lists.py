"""The reference side of the tests of the LDS-resident refinement pass (k_tf_pass16<N>, 8 x 16 and 16 x 16 codebooks; no device):
the records mcq_test_pass16 (include/mcq_probe.h) must leave, from the lists of tests/pass_lists.py.

The kernel keeps, per wave, exactly the arrays pass_lists.lists_of builds from OracleQuantizer.refine_trace -- for 16 x 16 ent [16][8],
pos1 [8][8][2], pos2 [4][16][2], pos3 [2][16][2] and S0 .. S3, for 8 x 16 one level less (the ladder (8, [(8, 8), (8, 16), (16, 16),
(16, 1)])) -- and its probe instantiation copies them, with E, R and the new codes, into one record per (vector, pass).  A wave
leaves a vector after the first pass that returns its input, so the records of later passes are never written.

  states   the three of pass_lists (plain, ties, degenerate) with pass_lists.reference as it is (67 vectors, 3 passes), and
           "graded": the plain state with codebook n's centers multiplied by float32(0.75 ** n), 4 passes -- its vectors stop at
           different passes (tests/test_pass16_lists_host.py asserts the spread)
"""
import ctypes

import numpy as np

import pass_lists as pl

D = pl.D
K = 16
SHAPES = [(8, K), (16, K)]
STATES = pl.STATES + ("graded",)
BATCHES = (1, 5, 67)
B = max(BATCHES)
GRADED_PASSES = 4
FILL = 0xA5
WRITTEN = 0x36315021            # MCQ_TEST_PASS16_WRITTEN

# the arrays of a record in the order mcq_test_pass16_layout reports them
ARRAYS = ("ent", "pos1", "pos2", "pos3", "S0", "S1", "S2", "S3", "E", "R", "idx", "mark")
LAYOUT_VALUES = 2 * len(ARRAYS) + 1
KC = (8, 8, 16, 16)             # the list length of levels 0 .. 3


def passes_of(name):
    return GRADED_PASSES if name == "graded" else pl.PASSES


def levels(N):
    """the levels that hold a list: 0 .. 3 for 16 codebooks, 0 .. 2 for 8 (the last combine keeps the winner only)"""
    return N.bit_length() - 1


def shapes_of(N):
    """array of a record -> (dtype as the device holds it, shape), for the arrays N codebooks have"""
    out = {"ent": (np.uint8, (N, KC[0])), "S0": (np.uint32, (N, KC[0])), "E": (np.uint32, ()), "R": (np.uint32, (N,)),
           "idx": (np.uint8, (N,)), "mark": (np.uint32, ())}
    for v in range(1, levels(N)):
        out[f"pos{v}"] = (np.uint8, (N >> v, KC[v], 2))
        out[f"S{v}"] = (np.uint32, (N >> v, KC[v]))
    return out


def layout(L, N):
    """mcq_test_pass16_layout as {"at": {array: (offset, bytes)}, "rec": bytes of a record}"""
    out = (ctypes.c_size_t * LAYOUT_VALUES)()
    n = L.mcq_test_pass16_layout(N, out, LAYOUT_VALUES)
    assert n == LAYOUT_VALUES, n
    v = list(out)
    return dict(at={name: (v[2 * i], v[2 * i + 1]) for i, name in enumerate(ARRAYS)}, rec=v[-1])


def decode(recs, lay, N):
    """records (uint8 [...][lay["rec"]]) -> the dict of pass_lists.lists_of with the leading axes kept, plus "mark".  Only the
    arrays N codebooks have: the rest of a record is scratch the kernel never wrote"""
    recs = np.asarray(recs, dtype=np.uint8)
    assert recs.shape[-1] == lay["rec"]
    out = {}
    for name, (dtype, shape) in shapes_of(N).items():
        off, nbytes = lay["at"][name]
        assert nbytes == int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, (N, name, nbytes)
        a = np.ascontiguousarray(recs[..., off:off + nbytes]).view(dtype).reshape(recs.shape[:-1] + shape)
        out[name] = a.astype(np.uint16) if name in ("ent", "idx") else a
    return out


def encode(lists, lay, N, fill=FILL):
    """the inverse of decode for one vector's lists (the dict of pass_lists.lists_of): a record over `fill`"""
    rec = np.full(lay["rec"], fill, np.uint8)
    for name, (dtype, shape) in shapes_of(N).items():
        off, nbytes = lay["at"][name]
        val = np.uint32(WRITTEN) if name == "mark" else lists[name]
        rec[off:off + nbytes] = np.ascontiguousarray(np.asarray(val).reshape(shape).astype(dtype)).view(np.uint8).reshape(-1)
    return rec


def make_graded_state(N):
    sd = pl.make_state("plain", N, K)
    for n in range(N):
        sd["centers"][n] *= np.float32(0.75 ** n)
    return sd


_REF = {}


def reference(N, name):
    """pass_lists.reference(N, 16, name) for its three states; the same dict (without ties and traces) for the graded one; plus
    "stop": for every vector the first pass (from 0) that returns its input, or the number of passes if none does, and
    "present" [B][passes]: the records the kernel must write, pass p <= stop"""
    key = (N, name)
    if key in _REF:
        return _REF[key]
    if name == "graded":
        sd = make_graded_state(N)
        x = pl.make_frames("plain", N, K, B)
        o = pl.oracle_of(sd)
        start = o.compute_indexes(x, 0).astype(np.uint16)
        idx, passes = start.copy(), []
        for _ in range(GRADED_PASSES):
            per = []
            for b in range(B):
                t = o.refine_trace(x[b], idx[b])
                want = pl.lists_of(t, N, K)
                assert np.array_equal(want["idx"], t["idx"]), (N, name, b)
                per.append(want)
                idx[b] = t["idx"]
            stacked = {k: np.stack([w[k] for w in per]) for k in per[0]}
            stacked["E"] = stacked["E"].reshape(B)
            passes.append(stacked)
        ref = dict(state=sd, x=x, start=start, passes=passes)
    else:
        ref = dict(pl.reference(N, K, name))
    P = len(ref["passes"])
    assert P == passes_of(name)
    stop = np.full(B, P, np.int64)
    cur = ref["start"].astype(np.uint16)
    for p in range(P):
        nxt = ref["passes"][p]["idx"].astype(np.uint16)
        same = (nxt == cur).all(axis=1)
        stop = np.where(same & (stop == P), p, stop)
        cur = nxt
    ref["stop"] = stop
    _REF[key] = ref
    return ref


def present(ref, nb, iters):
    """[nb][iters] bool: a call of `iters` passes writes the record of (b, p)"""
    return np.arange(iters)[None, :] <= ref["stop"][:nb, None]


def codes_after(ref, nb, iters):
    """the codes of the first nb vectors after `iters` passes (a pass past a fixed point returns it)"""
    return ref["passes"][iters - 1]["idx"][:nb].astype(np.int64)


def expected_records(ref, lay, N, nb, iters, fill=FILL):
    """uint8 [nb][iters][rec]: the oracle's lists where the record must exist, `fill` elsewhere -- and `fill` too in the bytes
    of a present record outside its arrays (compare through decode: those hold scratch)"""
    out = np.full((nb, iters, lay["rec"]), fill, np.uint8)
    pres = present(ref, nb, iters)
    for p in range(iters):
        for b in range(nb):
            if pres[b, p]:
                out[b, p] = encode({k: v[b] for k, v in ref["passes"][p].items()}, lay, N, fill)
    return out
