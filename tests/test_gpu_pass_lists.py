"""The candidate lists of a refinement pass, level by level, against the oracle's trace -- not only the winner's code.

mcq_test_pass (include/mcq_probe.h) runs ONE pass of B vectors as one chunk through the pass loop's own launchers and leaves the
workspace as the pass left it; mcq_test_pass_layout says where carve() put every array.  tests/pass_lists.py turns
OracleQuantizer.refine_trace into the arrays the device must hold.  D = 32; the shapes are chosen so that every kernel family of
run_tf_combines writes a list that is read back (pass_lists.SHAPES; 8 x 16 and 16 x 16 reach the separate kernels only here: the
encode takes the LDS-resident pass), with 1, 5 and 67 vectors (21 for 32 and 64 codebooks).

  per shape and state   plain (gen.synthetic_state), ties (its center rows repeated with a period that does not divide the list
                        length: a tie on the boundary of most lists of every level, tests/test_pass_lists_host.py asserts the
                        share) and degenerate (all centers equal, frames of zeros: every score ties).  From the arg max of the
                        oracle's logits, three passes, one probe call each, the device's own codes fed back in, the whole
                        workspace filled with 0xA5 before each call.  After each pass, bit for bit: E, R, ent, S[0], pos[v] and
                        S[v] of every level with a list AS ORDERED ARRAYS, the new codes in the workspace's idx and in idx_out;
                        every byte between two arrays and past the last one is still 0xA5, and so are the arrays a pass without
                        skipping does not use
  packed slots          nact = B - 3 and a permutation as map (4 x 64, 8 x 256, 16 x 32, 8 x 512): slot s holds what row map[s]
                        of the unmapped call held, slots >= nact keep 0xA5 in every list array; with MCQ_TEST_PASS_CAPPED too
                        at 8 x 256 and 16 x 32 (the grid-stride instantiations, one trip)
  the encode's path     mcq_refine_indexes(refine_iters = 1) on the same inputs leaves E, R, the list arrays and idx byte-equal
                        to the probe's, with the same number of launches (every shape but the two pass16 ones)"""
import numpy as np
import pytest
import torch

import pass_lists as pl

pytestmark = pytest.mark.gpu

D = pl.D
FILL = 0xA5
CAPPED = 1
PACKED_SHAPES = [(4, 64), (8, 256), (16, 32), (8, 512)]
CAPPED_SHAPES = [(8, 256), (16, 32)]
UNUSED = ("idxB", "idxC", "final_idx", "map0", "map1", "cnt", "gterms")     # without skipping, up to 8,192 vectors


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _L():
    from quantization_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


_Q = {}


def _blob(N, K, name):
    """the prepared state of (shape, state), once"""
    key = (N, K, name)
    if key not in _Q:
        from quantization_amd import Quantizer
        state = pl.reference(N, K, name)["state"]
        q = Quantizer(D, K, N)
        sd = q.state_dict()
        for k, v in state.items():
            sd[k] = torch.from_numpy(np.asarray(v))
        q.load_state_dict(sd)
        q = q.to("cuda:0")
        _Q[key] = (q, q._prepared())
    return _Q[key][1]


def _workspace(L, B, N, K):
    nws = L.mcq_encode_workspace_bytes(B, N, K, D)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
    assert ws.data_ptr() % 256 == 0
    return ws


def run_pass(L, blob, x, idx, N, K, ws, nact=None, map_=None, flags=0, encode=False):
    """one pass over a workspace of 0xA5: (the workspace's bytes, idx_out, launches).  encode: through mcq_refine_indexes"""
    B = x.shape[0]
    ws.fill_(FILL)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    idx_in = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    idx_out = torch.full((B, N), -7, dtype=torch.int64, device="cuda:0")
    nact_d = None if nact is None else torch.tensor([nact], dtype=torch.int32, device="cuda:0")
    map_d = None if map_ is None else torch.from_numpy(np.ascontiguousarray(map_, dtype=np.int32)).cuda()
    if encode:
        rc = L.mcq_refine_indexes(xd.data_ptr(), B, blob.data_ptr(), N, K, D, 1, idx_in.data_ptr(), idx_out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _st())
    else:
        rc = L.mcq_test_pass(xd.data_ptr(), B, blob.data_ptr(), N, K, D, idx_in.data_ptr(), idx_out.data_ptr(),
                             None if nact_d is None else nact_d.data_ptr(), None if map_d is None else map_d.data_ptr(), flags,
                             ws.data_ptr(), ws.numel(), _st())
    n = L.mcq_last_encode_launches()
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ws.cpu().numpy(), idx_out.cpu().numpy(), n


def arrays_of(raw, lay, B, N):
    """the arrays of pass_lists.lists_of, read from the workspace's bytes: scores as uint32, entries in their own width"""
    at, kc, cw = lay["at"], lay["kc"], lay["cw"]
    code = np.uint16 if cw == 2 else np.uint8

    def get(name, dtype, shape):
        off, nbytes = at[name]
        a = raw[off:off + nbytes].view(dtype)
        assert a.size == int(np.prod(shape)), (name, a.size, shape)
        return a.reshape(shape)

    out = {"E": get("E", np.uint32, (B,)), "R": get("R", np.uint32, (B, N)), "idx": get("idx", code, (B, N)),
           "ent": get("ent", code, (B, N, kc[0])), "S0": get("S0", np.uint32, (B, N, kc[0]))}
    for v in range(1, 6):
        if at[f"S{v}"][1]:
            out[f"pos{v}"] = get(f"pos{v}", np.uint8, (B, N >> v, kc[v], 2))
            out[f"S{v}"] = get(f"S{v}", np.uint32, (B, N >> v, kc[v]))
    return out


def assert_nothing_else_written(raw, lay, what, unused=UNUSED):
    end = 0
    for name in pl.CARVE_ORDER:
        off, nbytes = lay["at"][name]
        if nbytes == 0:
            continue
        assert (raw[end:off] == FILL).all(), (what, "before", name)
        if name in unused:
            assert (raw[off:off + nbytes] == FILL).all(), (what, name)
        end = off + nbytes
    assert end <= lay["total"] <= raw.size and (raw[end:] == FILL).all(), (what, "past the last array")


@pytest.mark.parametrize("name", pl.STATES)
@pytest.mark.parametrize("N,K", pl.SHAPES)
def test_lists_of_three_passes_equal_the_oracle(N, K, name):
    L = _L()
    ref = pl.reference(N, K, name)
    blob = _blob(N, K, name)
    for B in pl.batches(N):
        lay = pl.layout(L, B, N, K)
        ws = _workspace(L, B, N, K)
        assert lay["total"] <= ws.numel()
        idx = ref["start"][:B].astype(np.int64)
        for p in range(pl.PASSES):
            raw, idx, _ = run_pass(L, blob, ref["x"][:B], idx, N, K, ws)
            got, want = arrays_of(raw, lay, B, N), ref["passes"][p]
            assert set(got) == set(want), (sorted(got), sorted(want))
            for a in ("E", "R", "ent", "S0") + tuple(sorted(set(got) - {"E", "R", "ent", "S0", "idx"})) + ("idx",):
                w = want[a][:B]
                bad = np.argwhere(got[a] != w)
                assert bad.size == 0, (N, K, name, B, f"pass {p}", a, f"{len(bad)} of {w.size} differ, first at {bad[0].tolist()}: "
                                       f"{got[a][tuple(bad[0])]} for {w[tuple(bad[0])]}")
            assert np.array_equal(idx, want["idx"][:B].astype(np.int64)), (N, K, name, B, p, "idx_out")
            assert_nothing_else_written(raw, lay, (N, K, name, B, p))


@pytest.mark.parametrize("N,K,flags", [s + (0,) for s in PACKED_SHAPES] + [s + (CAPPED,) for s in CAPPED_SHAPES])
def test_packed_slots(N, K, flags):
    L = _L()
    ref = pl.reference(N, K, "ties")
    blob = _blob(N, K, "ties")
    B = max(pl.batches(N))
    nact = B - 3
    perm = np.random.RandomState(31 + N + K).permutation(B).astype(np.int32)
    lay, ws = pl.layout(L, B, N, K), _workspace(L, B, N, K)
    x, start = ref["x"][:B], ref["start"][:B].astype(np.int64)
    raw0, out0, _ = run_pass(L, blob, x, start, N, K, ws)
    full = arrays_of(raw0, lay, B, N)
    if flags:       # the capped launchers on every slot first: the same workspace as the plain ones, byte for byte in every list
        rawc, outc, _ = run_pass(L, blob, x, start, N, K, ws, flags=flags)
        capped = arrays_of(rawc, lay, B, N)
        for a in full:
            assert np.array_equal(capped[a], full[a]), (N, K, "capped", a)
        assert np.array_equal(outc, out0)
        assert_nothing_else_written(rawc, lay, (N, K, "capped"))
    raw, out, _ = run_pass(L, blob, x, start[perm], N, K, ws, nact=nact, map_=perm, flags=flags)
    got = arrays_of(raw, lay, B, N)
    for a in full:
        assert np.array_equal(got[a][:nact], full[a][perm[:nact]]), (N, K, flags, a)
        if a == "idx":          # (imported for every slot, refined in the active ones)
            assert np.array_equal(got[a][nact:], start[perm[nact:]].astype(got[a].dtype))
        else:
            tail = np.ascontiguousarray(got[a][nact:]).view(np.uint8)
            assert (tail == FILL).all(), (N, K, flags, a, "a slot past nact was written")
    assert np.array_equal(out[perm[:nact]], out0[perm[:nact]]) and (out[perm[nact:]] == -7).all()
    assert_nothing_else_written(raw, lay, (N, K, flags, "packed"))


@pytest.mark.parametrize("N,K", [s for s in pl.SHAPES if s not in ((8, 16), (16, 16))])
def test_encode_leaves_the_probes_lists(N, K):
    L = _L()
    ref = pl.reference(N, K, "ties")
    blob = _blob(N, K, "ties")
    B = max(pl.batches(N))
    lay, ws = pl.layout(L, B, N, K), _workspace(L, B, N, K)
    x, start = ref["x"][:B], ref["start"][:B].astype(np.int64)
    raw_p, out_p, n_p = run_pass(L, blob, x, start, N, K, ws)
    raw_e, out_e, n_e = run_pass(L, blob, x, start, N, K, ws, encode=True)
    for a in ("idx", "E", "R", "xx", "XC") + pl.LIST_ARRAYS:
        off, nbytes = lay["at"][a]
        assert np.array_equal(raw_e[off:off + nbytes], raw_p[off:off + nbytes]), (N, K, a)
    assert np.array_equal(out_e, out_p) and np.array_equal(out_e, ref["passes"][0]["idx"][:B].astype(np.int64))
    assert n_e == n_p, (n_e, n_p)
    assert_nothing_else_written(raw_e, lay, (N, K, "encode"))
