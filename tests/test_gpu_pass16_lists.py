"""The LDS-resident refinement pass (k_tf_pass16<N>: 8 x 16 and 16 x 16 codebooks, every pass of a call in one launch, the
candidate lists in wave-private LDS) level by level against the oracle's trace -- what tests/test_gpu_pass_lists.py does for the
separate kernels, which never run at these two shapes in an encode.

mcq_test_pass16 (include/mcq_probe.h) runs the encode's chunk start and launch_pass16 on caller-supplied codes.  With a dump buffer
it launches k_tf_pass16_probe<N> -- the same body, which also copies the wave's lists, E, R and the new codes into one record per
(vector, pass) -- and with dump = NULL the kernel the encode launches.  THE LISTS THEMSELVES ARE OBSERVED IN THE PROBE INSTANTIATION
ONLY; the shipping one is tied to it through its codes after 1, 2, 3 and 4 passes.  tests/pass16_lists.py decodes records and says,
from the oracle, which records must exist.  D = 32, at most 67 vectors (8 waves x 8 trips + 3 under max_workgroups = 1, where every
wave carries 8 or 9 vectors through the same 4 KB of LDS one after the other) and at most 4 passes.  Every comparison is bit for bit,
scores as uint32; dump, idx_out and workspace are 0xA5 before each call.

  lists        both shapes x (plain, ties, degenerate, graded), 1, 5 and 67 vectors, 3 passes (graded: 4), the launcher's grid and
               one workgroup: every record that must exist holds the oracle's E, R, ent, S[0], pos[v] and S[v] AS ORDERED ARRAYS and
               the pass's codes; every record past a vector's fixed point is still 0xA5 (the early exit is taken at the pass, not one
               later), and so is the dump past B * iters records; idx_out and the workspace's idx hold the last codes; the workspace
               outside idx, xx, XC and the frames' limb planes is untouched
  shipping     dump = NULL at both grids for 1 .. 4 passes: idx_out equals the probe's codes, the oracle's, and mcq_refine_indexes'
  carry-over   one workgroup, tie state, the vectors in reverse order: each vector's records are the ones it had, so no list entry
               depends on the vector the wave carried before
  non-finite   a row of NaN, one +inf, a row of -inf, a row of 1e30 among 67, one workgroup (each bad row shares its wave with later
               rows): through the shipping kernel of the probe and through Quantizer.encode (int64 and packed, skip_fixed_points
               both ways) every code is in [0, 16), the other rows are the oracle's, decode runs.  Only at these two shapes: in
               k_tf_pass16 no global address depends on data
  chunks       mcq_encode and mcq_logits_refine_codes over 300 vectors with a workspace for 130 (128 + 128 + 44): the same codes
               as in one chunk and as the oracle's, packed bytes and int64"""
import numpy as np
import pytest
import torch

import pass16_lists as p16
import pass_lists as pl
from test_gpu_pass_lists import assert_nothing_else_written

pytestmark = pytest.mark.gpu

D, K = p16.D, p16.K
FILL = p16.FILL
TAIL = 777                      # dump bytes past the last record
WRITTEN16 = ("idx", "xx", "XC", "xf", "xe")         # what the chunk start with imported codes and the LDS-resident pass write
UNUSED16 = tuple(a for a in pl.ARRAYS if a not in WRITTEN16)
LIST_ORDER = ("E", "R", "ent", "S0", "pos1", "S1", "pos2", "S2", "pos3", "S3", "idx")
BAD_ROWS = (3, 7, 9, 11)


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


def _quantizer(N, name):
    """the quantizer of (shape, state) and its prepared state, once"""
    key = (N, name)
    if key not in _Q:
        from quantization_amd import Quantizer
        state = p16.reference(N, name)["state"]
        q = Quantizer(D, K, N)
        sd = q.state_dict()
        for k, v in state.items():
            sd[k] = torch.from_numpy(np.asarray(v))
        q.load_state_dict(sd)
        q = q.to("cuda:0")
        _Q[key] = (q, q._prepared())
    return _Q[key]


_ORACLE = {}


def oracle_codes(N, name, iters):
    """the oracle's codes of the reference's 67 vectors after `iters` passes from the arg max of its logits"""
    key = (N, name, iters)
    if key not in _ORACLE:
        ref = p16.reference(N, name)
        _ORACLE[key] = pl.oracle_of(ref["state"]).compute_indexes(ref["x"], iters).astype(np.int64)
    return _ORACLE[key]


def _filled(nbytes):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda:0")


def _workspace(L, B, N):
    ws = torch.empty(L.mcq_encode_workspace_bytes(B, N, K, D), dtype=torch.uint8, device="cuda:0")
    assert ws.data_ptr() % 256 == 0
    return ws


def run16(L, blob, x, idx, N, iters, ws, lay=None, wgs=0, refine=False):
    """`iters` passes over a workspace, an idx_out and (lay given: the probe instantiation) a dump of 0xA5:
    (the workspace's bytes, idx_out, the dump's bytes or None).  refine: through mcq_refine_indexes instead"""
    B = x.shape[0]
    ws.fill_(FILL)
    xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    idx_in = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).cuda()
    idx_out = _filled(B * N * 8).view(torch.int64).reshape(B, N)
    dump = None if lay is None else _filled(B * iters * lay["rec"] + TAIL)
    if refine:
        rc = L.mcq_refine_indexes(xd.data_ptr(), B, blob.data_ptr(), N, K, D, iters, idx_in.data_ptr(), idx_out.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _st())
    else:
        rc = L.mcq_test_pass16(xd.data_ptr(), B, blob.data_ptr(), N, D, iters, idx_in.data_ptr(), idx_out.data_ptr(),
                               None if dump is None else dump.data_ptr(), 0 if dump is None else dump.numel(), wgs, ws.data_ptr(),
                               ws.numel(), _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return ws.cpu().numpy(), idx_out.cpu().numpy(), None if dump is None else dump.cpu().numpy()


def check_records(dump, lay, ref, N, rows, iters, what):
    """the dump of a call over the reference's vectors `rows` (device row r holds vector rows[r]) against the oracle: every
    record that must exist, array by array; fill in every other record, past the last one, and in the bytes of a record no lane
    writes.  Returns the decoded records"""
    rows = np.asarray(rows)
    nb, rec = len(rows), lay["rec"]
    assert dump.size == nb * iters * rec + TAIL
    assert (dump[nb * iters * rec:] == FILL).all(), (what, "written past the last record")
    recs = dump[:nb * iters * rec].reshape(nb, iters, rec)
    pres = p16.present(ref, p16.B, iters)[rows]
    got = p16.decode(recs, lay, N)
    late = np.argwhere((recs[~pres] != FILL).any(axis=-1))
    assert late.size == 0, (what, f"{len(late)} records past a fixed point were written, first (row, pass) "
                            f"{np.argwhere(~pres)[late[0, 0]].tolist()}")
    assert (got["mark"][pres] == p16.WRITTEN).all(), (what, "a record that must exist was not written",
                                                      np.argwhere(pres & (got["mark"] != p16.WRITTEN))[:4].tolist())
    assert set(got) - {"mark"} == set(ref["passes"][0]), (sorted(got), sorted(ref["passes"][0]))
    for p in range(iters):
        m = pres[:, p]
        for a in LIST_ORDER:
            if a not in got:
                continue
            g, w = got[a][m, p], ref["passes"][p][a][rows][m]
            bad = np.argwhere(g != w)
            assert bad.size == 0, (what, f"pass {p}", a, f"{len(bad)} of {w.size} differ, first at (row, ...) {bad[0].tolist()}: "
                                   f"{g[tuple(bad[0])]} for {w[tuple(bad[0])]}")
    at = lay["at"]
    for lo, hi in ((sum(at["R"]), at["idx"][0]), (sum(at["idx"]), at["mark"][0])):      # R[n], idx[n] of n >= N: no lane writes them
        assert (recs[..., lo:hi] == FILL).all(), (what, "bytes", lo, hi)
    return got


@pytest.mark.parametrize("wgs", (0, 1))
@pytest.mark.parametrize("name", p16.STATES)
@pytest.mark.parametrize("N,K_", p16.SHAPES)
def test_records_of_every_pass_equal_the_oracle(N, K_, name, wgs):
    L = _L()
    ref = p16.reference(N, name)
    _, blob = _quantizer(N, name)
    lay = p16.layout(L, N)
    iters = p16.passes_of(name)
    for B in p16.BATCHES:
        what = (N, name, B, f"max_workgroups {wgs}")
        ws = _workspace(L, B, N)
        raw, out, dump = run16(L, blob, ref["x"][:B], ref["start"][:B], N, iters, ws, lay, wgs)
        check_records(dump, lay, ref, N, np.arange(B), iters, what)
        want = p16.codes_after(ref, B, iters)
        assert np.array_equal(out, want), (what, "idx_out")
        carve = pl.layout(L, B, N, K)
        off, nbytes = carve["at"]["idx"]
        assert carve["cw"] == 1 and np.array_equal(raw[off:off + nbytes].reshape(B, N), want.astype(np.uint8)), (what, "workspace idx")
        assert_nothing_else_written(raw, carve, what, UNUSED16)


@pytest.mark.parametrize("name", p16.STATES)
@pytest.mark.parametrize("N,K_", p16.SHAPES)
def test_shipping_instantiation_gives_the_probes_codes(N, K_, name):
    """dump = NULL launches k_tf_pass16<N> itself, the kernel of every encode of these shapes.  Its lists are not observable (they
    are observed in the probe instantiation only, above); its codes after every number of passes are, and they are the probe's,
    the oracle's and those of mcq_refine_indexes, which reaches the kernel the way the trainer does"""
    L = _L()
    ref = p16.reference(N, name)
    _, blob = _quantizer(N, name)
    lay = p16.layout(L, N)
    B = p16.B
    ws = _workspace(L, B, N)
    x, start = ref["x"], ref["start"]
    for iters in (1, 2, 3, 4):
        want = oracle_codes(N, name, iters)
        if iters <= p16.passes_of(name):
            assert np.array_equal(want, p16.codes_after(ref, B, iters))
        _, refined, _ = run16(L, blob, x, start, N, iters, ws, refine=True)
        assert np.array_equal(refined, want), (N, name, iters, "mcq_refine_indexes")
        for wgs in (0, 1):
            _, probe, dump = run16(L, blob, x, start, N, iters, ws, lay, wgs)
            raw, ship, none = run16(L, blob, x, start, N, iters, ws, None, wgs)
            assert none is None and dump is not None
            assert np.array_equal(ship, probe), (N, name, iters, wgs, "the shipping kernel against the probe")
            assert np.array_equal(ship, want), (N, name, iters, wgs, "the shipping kernel against the oracle")
            assert_nothing_else_written(raw, pl.layout(L, B, N, K), (N, name, iters, wgs), UNUSED16)


@pytest.mark.parametrize("N,K_", p16.SHAPES)
def test_lists_do_not_depend_on_the_vector_before(N, K_):
    """one workgroup: wave w carries vectors w, w + 8, ... through the same scratch.  In reverse order every vector follows another
    one (and the three of the ragged last trip come first): its records are the same"""
    L = _L()
    ref = p16.reference(N, "ties")
    _, blob = _quantizer(N, "ties")
    lay = p16.layout(L, N)
    B, iters = p16.B, p16.passes_of("ties")
    ws = _workspace(L, B, N)
    fwd = check_records(run16(L, blob, ref["x"], ref["start"], N, iters, ws, lay, 1)[2], lay, ref, N, np.arange(B), iters, (N, "forward"))
    rows = np.arange(B)[::-1]
    _, out, dump = run16(L, blob, ref["x"][rows], ref["start"][rows], N, iters, ws, lay, 1)
    rev = check_records(dump, lay, ref, N, rows, iters, (N, "reversed"))
    pres = p16.present(ref, B, iters)
    for a in fwd:
        assert np.array_equal(rev[a][::-1][pres], fwd[a][pres]), (N, a)
    assert np.array_equal(out[::-1], p16.codes_after(ref, B, iters))


@pytest.mark.parametrize("N,K_", p16.SHAPES)
def test_non_finite_rows_give_codes_in_range_and_leave_their_neighbours(N, K_):
    L = _L()
    ref = p16.reference(N, "plain")
    q, blob = _quantizer(N, "plain")
    o = pl.oracle_of(ref["state"])
    B, iters = p16.B, p16.passes_of("plain")
    bad = ref["x"].copy()
    bad[3] = np.nan
    bad[7, 5] = np.inf
    bad[9] = -np.inf
    bad[11] = 1e30
    good = np.setdiff1d(np.arange(B), BAD_ROWS)
    want = p16.codes_after(ref, B, iters)
    ws = _workspace(L, B, N)
    _, out, _ = run16(L, blob, bad, ref["start"], N, iters, ws, None, 1)
    print(f"NON-FINITE {N} x {K}: probe codes of the bad rows {out[list(BAD_ROWS)].tolist()}")
    assert out.min() >= 0 and out.max() < K, (N, "probe", out.min(), out.max())
    assert np.array_equal(out[good], want[good]), (N, "probe")
    assert tuple(q.decode(torch.from_numpy(out).cuda()).shape) == (B, D)
    xd = torch.from_numpy(bad).cuda()
    packed_want = o.encode(ref["x"], iters)
    try:
        for skip in (False, True):
            q.skip_fixed_points = skip
            c = q.encode(xd, iters, as_bytes=False)
            y = q.decode(c)
            b = q.encode(xd, iters)
            yb = q.decode(b)
            torch.cuda.synchronize()
            c, b = c.cpu().numpy(), b.cpu().numpy()
            assert c.dtype == np.int64 and c.min() >= 0 and c.max() < K, (N, skip, c.min(), c.max())
            assert np.array_equal(c[good], want[good]), (N, skip)
            assert b.dtype == np.uint8 and b.shape == (B, N // 2)
            digits = np.stack([b & 15, b >> 4], axis=-1).reshape(B, N)
            assert digits.max() < K and np.array_equal(b[good], packed_want[good]), (N, skip, "packed")
            assert tuple(y.shape) == (B, D) and tuple(yb.shape) == (B, D)
            assert np.array_equal(y.cpu().numpy()[good], yb.cpu().numpy()[good])
    finally:
        q.skip_fixed_points = True


@pytest.mark.parametrize("N,K_", p16.SHAPES)
def test_chunks_of_128_give_the_codes_of_one_chunk(N, K_):
    """launch_pass16 gets the caller's arrays at the chunk's first vector and the chunk's own idx: 300 vectors as 128 + 128 + 44"""
    from quantization_amd import _lib
    L = _L()
    ref = p16.reference(N, "plain")
    q, blob = _quantizer(N, "plain")
    o = pl.oracle_of(ref["state"])
    B, iters = 300, 3
    x = pl.make_frames("plain", N, K, B)
    xd = torch.from_numpy(x).cuda()
    want, want_packed = o.compute_indexes(x, iters).astype(np.int64), o.encode(x, iters)
    small, whole = L.mcq_encode_workspace_bytes(130, N, K, D), L.mcq_encode_workspace_bytes(B, N, K, D)
    assert small < whole
    results = {}
    for nws in (whole, small):
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
        by = _filled(B * N // 2).reshape(B, N // 2)
        i64 = _filled(B * N * 8).view(torch.int64).reshape(B, N)
        rc = L.mcq_encode(xd.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, iters, by.data_ptr(), None, ws.data_ptr(), nws, _st())
        assert rc == 0, rc
        rc = L.mcq_encode(xd.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, iters, None, i64.data_ptr(), ws.data_ptr(), nws, _st())
        assert rc == 0, rc
        # the trainer's entry: the stored logits, int64 and unpacked bytes from the same launches
        logits = torch.empty((B, N * K), dtype=torch.float32, device="cuda:0")
        t64 = _filled(B * N * 8).view(torch.int64).reshape(B, N)
        tby = _filled(B * N).reshape(B, N)
        rc = L.mcq_logits_refine_codes(xd.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, iters, logits.data_ptr(), t64.data_ptr(),
                                       tby.data_ptr(), ws.data_ptr(), nws, _st(), q._scale_flags)
        _lib.check(rc, "mcq_logits_refine_codes")
        torch.cuda.synchronize()
        results[nws] = tuple(t.cpu().numpy() for t in (by, i64, t64, tby, logits))
    for nws, (by, i64, t64, tby, logits) in results.items():
        what = (N, "one chunk" if nws == whole else "chunks of 128")
        assert np.array_equal(i64, want) and np.array_equal(by, want_packed), what
        assert np.array_equal(t64, want) and np.array_equal(tby, want.astype(np.uint8)), what
        for got, one in zip((by, i64, t64, tby, logits), results[whole]):
            assert np.array_equal(got.view(np.uint8), one.view(np.uint8)), what
