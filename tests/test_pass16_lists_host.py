"""Host-side checks behind tests/test_gpu_pass16_lists.py (no GPU).

  records     pass16_lists.decode of a record built from the oracle's lists gives those lists back, for 16 and for 8 codebooks
              (which have no pos3 / S3: not decoded); the expected records hold the lists up to a vector's fixed point and fill past it
  coverage    conditions on the inputs, from the oracle alone: of the 67 graded vectors of each shape at least a tenth leave before
              the last of the four passes and at least a tenth run all four (seen: the first pass that returns its input is, counted
              from 0, pass 1 / 2 / 3 or none for 27 / 30 / 10 vectors at 8 x 16 and 11 / 46 / 10 at 16 x 16), so a wave under max_workgroups = 1
              carries vectors that stop at different passes one after the other; the tie state keeps a tie on the boundary of at
              least a quarter of the lists of every level (the floor of tests/test_pass_lists_host.py; seen 97 to 100 %)
  probes      mcq_test_pass16_layout and mcq_test_pass16 of include/mcq_probe.h: declared as _lib.PROBE_SIGNATURES binds them, the
              record layout against the shapes of the arrays, the argument checks in the documented order (fake pointers, nothing
              launches)"""
import ctypes

import numpy as np
import pytest

import pass16_lists as p16
import pass_lists as pl
from test_pass_lists_host import FLOOR

NEW = ("mcq_test_pass16_layout", "mcq_test_pass16")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


# ------------------------------------------------------------------------------------------------------------------ the records
@pytest.mark.parametrize("N,K", p16.SHAPES)
def test_record_layout_holds_the_arrays(N, K):
    lay = p16.layout(_lib().lib(), N)
    at, rec = lay["at"], lay["rec"]
    assert rec % 4 == 0 and rec == p16.layout(_lib().lib(), 24 - N)["rec"]          # one record size for both shapes
    shapes = p16.shapes_of(N)
    end = 0
    for name in p16.ARRAYS:
        off, nbytes = at[name]
        if name not in shapes:
            assert (off, nbytes) == (0, 0) and N == 8 and name in ("pos3", "S3")
            continue
        dtype, shape = shapes[name]
        assert nbytes == int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize, (N, name)
        assert off >= end and off % np.dtype(dtype).itemsize == 0 and off + nbytes <= rec, (N, name)     # in order, no overlap
        end = off + nbytes
    if N == 16:     # the scratch of the kernel as DESIGN.md gives it: the lists start the record as they lie
        assert [at[a][0] for a in p16.ARRAYS[:8]] == [0, 128, 256, 384, 512, 1024, 1280, 1536]


@pytest.mark.parametrize("name", p16.STATES)
@pytest.mark.parametrize("N,K", p16.SHAPES)
def test_decode_gives_the_lists_back(N, K, name):
    lay = p16.layout(_lib().lib(), N)
    ref = p16.reference(N, name)
    iters = p16.passes_of(name)
    recs = p16.expected_records(ref, lay, N, p16.B, iters)
    got = p16.decode(recs, lay, N)
    pres = p16.present(ref, p16.B, iters)
    assert pres[:, 0].all() and set(got) == set(ref["passes"][0]) | {"mark"}
    assert ("pos3" in got) == (N == 16) and ("S3" in got) == (N == 16)
    for p in range(iters):
        for a, want in ref["passes"][p].items():
            assert got[a][:, p].shape == want.shape, (a, got[a].shape, want.shape)
            assert np.array_equal(got[a][pres[:, p], p], want[pres[:, p]]), (N, name, p, a)
        assert (got["mark"][pres[:, p], p] == p16.WRITTEN).all()
        assert (recs[~pres[:, p], p] == p16.FILL).all()
    # past a fixed point the oracle's passes return their input: the codes after `iters` passes are the last record's
    for it in range(1, iters + 1):
        last = np.minimum(ref["stop"], it - 1)
        assert np.array_equal(got["idx"][np.arange(p16.B), last].astype(np.int64), p16.codes_after(ref, p16.B, it))


def test_decode_reads_every_byte_of_an_array_once():
    """a record of distinct bytes: every array decodes to its own bytes, in order"""
    L = _lib().lib()
    for N, _ in p16.SHAPES:
        lay = p16.layout(L, N)
        rec = (np.arange(lay["rec"]) * 131 % 251).astype(np.uint8)
        got = p16.decode(rec, lay, N)
        for name, (dtype, shape) in p16.shapes_of(N).items():
            off, nbytes = lay["at"][name]
            want = rec[off:off + nbytes].view(dtype).reshape(shape)
            assert np.array_equal(got[name], want), (N, name)
        again = p16.encode(got, lay, N)
        mask = np.zeros(lay["rec"], bool)
        for name in p16.shapes_of(N):
            if name != "mark":
                mask[lay["at"][name][0]:sum(lay["at"][name])] = True
        assert np.array_equal(again[mask], rec[mask]) and (again[~mask][:-4] == p16.FILL).all()


# ----------------------------------------------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("N,K", p16.SHAPES)
def test_graded_vectors_stop_at_different_passes(N, K):
    ref = p16.reference(N, "graded")
    stop, P = ref["stop"], p16.GRADED_PASSES
    counts = np.bincount(stop, minlength=P + 1)
    print(f"FIRST PASS THAT RETURNS ITS INPUT {N} x {K} (pass 0 .. {P - 1}, none): {counts.tolist()}")
    assert stop.size == p16.B == 67
    early = int((stop < P - 1).sum())            # the wave breaks before the last pass
    full = int((stop >= P - 1).sum())            # the wave runs all four
    assert 10 * early >= p16.B, (N, counts)
    assert 10 * full >= p16.B, (N, counts)
    # and the three states of pass_lists are the ones its own host tests look at, unchanged
    for name in pl.STATES:
        r = p16.reference(N, name)
        assert r["passes"] is pl.reference(N, K, name)["passes"] and len(r["passes"]) == pl.PASSES


@pytest.mark.parametrize("N,K", p16.SHAPES)
def test_tie_state_keeps_its_boundary_ties(N, K):
    ref = pl.reference(N, K, "ties")
    for p, ties in enumerate(ref["ties"]):
        assert len(ties) == p16.levels(N)
        for v, (hit, lists) in enumerate(ties):
            print(f"BOUNDARY TIES {N} x {K} pass {p} level {v}: {hit} of {lists}")
            assert lists == p16.B * (N >> v) and hit >= FLOOR * lists, (N, p, v, hit, lists)


# ------------------------------------------------------------------------------------------------------------------ the probes
def test_probes_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    from test_er_probe_host import PROBE_HDR
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(PROBE_HDR)
    assert tuple(hdr)[-2:] == NEW == m.PROBE_SYMBOLS[-2:]
    assert ab.mismatches(hdr, m.PROBE_SIGNATURES) == []
    assert not set(NEW) & set(m.SYMBOLS) and not set(NEW) & set(ab.header_signatures())       # include/mcq.h keeps its table
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.PROBE_SIGNATURES[name][1])
    P = ab.POINTER
    assert hdr["mcq_test_pass16_layout"] == (ctypes.c_int, (ctypes.c_int, P, ctypes.c_int))
    # x, B, prepared, N as mcq_test_pass has them, then D, iters (no K: 16), idx_in, idx_out; the workspace and stream last
    a, b = m.PROBE_SIGNATURES["mcq_test_pass16"][1], m.PROBE_SIGNATURES["mcq_test_pass"][1]
    assert a[:4] == b[:4] and a[4:6] == (ctypes.c_int, ctypes.c_int) and a[6:8] == b[6:8] and a[-3:] == b[-3:]
    assert a[8:11] == (ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int)
    text = open(PROBE_HDR).read()
    assert f"#define MCQ_TEST_PASS16_LAYOUT_VALUES {p16.LAYOUT_VALUES}" in text
    assert f"#define MCQ_TEST_PASS16_WRITTEN 0x{p16.WRITTEN:08x}u" in text
    assert L.mcq_abi_version() == 7


def test_layout_argument_checks():
    m = _lib()
    L = m.lib()
    out = (ctypes.c_size_t * p16.LAYOUT_VALUES)()
    for N in (0, 1, 3, 4, 32, 64, -8):
        assert L.mcq_test_pass16_layout(N, out, p16.LAYOUT_VALUES) == m.MCQ_EUNSUPPORTED, N
    assert L.mcq_test_pass16_layout(4, None, -1) == m.MCQ_EUNSUPPORTED
    assert L.mcq_test_pass16_layout(8, None, 25) == m.MCQ_EINVAL and L.mcq_test_pass16_layout(16, out, -1) == m.MCQ_EINVAL
    out[3] = 77
    assert L.mcq_test_pass16_layout(16, out, 3) == p16.LAYOUT_VALUES and out[3] == 77 and out[1] == 16 * 8       # cap is honoured


def test_pass16_probe_argument_checks_in_order():
    m = _lib()
    L = m.lib()
    X, P, IDX, WS, DUMP = 1 << 20, 1 << 21, 1 << 22, 1 << 23, 1 << 24          # fake device pointers; never dereferenced
    big = 1 << 40
    rec = p16.layout(L, 16)["rec"]

    def call(N=16, D=32, B=5, iters=3, x=X, prepared=P, idx_in=IDX, idx_out=IDX, dump=DUMP, dump_bytes=big, wgs=0, ws=WS, nbytes=big):
        return L.mcq_test_pass16(x, B, prepared, N, D, iters, idx_in, idx_out, dump, dump_bytes, wgs, ws, nbytes, None)

    assert call(N=3) == m.MCQ_EINVAL and call(N=3, B=-1, iters=0) == m.MCQ_EINVAL          # the domain first, as the encode
    assert call(N=128, B=-1) == m.MCQ_EUNSUPPORTED and call(D=1 << 20, B=-1) == m.MCQ_EUNSUPPORTED
    for N in (1, 2, 4, 32, 64):                                       # shapes the encode has, the LDS-resident pass has not
        assert call(N=N, B=-1) == m.MCQ_EUNSUPPORTED, N
    assert call(B=-1) == m.MCQ_EINVAL and call(iters=0) == m.MCQ_EINVAL and call(iters=61) == m.MCQ_EINVAL
    assert call(wgs=-1) == m.MCQ_EINVAL and call(iters=-1, B=0) == m.MCQ_EINVAL
    assert call(B=0, x=None, prepared=None, idx_in=None, idx_out=None, dump=None, dump_bytes=0, ws=None, nbytes=0) == 0
    for null in ("x", "prepared", "idx_in", "idx_out", "ws"):
        assert call(**{null: None}) == m.MCQ_EINVAL, null
    assert call(ws=WS + 128) == m.MCQ_EINVAL and call(dump=DUMP + 2) == m.MCQ_EINVAL
    for N, B in ((8, 5), (16, 67)):
        need = L.mcq_encode_workspace_bytes(B, N, 16, 32)
        assert call(N=N, B=B, nbytes=need - 1) == m.MCQ_EWORKSPACE and call(N=N, B=B + 1, nbytes=need) == m.MCQ_EWORKSPACE
        assert call(N=N, B=B, nbytes=need - 1, ws=WS + 128) == m.MCQ_EINVAL        # alignment before the workspace's size
        assert call(N=N, B=B, nbytes=need - 1, dump_bytes=0) == m.MCQ_EWORKSPACE
        for iters in (1, 4):
            assert call(N=N, B=B, iters=iters, dump_bytes=B * iters * rec - 1) == m.MCQ_EWORKSPACE
    assert call(nbytes=0) == m.MCQ_EWORKSPACE and call(dump_bytes=0) == m.MCQ_EWORKSPACE
