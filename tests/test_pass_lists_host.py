"""Host-side checks behind tests/test_gpu_pass_lists.py (no GPU).

  selection   the oracle's trace against DESIGN.md section 2(d), by brute force: for every stage-0 row and every combine block of
              the kept traces, the kout smallest by (value, position) -- lowest position on equal values --, listed in ascending
              position, are sel_pos / sel_val.  On the plain, the tie and the degenerate state of every shape
  coverage    from the oracle alone: on the tie state of every shape of the GPU table, in every pass, at least a quarter of the
              lists of every level have a value outside the list equal to the list's largest kept value (half the lowest share
              measured when the periods were chosen, 56 %); on the plain state none has (which is why the code-parity tests never
              see the boundary rule); on the degenerate state every list has, and every list is the positions 0 .. kc - 1
  probes      mcq_test_pass_layout and mcq_test_pass of include/mcq_probe.h: declared as _lib.PROBE_SIGNATURES binds them, the
              argument checks in the documented order (fake pointers, nothing launches), and the layout itself: carve's order,
              256-byte offsets, the sizes of the arrays the tests read, inside the workspace the encode asks for"""
import ctypes

import numpy as np
import pytest

import pass_lists as pl

FLOOR = 0.25


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def brute_select(scores, kout):
    """section 2(d) restated: the kout smallest by (value, position), in ascending position"""
    order = np.lexsort((np.arange(scores.size), scores))[:kout]
    pos = np.sort(order)
    return pos, scores[pos]


def test_brute_select_is_the_rule():
    s = np.array([3, 1, 2, 1, 2, 2, 0, 2], np.float32)
    pos, val = brute_select(s, 4)
    assert pos.tolist() == [1, 2, 3, 6] and val.tolist() == [1, 2, 1, 0]       # of the four 2s the lowest position, listed by position
    assert brute_select(s, 1)[0].tolist() == [6] and brute_select(np.zeros(9, np.float32), 3)[0].tolist() == [0, 1, 2]


@pytest.mark.parametrize("name", pl.STATES)
@pytest.mark.parametrize("N,K", pl.SHAPES)
def test_trace_selects_by_value_then_position(N, K, name):
    ref = pl.reference(N, K, name)
    assert len(ref["traces"]) == pl.PASSES * pl.KEPT_TRACES
    seen = 0
    for t in ref["traces"]:
        for v, g, scores, kin, kout, pos, val in pl.blocks(t, N, K):
            want_pos, want_val = brute_select(scores, kout)
            assert np.array_equal(pos, want_pos), (N, K, name, v, g)
            assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32)), (N, K, name, v, g)
            seen += 1
    assert seen == len(ref["traces"]) * (2 * N - 1)          # N stage-0 rows and N - 1 combines per trace


@pytest.mark.parametrize("N,K", pl.SHAPES)
def test_tie_state_puts_ties_on_the_boundaries(N, K):
    assert (8 if K == 16 else 16) % pl.PERIODS[K] != 0 and pl.PERIODS[K] < K
    ref = pl.reference(N, K, "ties")
    for p, ties in enumerate(ref["ties"]):
        assert len(ties) == max(1, N.bit_length() - 1)                  # one entry per level that holds a list
        for v, (hit, lists) in enumerate(ties):
            print(f"BOUNDARY TIES {N} x {K} pass {p} level {v}: {hit} of {lists}")
            assert lists == max(pl.batches(N)) * (N >> v)
            assert hit >= FLOOR * lists, (N, K, p, v, hit, lists)


@pytest.mark.parametrize("N,K", pl.SHAPES)
def test_plain_state_has_no_boundary_tie(N, K):
    """a record, not a requirement of the code: random centers put no tie on any boundary (0 of every level's lists in all 16
    shapes), so nothing that compares winners on such inputs sees the boundary rule"""
    for p, ties in enumerate(pl.reference(N, K, "plain")["ties"]):
        print(f"BOUNDARY TIES plain {N} x {K} pass {p}: {[tuple(t) for t in ties]}")
        assert all(hit == 0 for hit, _ in ties)


@pytest.mark.parametrize("N,K", pl.SHAPES)
def test_degenerate_state_keeps_the_first_positions(N, K):
    ref = pl.reference(N, K, "degenerate")
    first, lad = pl.ladder(N, K)
    for want, ties in zip(ref["passes"], ref["ties"]):
        assert all(hit == lists for hit, lists in ties)
        assert (want["ent"] == np.arange(first)).all() and (want["idx"] == 0).all()
        for v, (kin, kout) in enumerate(lad[:-1], start=1):
            p = np.arange(kout)
            assert (want[f"pos{v}"] == np.stack([p // kin, p % kin], axis=1)).all()
            assert (want[f"S{v}"] == want[f"S{v}"][0, 0, 0]).all()


# ------------------------------------------------------------------------------------------------------------------ the probes
NEW = ("mcq_test_pass_layout", "mcq_test_pass")


def test_probes_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    from test_er_probe_host import PROBE_HDR
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(PROBE_HDR)
    # (after them: the probe of the LDS-resident pass, tests/test_pass16_lists_host.py)
    assert tuple(hdr)[-4:-2] == NEW == m.PROBE_SYMBOLS[-4:-2]
    assert ab.mismatches(hdr, m.PROBE_SIGNATURES) == []
    assert not set(NEW) & set(m.SYMBOLS) and not set(NEW) & set(ab.header_signatures())       # include/mcq.h keeps its table
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.PROBE_SIGNATURES[name][1])
    P = ab.POINTER
    assert hdr["mcq_test_pass_layout"] == (ctypes.c_int, (ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, ctypes.c_int))
    # x, B, prepared, N, K, D, idx_in, idx_out as mcq_refine_indexes has them (without its refine_iters)
    a, b = m.PROBE_SIGNATURES["mcq_test_pass"][1], m.SIGNATURES["mcq_refine_indexes"][1]
    assert a[:6] == b[:6] and a[6:8] == b[7:9] and a[10] is ctypes.c_uint and a[-3:] == b[-3:]
    text = open(PROBE_HDR).read()
    assert "#define MCQ_TEST_PASS_CAPPED 1u" in text and f"#define MCQ_TEST_PASS_LAYOUT_VALUES {pl.LAYOUT_VALUES}" in text


def test_pass_probe_argument_checks_in_order():
    m = _lib()
    L = m.lib()
    X, P, IDX, WS = 1 << 20, 1 << 21, 1 << 22, 1 << 23            # fake device pointers; never dereferenced
    big = 1 << 40

    def call(N=8, K=256, D=32, B=5, x=X, prepared=P, idx_in=IDX, idx_out=IDX, flags=0, ws=WS, nbytes=big):
        return L.mcq_test_pass(x, B, prepared, N, K, D, idx_in, idx_out, None, None, flags, ws, nbytes, None)

    assert call(N=3) == m.MCQ_EINVAL and call(N=3, B=-1, flags=6) == m.MCQ_EINVAL and call(K=2048, B=-1) == m.MCQ_EUNSUPPORTED
    assert call(N=128, K=16) == m.MCQ_EUNSUPPORTED and call(N=32, K=1024) == m.MCQ_EUNSUPPORTED    # the domain first, as the encode
    assert call(N=1, B=-1) == m.MCQ_EUNSUPPORTED                       # one codebook has no lists
    assert call(B=-1) == m.MCQ_EINVAL and call(flags=2) == m.MCQ_EINVAL and call(flags=3, B=0) == m.MCQ_EINVAL
    assert call(B=0, x=None, prepared=None, idx_in=None, idx_out=None, ws=None, nbytes=0) == 0      # an empty call looks at nothing
    for null in ("x", "prepared", "idx_in", "idx_out", "ws"):
        assert call(**{null: None}) == m.MCQ_EINVAL, null
    assert call(ws=WS + 128) == m.MCQ_EINVAL
    for N, K, B in ((8, 256, 5), (64, 32, 21), (4, 1024, 67)):
        need = L.mcq_encode_workspace_bytes(B, N, K, 32)
        assert call(N=N, K=K, B=B, nbytes=need - 1) == m.MCQ_EWORKSPACE and call(N=N, K=K, B=B + 1, nbytes=need) == m.MCQ_EWORKSPACE
        assert call(N=N, K=K, B=B, nbytes=need - 1, ws=WS + 128) == m.MCQ_EINVAL        # alignment before the workspace's size
    assert call(nbytes=0) == m.MCQ_EWORKSPACE


def test_layout_argument_checks():
    m = _lib()
    L = m.lib()
    out = (ctypes.c_size_t * pl.LAYOUT_VALUES)()
    assert L.mcq_test_pass_layout(5, 3, 256, 32, out, 64) == m.MCQ_EINVAL and L.mcq_test_pass_layout(0, 8, 2048, 32, None, -1) == m.MCQ_EUNSUPPORTED
    assert L.mcq_test_pass_layout(0, 8, 256, 32, out, 64) == m.MCQ_EINVAL and L.mcq_test_pass_layout(-1, 8, 256, 32, out, 64) == m.MCQ_EINVAL
    assert L.mcq_test_pass_layout(5, 8, 256, 32, None, 64) == m.MCQ_EINVAL and L.mcq_test_pass_layout(5, 8, 256, 32, out, -1) == m.MCQ_EINVAL
    out[3] = 77
    assert L.mcq_test_pass_layout(5, 8, 256, 32, out, 3) == pl.LAYOUT_VALUES and out[3] == 77 and out[1] == 5 * 8       # cap is honoured


@pytest.mark.parametrize("N,K", pl.SHAPES + [(1, 16), (16, 256), (64, 256), (32, 512)])
def test_layout_is_carves(N, K):
    L = _lib().lib()
    first, lad = pl.ladder(N, K) if N > 1 else (0, [])
    nlev = max(0, N.bit_length() - 1)
    for B in (1, 5, 67, 300):
        lay = pl.layout(L, B, N, K)
        at, kc, cw = lay["at"], lay["kc"], lay["cw"]
        assert cw == (2 if K > 256 else 1)
        # the list lengths are the oracle's ladder: level v holds what step v - 1 keeps and what step v takes in
        if N > 1:
            assert kc[0] == first and [kc[v] for v in range(nlev)] == [kin for kin, _ in lad]
            assert [kc[v] for v in range(1, nlev)] == [kout for _, kout in lad[:-1]]
        want = {"idx": B * N * cw, "idxB": B * N * cw, "idxC": B * N * cw, "final_idx": B * N * cw, "map0": 4 * B, "map1": 4 * B,
                "cnt": 256, "E": 4 * B, "R": 4 * B * N, "xx": 4 * B, "gterms": 4 * B * N * N, "XC": 4 * B * N * K,
                "ent": B * N * kc[0] * cw if nlev else 0}
        for v in range(6):
            has = v < nlev
            want[f"S{v}"] = 4 * B * (N >> v) * kc[v] if has else 0
            if v:
                want[f"pos{v}"] = 2 * B * (N >> v) * kc[v] if has else 0
        for name, nbytes in want.items():
            assert at[name][1] == nbytes, (N, K, B, name)
        assert at["xf"][1] >= 4 * B * 32 and at["xe"][1] >= 4 * B and (at["tabs0"][1] > 0) == (N >= 8) and at["tabs0"][1] == at["tabs1"][1]
        # carve's order, 256-byte offsets, no overlap, nothing but alignment between two arrays
        end = 0
        for name in pl.CARVE_ORDER:
            off, nbytes = at[name]
            if nbytes == 0:
                assert off == 0
                continue
            assert off % 256 == 0 and off == (end + 255) // 256 * 256, (N, K, B, name)
            end = off + nbytes
        assert lay["total"] == (end + 255) // 256 * 256
        assert lay["total"] <= L.mcq_encode_workspace_bytes(B, N, K, 32), (N, K, B)      # what the encode is given holds the chunk
