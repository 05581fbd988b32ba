"""Host-side checks of include/mcq_probe.h (no GPU): its entries are declared as _lib.PROBE_SIGNATURES binds them, exported and
bound; include/mcq.h and include/mcq_residual.h keep what they had; the argument checks of mcq_test_er answer in the
documented order before anything touches the device (fake pointers, no launch); and the pair plan of the dense Gram-terms
kernel -- row block m owns the pairs (m, (m + d) mod N), d = 0 .. N / 2, the last for m < N / 2 only -- restated here covers
every unordered pair exactly once, evenly, the reader's plane rule finds each of the N * N ordered terms, and the planes fit
the Gram-terms buffer."""
import ctypes

import pytest

import search_selection_grid as sel

NEW = ("mcq_test_er_workspace_bytes", "mcq_test_er", "mcq_test_xc_xx",
       "mcq_test_pass_layout", "mcq_test_pass",      # (these two: tests/test_pass_lists_host.py checks their arguments,
       "mcq_test_pass16_layout", "mcq_test_pass16")  # these two: tests/test_pass16_lists_host.py)
PROBE_HDR = sel.API.replace("quantization_amd/csrc/mcq_api.hip", "include/mcq_probe.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_exported_and_bound():
    import test_abi_signatures_host as ab
    m = _lib()
    L = m.lib()
    hdr = ab.header_signatures(PROBE_HDR)
    assert tuple(hdr) == NEW == m.PROBE_SYMBOLS == tuple(m.PROBE_SIGNATURES)
    assert ab.mismatches(hdr, m.PROBE_SIGNATURES) == []
    assert not set(NEW) & set(m.SYMBOLS) and not set(NEW) & set(m.RESIDUAL_SYMBOLS) and not set(NEW) & set(ab.header_signatures())
    for name in NEW:
        assert hasattr(L, name) and getattr(L, name).argtypes == list(m.PROBE_SIGNATURES[name][1])
    a, b = m.PROBE_SIGNATURES["mcq_test_xc_xx"][1], m.SIGNATURES["mcq_test_xc"][1]
    assert a[:7] + a[8:] == b and a[7] is ctypes.c_void_p              # mcq_test_xc with xx_out after the x.C output
    assert '#include "mcq.h"' in open(PROBE_HDR).read() and L.mcq_abi_version() == 7
    doctored = dict(m.PROBE_SIGNATURES)
    r, args = doctored["mcq_test_er"]
    at = args.index(ctypes.c_long)
    doctored["mcq_test_er"] = (r, args[:at] + (ctypes.c_int,) + args[at + 1:])
    assert len(ab.mismatches(hdr, doctored)) == 1


def test_argument_checks_in_order():
    m = _lib()
    L = m.lib()
    P, IDX, WS = 1 << 20, 1 << 21, 1 << 22               # fake device pointers, aligned as asked; never dereferenced
    big = 1 << 40

    def call(N=8, K=256, D=32, B=64, form=1, prepared=P, xc=P, xx=P, idx=IDX, E=P, R=P, ws=WS, nbytes=big):
        return L.mcq_test_er(prepared, N, K, D, xc, xx, idx, B, None, None, form, E, R, ws, nbytes, None)

    assert call(N=3) != 0 and call(N=3, B=-1, form=7) == call(N=3)      # the domain first
    assert call(K=512, N=4, B=-1) == m.MCQ_EUNSUPPORTED                  # one-byte entries only
    assert call(B=-1) == m.MCQ_EINVAL and call(form=2) == m.MCQ_EINVAL and call(form=-1) == m.MCQ_EINVAL
    assert call(B=0, prepared=None, xc=None, idx=None, ws=None, nbytes=0) == 0        # an empty call looks at nothing
    for null in ("prepared", "xc", "xx", "idx", "E", "R", "ws"):
        assert call(**{null: None}) == m.MCQ_EINVAL, null
    assert call(idx=IDX + 8) == m.MCQ_EINVAL and call(ws=WS + 128) == m.MCQ_EINVAL
    need = L.mcq_test_er_workspace_bytes(64, 8)
    assert need == 64 * 8 * 8 * 4 and need % 256 == 0
    assert call(nbytes=need - 1) == m.MCQ_EWORKSPACE
    assert call(nbytes=need - 1, idx=IDX + 8) == m.MCQ_EINVAL            # alignment before the workspace's size
    assert L.mcq_test_xc_xx(P, 4, P, 8, 256, 32, P, None, WS, big, None, 0) == m.MCQ_EINVAL


def planes(N):
    return N // 2 + 1


def owned(N, m):
    """the distances d of the pairs (m, (m + d) mod N) that row block m gathers"""
    return [d for d in range(planes(N)) if d < N // 2 or m < N // 2]


def plane_of(N, m, n):
    """the reader's rule (tf_gram_plane): the plane that holds G[o_m][o_n] or its mirror, and whether it is the mirror"""
    d = (n - m) % N
    own = d < N // 2 or (d == N // 2 and m < N // 2)
    return (m * planes(N) + d, False) if own else (n * planes(N) + (N - d), True)


@pytest.mark.parametrize("N", [4, 8, 16])
def test_pair_plan_covers_every_pair_once(N):
    written = {}
    for m in range(N):
        for d in owned(N, m):
            key = m * planes(N) + d
            assert key not in written and key < N * planes(N)
            written[key] = (m, (m + d) % N)
    pairs = sorted(tuple(sorted(p)) for p in written.values())
    assert pairs == sorted((a, b) for a in range(N) for b in range(a, N))              # each unordered pair exactly once
    assert N * planes(N) <= N * N            # inside the N * N floats a vector has in the Gram-terms buffer
    per_block = [len(owned(N, m)) for m in range(N)]
    assert max(per_block) - min(per_block) == 1 and sum(per_block) == N * (N + 1) // 2
    for m in range(N):
        for n in range(N):
            key, mirror = plane_of(N, m, n)
            assert written[key] == ((n, m) if mirror else (m, n))
