"""Host-side checks of the coarse probes for fp32 queries by six bf16 plane products (no GPU; include/mcq_coarse_split.h rules
64-67): signatures against the header, the order of the argument checks (fake pointers, no launch) beside
mcq_coarse_probe_half where rule 64 shares rule 52, mcq_coarse_split_parts, and the Python argument errors."""
import ctypes
import os

import pytest

import test_abi_signatures_host as ab

NEW = ("mcq_coarse_split_parts", "mcq_coarse_split_planes", "mcq_coarse_probe_split")
HDR = os.path.join(os.path.dirname(ab.HEADER), "mcq_coarse_split.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_and_bound():
    m = _lib()
    L = m.lib()
    assert tuple(ab.header_declarations(HDR)) == NEW == m.COARSE_SPLIT_SYMBOLS
    assert ab.mismatches(ab.header_signatures(HDR), m.COARSE_SPLIT_SIGNATURES) == []
    assert len(ab.header_signatures()) == 64 and L.mcq_abi_version() == 7       # include/mcq.h and the ABI version are unchanged
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.COARSE_SPLIT_SIGNATURES[name][1])
    text = open(HDR).read()
    assert all(rule in text for rule in (" 64. ", " 65. ", " 66. ", " 67. "))
    assert '#include "mcq_split.h"' in text and '#include "mcq_coarse.h"' in text


def test_argument_checks_in_order_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    fake, odd1, odd2, odd8, big = *(ctypes.c_void_p((1 << 20) + k) for k in (0, 1, 2, 8)), (1 << 31) - 1

    def new(q=fake, Q=40, c=fake, planes=fake, L_=300, D=64, terms=fake, P=8, metric=0, parts=1, outs=fake, bias=None, ps=fake,
            pl=fake, qp=fake):
        return L.mcq_coarse_probe_split(q, Q, c, planes, L_, D, terms, P, metric, parts, outs, outs, bias, ps, pl, qp, None)

    def half(qp=None, **kw):                                                 # the same call of rule 52's entry: no query planes
        a = dict(q=fake, Q=40, c=fake, planes=fake, L_=300, D=64, terms=fake, P=8, metric=0, parts=1, outs=fake, bias=None,
                 ps=fake, pl=fake)
        a.update(kw)
        return L.mcq_coarse_probe_half(a["q"], a["Q"], a["c"], a["planes"], a["L_"], a["D"], a["terms"], a["P"], a["metric"],
                                       a["parts"], a["outs"], a["outs"], a["bias"], a["ps"], a["pl"], None)

    nothing = dict(q=None, c=None, planes=None, terms=None, outs=None, ps=None, pl=None, qp=None)
    shared = [(dict(D=D, P=P, Q=-1, metric=9, **nothing), U) for D, P in ((16385, 8), (64, 129), (16385, 0), (0, 129))]
    shared += [(dict(metric=9, **kw, **nothing), I) for kw in (dict(D=0), dict(P=0), dict(Q=-1), dict(L_=-1))]
    shared += [(dict(metric=3, Q=big, **nothing), I), (dict(metric=-1, L_=big, **nothing), I)]      # the metric before the large sizes
    shared += [(dict(Q=big, **nothing), U), (dict(L_=1 << 40, **nothing), U), (dict(outs=None), I)]
    shared += [(dict(Q=0, **nothing), 0), (dict(Q=0, P=129, **nothing), U)]                         # no queries: nothing is looked at
    shared += [(dict(L_=0, outs=None, q=odd1, c=odd1, planes=odd1), I)]                             # L == 0 needs its outputs alone
    shared += [(dict(parts=parts, **{**nothing, "outs": fake}), I) for parts in (0, -1, 1 << 40)]
    shared += [(dict(Q=big - 1, L_=big - 1, parts=1 << 24, **{**nothing, "outs": fake}), U)]        # the grid
    shared += [(dict(**{name: None}, outs=odd2), I) for name in ("q", "c", "planes", "ps", "pl", "terms")]   # pointers, then alignments
    shared += [(dict(terms=None, metric=1, outs=odd2), I)]                   # (ip needs no terms: the alignment answered)
    shared += [(dict(**{name: ptr}), I) for name, ptr in (("c", odd2), ("planes", odd8), ("terms", odd2), ("outs", odd2),
                                                            ("bias", odd2), ("ps", odd2), ("pl", odd2))]
    for kw, rc in shared:
        assert new(**kw) == rc == half(**kw), kw
    # what rule 64 has of its own: tiles of 128 centroids (300 lists are 3), the query planes, fp32 queries on 4 bytes
    assert new(parts=4) == I and new(Q=big - 1, L_=big - 1, parts=1 << 25) == I and new(qp=None, outs=odd2) == I and new(qp=odd8) == I and new(q=odd2) == I and new(q=odd1) == I

    def s(c=fake, R=300, D=64, planes=fake):
        return L.mcq_coarse_split_planes(c, R, D, planes, None), L.mcq_coarse_half_split(c, R, D, planes, None)

    assert s(D=16385, R=-1, c=None) == (U, U) and s(D=0, c=None) == (I, I) and s(R=-1, c=None) == (I, I) and s(R=big, c=None) == (U, U)
    assert s(R=0, c=None, planes=None) == (0, 0) and s(c=None) == (I, I) and s(planes=None) == (I, I)
    assert s(c=odd2) == (I, I) and s(planes=odd8) == (I, I)


def test_recommended_parts():
    L = _lib().lib()
    for P, tile in ((1, 128), (32, 128), (33, 128), (64, 128), (65, 64), (128, 64)):
        for Q in (1, 64, 127, 128, 129, 1024, 16384, 32768, 1 << 20):
            for lists in (1, 128, 129, 1024, 16384, 1 << 20):
                parts, tiles, qt = L.mcq_coarse_split_parts(Q, lists, 512, P), -(-lists // 128), -(-Q // tile)
                assert 1 <= parts <= tiles and (parts == 1 if qt >= 256 else parts == min(tiles, -(-256 // qt))), (P, Q, lists)
    assert L.mcq_coarse_split_parts(64, 65536, 512, 8) == 256 and L.mcq_coarse_split_parts(1024, 65536, 512, 64) == 32
    assert L.mcq_coarse_split_parts(1024, 65536, 512, 128) == 16 and L.mcq_coarse_split_parts(1, 1024, 512, 1) == 8
    for bad in ((0, 100, 64, 8), (4, 0, 64, 8), (-1, 100, 64, 8), (4, 100, 0, 8), (4, 100, 64, 129), ((1 << 31) - 1, 100, 64, 8)):
        assert L.mcq_coarse_split_parts(*bad) == 1
    assert L.mcq_kmeans_split_planes(300, 33) == 3 * 300 * 64            # what mcq_coarse_split_planes writes


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    import quantization_amd as qa
    assert {"coarse_planes_split", "coarse_probe_split"} <= set(qa.__all__)
    q, c = torch.zeros(7, 24), torch.zeros(5, 24)
    for call in (lambda: qa.coarse_planes_split(c), lambda: qa.coarse_probe_split(q, c, 3), lambda: qa.coarse_probe_split(q, c, 3, "ip")):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            call()
    planes = torch.zeros(3 * 5 * 32, dtype=torch.int16)
    bad = ((lambda: qa.coarse_probe_split(q.half(), c, 3), "coarse_probe_half;"), (lambda: qa.coarse_probe_split(q.bfloat16(), c, 3), "no probe takes bf16"),
           (lambda: qa.coarse_probe_split(q.double(), c, 3), "queries"), (lambda: qa.coarse_probe_split(q[:, :23], c, 3), "queries"),
           (lambda: qa.coarse_probe_split(q, c.half(), 3), "centroids"), (lambda: qa.coarse_planes_split(c.half()), "centroids"),
           (lambda: qa.coarse_probe_split(q, c, 0), "nprobe"), (lambda: qa.coarse_probe_split(q, c, 129), "nprobe"),
           (lambda: qa.coarse_probe_split(q, c, True), "nprobe"), (lambda: qa.coarse_probe_split(q, c, 3, metric="dot"), "metric"),
           (lambda: qa.coarse_probe_split(q, c, 3, terms=torch.zeros(4)), "terms"),
           (lambda: qa.coarse_probe_split(q, c, 3, planes=planes[:-1]), "planes"),
           (lambda: qa.coarse_probe_split(q, c, 3, planes=planes.float()), "planes"),
           (lambda: qa.coarse_probe_split(q, c, 3, planes=torch.zeros(2 * 5 * 32, dtype=torch.int16)), "coarse_planes_split"))
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
