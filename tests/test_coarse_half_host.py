"""Host-side checks of the coarse probes for fp16 queries (no GPU; include/mcq_coarse_half.h rules 52-55): signatures against
the header, the order of the argument checks (fake pointers, no launch), mcq_coarse_half_parts, and the Python argument errors."""
import ctypes
import os

import pytest

import test_abi_signatures_host as ab

NEW = ("mcq_coarse_half_parts", "mcq_coarse_half_split", "mcq_coarse_probe_half")
HDR = os.path.join(os.path.dirname(ab.HEADER), "mcq_coarse_half.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_and_bound():
    m = _lib()
    L = m.lib()
    assert tuple(ab.header_declarations(HDR)) == NEW == m.COARSE_HALF_SYMBOLS
    assert ab.mismatches(ab.header_signatures(HDR), m.COARSE_HALF_SIGNATURES) == []
    assert len(ab.header_signatures()) == 64 and L.mcq_abi_version() == 7       # include/mcq.h and the ABI version are unchanged
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.COARSE_HALF_SIGNATURES[name][1])
    text = open(HDR).read()
    assert all(rule in text for rule in (" 52. ", " 53. ", " 54. ", " 55. ")) and '#include "mcq_half.h"' in text


def test_argument_checks_in_order_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    fake, odd1, odd2, odd8, big = *(ctypes.c_void_p((1 << 20) + k) for k in (0, 1, 2, 8)), (1 << 31) - 1

    def f(q=fake, Q=40, c=fake, planes=fake, L_=300, D=64, terms=fake, P=8, metric=0, parts=1, outs=fake, bias=None, ps=fake, pl=fake):
        return L.mcq_coarse_probe_half(q, Q, c, planes, L_, D, terms, P, metric, parts, outs, outs, bias, ps, pl, None)

    nothing = dict(q=None, c=None, planes=None, terms=None, outs=None, ps=None, pl=None)
    for D, P in ((16385, 8), (64, 129), (16385, 0), (0, 129)):               # the limits first, before any pointer is looked at
        assert f(D=D, P=P, Q=-1, metric=9, **nothing) == U
    for kw in (dict(D=0), dict(P=0), dict(Q=-1), dict(L_=-1)):
        assert f(metric=9, **kw, **nothing) == I
    assert f(metric=3, Q=big, **nothing) == I and f(metric=-1, L_=big, **nothing) == I       # the metric before the large sizes
    assert f(Q=big, **nothing) == U and f(L_=1 << 40, **nothing) == U
    assert f(outs=None) == I                                                 # missing outputs
    assert f(Q=0, **nothing) == 0 and f(Q=0, P=129, **nothing) == U          # no queries: nothing is looked at
    assert f(L_=0, outs=None, q=odd1, c=odd1, planes=odd1) == I              # L == 0 needs its outputs alone
    for parts in (0, -1, 6, 1 << 40):                                        # 300 lists are 5 tiles of 64
        assert f(parts=parts, **{**nothing, "outs": fake}) == I
    assert f(Q=big - 1, L_=big - 1, parts=1 << 25, **{**nothing, "outs": fake}) == U         # the grid
    for name in ("q", "c", "planes", "ps", "pl", "terms"):                   # the pointers, then the alignments
        assert f(**{name: None}, outs=odd2) == I
    assert f(terms=None, metric=1, outs=odd2) == I                           # (ip needs no terms: the alignment answered)
    for name, ptr in (("q", odd1), ("c", odd2), ("planes", odd8), ("terms", odd2), ("outs", odd2), ("bias", odd2), ("ps", odd2),
                      ("pl", odd2)):
        assert f(**{name: ptr}) == I

    def s(c=fake, L_=300, D=64, planes=fake):
        return L.mcq_coarse_half_split(c, L_, D, planes, None)

    assert s(D=16385, L_=-1, c=None) == U and s(D=0, c=None) == I and s(L_=-1, c=None) == I and s(L_=big, c=None) == U
    assert s(L_=0, c=None, planes=None) == 0 and s(c=None) == I and s(planes=None) == I and s(c=odd2) == I and s(planes=odd8) == I


def test_recommended_parts():
    L = _lib().lib()
    for P, target in ((1, 512), (16, 512), (17, 256), (64, 256), (65, 256), (128, 256)):
        for Q in (1, 63, 64, 65, 1024, 16383, 16384, 32768, 1 << 20):
            for lists in (1, 64, 65, 1024, 16384, 1 << 20):
                parts, tiles, qt = L.mcq_coarse_half_parts(Q, lists, 512, P), -(-lists // 64), -(-Q // 64)
                assert 1 <= parts <= tiles and (parts == 1 if qt >= target else parts == min(tiles, -(-target // qt))), (P, Q, lists)
    assert L.mcq_coarse_half_parts(64, 65536, 512, 8) == 512 and L.mcq_coarse_half_parts(1024, 65536, 512, 64) == 16
    for bad in ((0, 100, 64, 8), (4, 0, 64, 8), (-1, 100, 64, 8), (4, 100, 0, 8), (4, 100, 64, 129), ((1 << 31) - 1, 100, 64, 8)):
        assert L.mcq_coarse_half_parts(*bad) == 1


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    import quantization_amd as qa
    assert {"coarse_planes", "coarse_probe_half"} <= set(qa.__all__)
    q, c = torch.zeros(7, 24, dtype=torch.float16), torch.zeros(5, 24)
    for call in (lambda: qa.coarse_planes(c), lambda: qa.coarse_probe_half(q, c, 3), lambda: qa.coarse_probe_half(q, c, 3, "ip")):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            call()
    planes = torch.zeros(2 * 5 * 32, dtype=torch.int16)
    bad = ((lambda: qa.coarse_probe_half(q.float(), c, 3), "coarse_probe;"), (lambda: qa.coarse_probe_half(q.bfloat16(), c, 3), "queries"),
           (lambda: qa.coarse_probe_half(q[:, :23], c, 3), "queries"), (lambda: qa.coarse_probe_half(q, c.half(), 3), "centroids"),
           (lambda: qa.coarse_planes(c.half()), "centroids"), (lambda: qa.coarse_probe_half(q, c, 0), "nprobe"),
           (lambda: qa.coarse_probe_half(q, c, 129), "nprobe"), (lambda: qa.coarse_probe_half(q, c, True), "nprobe"),
           (lambda: qa.coarse_probe_half(q, c, 3, metric="dot"), "metric"),
           (lambda: qa.coarse_probe_half(q, c, 3, terms=torch.zeros(4)), "terms"),
           (lambda: qa.coarse_probe_half(q, c, 3, planes=planes[:-1]), "planes"),
           (lambda: qa.coarse_probe_half(q, c, 3, planes=planes.float()), "planes"),
           (lambda: qa.coarse_probe(q, c, 3), "queries"), (lambda: qa.coarse_assign(q, c), "vectors"))     # the fp32 calls still refuse
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
