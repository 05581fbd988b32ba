"""Host-side checks of the coarse probes (no GPU; include/mcq_coarse.h rules 40-43): signatures against the header, the order
of the argument checks (fake pointers, no launch), mcq_coarse_parts, and the Python argument errors."""
import ctypes
import os

import pytest

import test_abi_signatures_host as ab

NEW = ("mcq_coarse_terms", "mcq_coarse_parts", "mcq_coarse_probe")
HDR = os.path.join(os.path.dirname(ab.HEADER), "mcq_coarse.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_and_bound():
    m = _lib()
    L = m.lib()
    assert tuple(ab.header_declarations(HDR)) == NEW == m.COARSE_SYMBOLS
    assert ab.mismatches(ab.header_signatures(HDR), m.COARSE_SIGNATURES) == []
    assert len(ab.header_signatures()) == 64 and L.mcq_abi_version() == 7       # include/mcq.h and the ABI version are unchanged
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.COARSE_SIGNATURES[name][1])
    text = open(HDR).read()
    assert all(rule in text for rule in (" 40. ", " 41. ", " 42. ", " 43. "))


def test_argument_checks_in_order_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    fake, odd, big = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 2), (1 << 31) - 1

    def f(q=fake, Q=40, c=fake, L_=300, D=64, terms=fake, P=8, metric=0, parts=1, outs=fake, bias=None, ps=fake, pl=fake):
        return L.mcq_coarse_probe(q, Q, c, L_, D, terms, P, metric, parts, outs, outs, bias, ps, pl, None)

    nothing = dict(q=None, c=None, terms=None, outs=None, ps=None, pl=None)
    for D, P in ((16385, 8), (64, 129), (16385, 0), (0, 129)):               # the limits first, before any pointer is looked at
        assert f(D=D, P=P, Q=-1, metric=9, **nothing) == U
    for kw in (dict(D=0), dict(P=0), dict(Q=-1), dict(L_=-1)):
        assert f(metric=9, **kw, **nothing) == I
    assert f(metric=3, Q=big) == I and f(metric=-1, L_=big) == I             # the metric before the large sizes
    assert f(Q=big, **nothing) == U and f(L_=1 << 40, **nothing) == U
    assert f(outs=None) == I                                                 # missing outputs
    assert f(Q=0, **nothing) == 0 and f(Q=0, P=129, **nothing) == U          # no queries: nothing is looked at
    assert f(L_=0, outs=None, q=odd, c=odd) == I                             # L == 0 needs its outputs alone
    for parts in (0, -1, 4, 1 << 40):                                        # 300 lists are 3 tiles
        assert f(parts=parts, **{**nothing, "outs": fake}) == I
    assert f(Q=big - 1, L_=big - 1, parts=1 << 24, **{**nothing, "outs": fake}) == U         # the grid
    for name in ("q", "c", "terms", "ps", "pl"):                             # the pointers, then the alignments
        assert f(**{name: None}, outs=odd) == I
    assert f(terms=None, metric=1, outs=odd) == I                            # (ip needs no terms: the alignment answered)
    for name in ("q", "c", "terms", "outs", "bias", "ps", "pl"):
        assert f(**{name: odd}) == I

    def t(c=fake, L_=300, D=64, metric=0, terms=fake):
        return L.mcq_coarse_terms(c, L_, D, metric, terms, None)

    assert t(D=16385, L_=-1, c=None) == U and t(D=0, metric=9) == I and t(L_=-1, metric=9) == I and t(metric=5, L_=big) == I
    assert t(L_=big, c=None) == U and t(metric=1, c=None, terms=None) == 0 and t(L_=0, c=None, terms=None) == 0
    assert t(c=None) == I and t(terms=None) == I and t(c=odd) == I and t(terms=odd, metric=2) == I


def test_recommended_parts():
    L = _lib().lib()
    for Q in (1, 31, 64, 1024, 8191, 8192, 1 << 20):
        for lists in (1, 128, 129, 1024, 16384, 1 << 20):
            parts, tiles, qt = L.mcq_coarse_parts(Q, lists, 512, 8), -(-lists // 128), -(-Q // 32)
            assert 1 <= parts <= tiles and (parts == 1 if qt >= 256 else parts == min(tiles, -(-512 // qt)))
    assert L.mcq_coarse_parts(64, 16384, 512, 8) == 128 and L.mcq_coarse_parts(8192, 16384, 512, 8) == 1
    for bad in ((0, 100, 64, 8), (4, 0, 64, 8), (-1, 100, 64, 8), (4, 100, 0, 8), (4, 100, 64, 129), ((1 << 31) - 1, 100, 64, 8)):
        assert L.mcq_coarse_parts(*bad) == 1


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    import quantization_amd as qa
    assert {"coarse_terms", "coarse_probe", "coarse_assign"} <= set(qa.__all__)
    q, c = torch.zeros(3, 24), torch.zeros(50, 24)
    for call in (lambda: qa.coarse_probe(q, c, 4), lambda: qa.coarse_assign(q, c), lambda: qa.coarse_terms(c, "cosine")):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            call()
    bad = ((lambda: qa.coarse_probe(q, c, 4, metric="dot"), "metric"), (lambda: qa.coarse_probe(q, c, 129), "probe_lists"),
           (lambda: qa.coarse_probe(q, c, 0), "nprobe ="), (lambda: qa.coarse_probe(q, c, 2.0), "nprobe ="),
           (lambda: qa.coarse_probe(q, c, True), "nprobe ="), (lambda: qa.coarse_probe(q, c.half(), 4), "centroids"),
           (lambda: qa.coarse_terms(torch.zeros(2, 16385)), "dim"), (lambda: qa.coarse_probe(torch.zeros(3, 23), c, 4), "queries"),
           (lambda: qa.coarse_probe(q, c, 4, terms=torch.zeros(49)), "terms"),
           (lambda: qa.coarse_assign(q.reshape(3, 1, 24), c), "vectors"), (lambda: qa.coarse_assign(q, c[:0]), "at least one"))
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
