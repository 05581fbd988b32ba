"""Host-side checks of the Lloyd step over an fp16 store (no GPU; include/mcq_half.h rules 48-51): signatures against the header,
the two size queries, the checks that precede any launch (fake pointers), and the Python argument errors."""
import ctypes
import os

import pytest

import test_abi_signatures_host as ab

NEW = ("mcq_kmeans_half_parts", "mcq_kmeans_half_planes", "mcq_kmeans_assign_half", "mcq_kmeans_update_half")
HDR = os.path.join(os.path.dirname(ab.HEADER), "mcq_half.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_and_bound():
    m = _lib()
    L = m.lib()
    assert tuple(ab.header_declarations(HDR)) == NEW == m.HALF_SYMBOLS
    assert ab.mismatches(ab.header_signatures(HDR), m.HALF_SIGNATURES) == []
    assert L.mcq_abi_version() == 7
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.HALF_SIGNATURES[name][1])
    text = open(HDR).read()
    assert all(rule in text for rule in (" 48. ", " 49. ", " 50. ", " 51. ")) and '#include "mcq_kmeans.h"' in text


def test_queries_and_checks_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    for lists, D in ((1, 1), (300, 32), (300, 33), (16384, 512)):
        assert L.mcq_kmeans_half_planes(lists, D) == 2 * lists * 32 * -(-D // 32)
    assert L.mcq_kmeans_half_planes(0, 8) == 0 and L.mcq_kmeans_half_planes(5, 16385) == 0 and L.mcq_kmeans_half_planes(5, 0) == 0
    assert L.mcq_kmeans_half_parts(1024, 16384, 512) == 64 and L.mcq_kmeans_half_parts(65536, 16384, 512) == 1
    assert L.mcq_kmeans_half_parts(0, 100, 64) == 1 and L.mcq_kmeans_half_parts(300, 300, 64) == 3
    fake, odd2, odd1 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 2), ctypes.c_void_p((1 << 20) + 1)

    def f(x=fake, B=300, c=fake, L_=300, D=64, terms=fake, parts=1, prev=None, outs=fake, changed=fake, ps=fake, pl=fake, planes=fake):
        return L.mcq_kmeans_assign_half(x, B, c, L_, D, terms, parts, prev, outs, outs, changed, ps, pl, planes, None)

    nothing = dict(x=None, c=None, terms=None, outs=None, changed=None, ps=None, pl=None, planes=None)
    assert f(D=16385, B=-1, L_=0, **nothing) == U and f(D=0, **nothing) == I and f(B=(1 << 31) - 1, **nothing) == U
    assert f(outs=None) == I and f(prev=fake, changed=None) == I and f(B=0, **nothing) == 0
    assert f(parts=4, **{**nothing, "outs": fake}) == I
    for name in ("x", "c", "terms", "ps", "pl", "planes"):
        assert f(**{name: None}) == I
    for name, ptr in (("x", odd1), ("c", odd2), ("terms", odd2), ("outs", odd2), ("prev", odd2), ("ps", odd2), ("pl", odd2),
                      ("planes", ctypes.c_void_p((1 << 20) + 8))):
        assert f(**{name: ptr}) == I

    def u(x=fake, B=300, D=64, order=fake, L_=7, sums=fake):
        return L.mcq_kmeans_update_half(x, B, D, order, fake, L_, fake, fake, fake, fake, sums, None)

    assert u(D=16385, B=-1) == U and u(L_=0) == I and u(B=(1 << 31) - 2, L_=(1 << 31) - 2) == U
    assert u(x=None) == I and u(order=None) == I and u(x=odd1) == I and u(sums=ctypes.c_void_p((1 << 20) + 4)) == I


def test_half_parts_is_the_fp32_recommendation():
    """rule 48 takes rule 44's formula: one function behind both queries"""
    L = _lib().lib()
    for B in (0, 1, 128, 129, 1024, 65536):
        for lists in (1, 128, 129, 300, 16384):
            for D in (1, 64, 16384):
                assert L.mcq_kmeans_half_parts(B, lists, D) == L.mcq_kmeans_parts(B, lists, D), (B, lists, D)
    for bad in ((300, 300, 0), (300, 300, 16385), (300, 0, 64)):
        assert L.mcq_kmeans_half_parts(*bad) == L.mcq_kmeans_parts(*bad) == 1


def test_fp32_and_fp16_entries_refuse_alike():
    """one table of bad arguments against both entries of each pair (fake pointers, no launch): the same return code case by
    case.  The stated exceptions: `planes`, which the fp32 entry does not have, and vectors at a 2-byte boundary, which only
    the fp32 entries refuse"""
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    big = (1 << 31) - 1
    fake, odd1, odd2, odd4 = (ctypes.c_void_p((1 << 20) + k) for k in (0, 1, 2, 4))

    def assign(half, x=fake, B=300, c=fake, L_=300, D=64, terms=fake, parts=1, prev=None, assign=fake, score=fake, changed=fake,
               ps=fake, pl=fake, planes=fake):
        if half:
            return L.mcq_kmeans_assign_half(x, B, c, L_, D, terms, parts, prev, assign, score, changed, ps, pl, planes, None)
        return L.mcq_kmeans_assign(x, B, c, L_, D, terms, parts, prev, assign, score, changed, ps, pl, None)

    none = dict(x=None, c=None, terms=None, assign=None, score=None, changed=None, ps=None, pl=None, planes=None)
    outs = {**none, "assign": fake, "score": fake}
    cases = [(dict(D=16385, B=-1, L_=0, **none), U), (dict(D=0, L_=big, **none), I), (dict(B=-1, L_=big, **none), I),
             (dict(L_=0, B=big, **none), I), (dict(B=big, **none), U), (dict(L_=1 << 40, **none), U),       # the domain
             (dict(assign=None), I), (dict(score=None), I), (dict(prev=fake, changed=None), I),            # outputs; prev without changed
             (dict(B=0, **none), 0), (dict(B=0, prev=fake, **{**none, "changed": odd2}), I),               # B == 0
             (dict(B=0, parts=0, **none), 0)]
    cases += [(dict(parts=p, **outs), I) for p in (0, -1, 4, 1 << 40)]                                      # 300 lists are 3 tiles
    cases += [(dict(B=big - 1, L_=big - 1, parts=1 << 24, **outs), U)]                                      # the grid
    cases += [({n: None}, I) for n in ("x", "c", "terms", "ps", "pl")]                                      # null pointers
    cases += [({n: odd2}, I) for n in ("c", "terms", "assign", "score", "prev", "ps", "pl")] + [(dict(x=odd1), I)]   # odd pointers
    cases += [(dict(prev=fake, changed=odd2), I)]
    for kw, want in cases:
        assert assign(False, **kw) == assign(True, **kw) == want, kw
    assert assign(True, planes=None) == I and assign(True, planes=ctypes.c_void_p((1 << 20) + 8)) == I     # exception: planes
    assert assign(False, x=odd2) == I                                                                      # exception: 2-byte vectors

    names = ("x", "order", "off", "cin", "cout", "counts", "first", "sums")

    def update(half, B=300, D=64, L_=7, **kw):
        p = {n: kw.get(n, fake) for n in names}
        f = L.mcq_kmeans_update_half if half else L.mcq_kmeans_update
        return f(p["x"], B, D, p["order"], p["off"], L_, p["cin"], p["cout"], p["counts"], p["first"], p["sums"], None)

    nothing = {n: None for n in names}
    cases = [(dict(D=16385, B=-1, L_=0, **nothing), U), (dict(D=0, B=big, **nothing), I), (dict(B=-1, L_=big, **nothing), I),
             (dict(L_=0, B=big, **nothing), I), (dict(B=big, **nothing), U), (dict(L_=big, **nothing), U),
             (dict(B=big - 1, L_=big - 1, **nothing), U),                                                   # ceil(B / 4096) + L: the grid
             (dict(B=0, x=None, order=None, off=None), I)]
    cases += [({n: None}, I) for n in names]
    cases += [({n: odd4}, I) for n in ("order", "off", "first", "sums")] + [({n: odd2}, I) for n in ("cin", "cout", "counts")]
    cases += [(dict(x=odd1), I)]
    for kw, want in cases:
        assert update(False, **kw) == update(True, **kw) == want, kw
    assert update(False, x=odd2) == I                                                                      # exception: 2-byte vectors


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    import quantization_amd as qa
    assert {"coarse_assign_half", "kmeans_step_half", "coarse_train_half"} <= set(qa.__all__)
    x, c = torch.zeros(30, 24, dtype=torch.float16), torch.zeros(5, 24)
    for call in (lambda: qa.coarse_assign_half(x, c), lambda: qa.kmeans_step_half(x, c), lambda: qa.coarse_train_half(x, 5),
                 lambda: qa.coarse_train_half(x, 5, init=c)):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            call()
    i32 = torch.zeros(30, dtype=torch.int32)
    bad = ((lambda: qa.coarse_assign_half(x.float(), c), "coarse_assign;"), (lambda: qa.kmeans_step_half(x.float(), c), "kmeans_step;"),
           (lambda: qa.coarse_train_half(x.float(), 5), "coarse_train;"), (lambda: qa.kmeans_step_half(x.bfloat16(), c), "vectors"),
           (lambda: qa.kmeans_step_half(x, c.half()), "centroids"), (lambda: qa.coarse_assign_half(x[:, :23], c), "vectors"),
           (lambda: qa.coarse_assign_half(x.reshape(3, 10, 24), c), "vectors"), (lambda: qa.kmeans_step_half(x, c[:0]), "at least one"),
           (lambda: qa.kmeans_step_half(x, c, terms=torch.zeros(4)), "terms"),
           (lambda: qa.kmeans_step_half(x, c, prev_assign=i32.long()), "prev_assign"),
           (lambda: qa.coarse_train_half(x, 0), "num_lists"), (lambda: qa.coarse_train_half(x, 31), "distinct rows"),
           (lambda: qa.coarse_train_half(x, 5, iters=-1), "iters"), (lambda: qa.coarse_train_half(x, 5, seed="a"), "seed"),
           (lambda: qa.coarse_train_half(x, 5, init=c[:4]), "init"), (lambda: qa.coarse_train_half(x, 5, init=c.half()), "init"),
           (lambda: qa.kmeans_step(x, c), "vectors"), (lambda: qa.coarse_train(x, 5), "vectors"))       # the fp32 calls still refuse
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
