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
