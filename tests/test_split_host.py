"""Host-side checks of the assignment of fp32 rows by six bf16 plane products (no GPU; include/mcq_split.h rules 60-63)."""
import ctypes
import os

import pytest

import test_abi_signatures_host as ab

NEW = ("mcq_kmeans_split_parts", "mcq_kmeans_split_planes", "mcq_kmeans_assign_split")
HDR = os.path.join(os.path.dirname(ab.HEADER), "mcq_split.h")


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_and_bound():
    m = _lib()
    L = m.lib()
    assert tuple(ab.header_declarations(HDR)) == NEW == m.SPLIT_SYMBOLS
    assert ab.mismatches(ab.header_signatures(HDR), m.SPLIT_SIGNATURES) == []
    assert L.mcq_abi_version() == 7
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.SPLIT_SIGNATURES[name][1])


def test_queries_and_checks_without_launch():
    """rule 60: three planes, parts from 256 tiles of 128 vectors, rule 48's checks case by case beside the bf16 entry"""
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    for lists, D in ((1, 1), (300, 32), (300, 33), (16384, 512)):
        assert L.mcq_kmeans_split_planes(lists, D) == 3 * lists * 32 * -(-D // 32)
    assert L.mcq_kmeans_split_planes(0, 8) == 0 and L.mcq_kmeans_split_planes(5, 16385) == 0 and L.mcq_kmeans_split_planes(5, 0) == 0
    for (B, lists, D), want in (((1024, 16384, 512), 32), ((32768, 16384, 512), 1), ((32767, 16384, 512), 1), ((16384, 300, 64), 2),
                                ((0, 100, 64), 1), ((300, 300, 64), 3), ((129, 16384, 8), 128), ((300, 300, 0), 1), ((300, 0, 64), 1)):
        assert L.mcq_kmeans_split_parts(B, lists, D) == want, (B, lists, D)
    fake, odd1, odd2, odd8 = (ctypes.c_void_p((1 << 20) + k) for k in (0, 1, 2, 8))
    names = ("x", "c", "terms", "prev", "assign", "score", "changed", "ps", "pl", "planes")

    def f(entry, B=300, L_=300, D=64, parts=1, **kw):
        p = {n: kw.get(n, None if n == "prev" else fake) for n in names}
        return entry(p["x"], B, p["c"], L_, D, p["terms"], parts, *(p[n] for n in names[3:]), None)

    none = {n: None for n in names}
    cases = [(dict(D=16385, B=-1, L_=0, **none), U), (dict(D=0, **none), I), (dict(B=(1 << 31) - 1, **none), U), (dict(assign=None), I),
             (dict(score=None), I), (dict(prev=fake, changed=None), I), (dict(B=0, **none), 0), (dict(parts=4, **{**none, "assign": fake, "score": fake}), I)]
    cases += [({n: None}, I) for n in ("x", "c", "terms", "ps", "pl", "planes")] + [(dict(x=odd1), I), (dict(planes=odd8), I)]
    cases += [({n: odd2}, I) for n in ("c", "terms", "assign", "score", "prev", "ps", "pl")]
    for kw, want in cases:
        assert f(L.mcq_kmeans_assign_split, **kw) == f(L.mcq_kmeans_assign_bf16, **kw) == want, kw
    assert f(L.mcq_kmeans_assign_split, x=odd2) == I        # (2 bytes past a boundary: a bf16 row may start there, an fp32 row not)


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    import quantization_amd as qa
    assert {"coarse_assign_split", "kmeans_step_split", "coarse_train_split"} <= set(qa.__all__)
    x, c = torch.zeros(30, 24), torch.zeros(5, 24)
    for call in (lambda: qa.coarse_assign_split(x, c), lambda: qa.kmeans_step_split(x, c), lambda: qa.coarse_train_split(x, 5)):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            call()
    bad = ((lambda: qa.coarse_assign_split(x.half(), c), "coarse_assign_half;"), (lambda: qa.kmeans_step_split(x.half(), c), "kmeans_step_half;"),
           (lambda: qa.coarse_train_split(x.half(), 5), "coarse_train_half;"), (lambda: qa.coarse_assign_split(x.bfloat16(), c), "coarse_assign_bf16;"),
           (lambda: qa.kmeans_step_split(x.bfloat16(), c), "kmeans_step_bf16;"), (lambda: qa.coarse_train_split(x.bfloat16(), 5), "coarse_train_bf16;"),
           (lambda: qa.coarse_assign_split(x[:, :23], c), "vectors"), (lambda: qa.coarse_assign_split(x.reshape(3, 10, 24), c), "vectors"),
           (lambda: qa.coarse_assign_split(x.double(), c), "vectors"), (lambda: qa.coarse_assign_split(x, c[:0]), "centroids"),
           (lambda: qa.kmeans_step_split(x, c, prev_assign=torch.zeros(30, dtype=torch.int64)), "prev_assign"), (lambda: qa.coarse_train_split(x, 0), "num_lists"),
           (lambda: qa.coarse_train_split(x, 5, iters=-1), "iters"), (lambda: qa.coarse_train_split(x, 5, init=c.bfloat16()), "init"),
           (lambda: qa.coarse_train_split(x.reshape(3, 10, 24), 5), "an fp32"), (lambda: qa.coarse_train_split(x, 31), "num_lists"),
           (lambda: qa.kmeans_step_bf16(x, c), "kmeans_step;"))   # (the other calls as before)
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
