"""Host-side checks of the Lloyd step (no GPU; include/mcq_kmeans.h rules 44-47): signatures against the header, the order of
the argument checks (fake pointers, no launch), mcq_kmeans_parts and mcq_kmeans_blocks, and the Python argument errors."""
import ctypes
import os

import pytest

import test_abi_signatures_host as ab

NEW = ("mcq_kmeans_parts", "mcq_kmeans_assign", "mcq_kmeans_blocks", "mcq_kmeans_update")
HDR = os.path.join(os.path.dirname(ab.HEADER), "mcq_kmeans.h")
BIG = (1 << 31) - 1


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_symbols_are_declared_and_bound():
    m = _lib()
    L = m.lib()
    assert tuple(ab.header_declarations(HDR)) == NEW == m.KMEANS_SYMBOLS
    assert ab.mismatches(ab.header_signatures(HDR), m.KMEANS_SIGNATURES) == []
    assert len(ab.header_signatures()) == 64 and L.mcq_abi_version() == 7       # include/mcq.h and the ABI version are unchanged
    for name in NEW:
        assert getattr(L, name).argtypes == list(m.KMEANS_SIGNATURES[name][1])
    text = open(HDR).read()
    assert all(rule in text for rule in (" 44. ", " 45. ", " 46. ", " 47. "))


def test_assign_checks_in_order_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    fake, odd = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 2)

    def f(x=fake, B=300, c=fake, L_=300, D=64, terms=fake, parts=1, prev=None, outs=fake, changed=fake, ps=fake, pl=fake):
        return L.mcq_kmeans_assign(x, B, c, L_, D, terms, parts, prev, outs, outs, changed, ps, pl, None)

    nothing = dict(x=None, c=None, terms=None, outs=None, changed=None, ps=None, pl=None)
    assert f(D=16385, B=-1, L_=0, **nothing) == U                            # the limit first, before any pointer is looked at
    for kw in (dict(D=0, L_=BIG), dict(B=-1, L_=BIG), dict(L_=0, B=BIG), dict(L_=-5, B=BIG)):       # before the large sizes
        assert f(**kw, **nothing) == I
    assert f(B=BIG, **nothing) == U and f(L_=1 << 40, **nothing) == U
    assert f(outs=None) == I and f(prev=fake, changed=None) == I             # missing outputs
    assert f(B=0, **nothing) == 0                                            # no vectors and no prev_assign: nothing is looked at
    assert f(B=0, prev=fake, **{**nothing, "changed": odd}) == I
    for parts in (0, -1, 4, 1 << 40):                                        # 300 lists are 3 tiles
        assert f(parts=parts, **{**nothing, "outs": fake}) == I
    assert f(B=BIG - 1, L_=BIG - 1, parts=1 << 24, **{**nothing, "outs": fake}) == U         # the grid
    for name in ("x", "c", "terms", "ps", "pl"):                             # the pointers, then the alignments
        assert f(**{name: None}, outs=odd) == I
    for name in ("x", "c", "terms", "outs", "prev", "ps", "pl"):
        assert f(**{name: odd}) == I
    assert f(prev=fake, changed=odd) == I


def test_update_checks_in_order_without_launch():
    m = _lib()
    L = m.lib()
    U, I = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL
    fake, odd4 = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    names = ("x", "order", "off", "cin", "cout", "counts", "first", "sums")

    def f(B=300, D=64, L_=7, **kw):
        p = {n: kw.get(n, fake) for n in names}
        return L.mcq_kmeans_update(p["x"], B, D, p["order"], p["off"], L_, p["cin"], p["cout"], p["counts"], p["first"], p["sums"], None)

    nothing = {n: None for n in names}
    assert f(D=16385, B=-1, L_=0, **nothing) == U
    for kw in (dict(D=0, B=BIG), dict(B=-1, L_=BIG), dict(L_=0, B=BIG)):
        assert f(**kw, **nothing) == I
    assert f(B=BIG, **nothing) == U and f(L_=BIG, **nothing) == U
    assert f(B=BIG - 1, L_=BIG - 1, **nothing) == U                          # ceil(B / 4096) + L: the grid
    for n in names:
        assert f(**{n: None}) == I
    assert f(B=0, x=None, order=None, off=None) == I                         # no vectors: the offsets are still needed
    for n in ("order", "off", "first", "sums"):                              # 8-byte alignment of the int64 and float64 pointers
        assert f(**{n: odd4}) == I
    for n in ("x", "cin", "cout", "counts"):
        assert f(**{n: ctypes.c_void_p((1 << 20) + 2)}) == I


def test_recommended_parts_and_block_counts():
    L = _lib().lib()
    for B in (1, 127, 129, 4096, 65535, 65536, 1 << 20):
        for lists in (1, 128, 129, 1024, 16384):
            parts, tiles, vt = L.mcq_kmeans_parts(B, lists, 512), -(-lists // 128), -(-B // 128)
            assert 1 <= parts <= tiles and (parts == 1 if vt >= 512 else parts == min(tiles, -(-512 // vt)))
            assert L.mcq_kmeans_blocks(B, lists, 70) == (-(-B // 4096) + lists) * 70
    assert L.mcq_kmeans_parts(1024, 16384, 512) == 64 and L.mcq_kmeans_parts(65536, 16384, 512) == 1
    assert L.mcq_kmeans_blocks(0, 5, 3) == 15 and L.mcq_kmeans_blocks(4097, 1, 1) == 3
    for bad in ((0, 100, 64), (-1, 100, 64), (4, 0, 64), (4, 100, 0), (4, 100, 16385), (BIG, 100, 64)):
        assert L.mcq_kmeans_parts(*bad) == 1 and (bad[0] == 0 or L.mcq_kmeans_blocks(*bad) == 0)
    assert L.mcq_kmeans_blocks(BIG - 1, BIG - 1, 1) == 0


def test_python_argument_errors_precede_device_work():
    import torch
    m = _lib()
    import quantization_amd as qa
    assert {"kmeans_step", "coarse_train"} <= set(qa.__all__)
    x, c = torch.zeros(30, 24), torch.zeros(5, 24)
    for call in (lambda: qa.kmeans_step(x, c), lambda: qa.coarse_train(x, 5), lambda: qa.coarse_train(x, 5, init=c)):
        with pytest.raises(m.McqError):                       # CPU tensors: no fallback
            call()
    i32 = torch.zeros(30, dtype=torch.int32)
    bad = ((lambda: qa.kmeans_step(x.half(), c), "vectors"), (lambda: qa.kmeans_step(x, c.double()), "centroids"),
           (lambda: qa.kmeans_step(x.reshape(3, 10, 24), c), "vectors"), (lambda: qa.kmeans_step(x, c[:0]), "at least one"),
           (lambda: qa.kmeans_step(x[:, :23], c), "vectors"), (lambda: qa.kmeans_step(x, c, terms=torch.zeros(4)), "terms"),
           (lambda: qa.kmeans_step(x, c, prev_assign=i32.long()), "prev_assign"),
           (lambda: qa.kmeans_step(x, c, prev_assign=i32[:29]), "prev_assign"),
           (lambda: qa.coarse_train(x, 0), "num_lists"), (lambda: qa.coarse_train(x, 5.0), "num_lists"),
           (lambda: qa.coarse_train(x, 31), "distinct rows"), (lambda: qa.coarse_train(x, 5, iters=-1), "iters"),
           (lambda: qa.coarse_train(x, 5, seed="a"), "seed"), (lambda: qa.coarse_train(x.half(), 5), "vectors"),
           (lambda: qa.coarse_train(torch.zeros(4, 16385), 2), "vectors"), (lambda: qa.coarse_train(x, 5, init=c[:4]), "init"),
           (lambda: qa.coarse_train(x, 5, init=c.half()), "init"))
    for call, match in bad:
        with pytest.raises(ValueError, match=match):
            call()
