"""tests/fix_products.py pinned on the CPU (not gpu): the plane image byte by byte against a hand-written example, the product
table against the scalar restatement in Python integers of tests/test_oracle_fixdot.py, every edge row against the limbs and the
exponent its name claims, the sampling of large outputs, and the layout hook mcq_test_prepared_layout against the size
queries of the ABI over the whole (N, K) domain."""
import ctypes

import numpy as np

import fix_products as fp
from logits_screen import limbs_of
from test_oracle_fixdot import _fixdot

ORDER = ("C", "Q", "Cf", "Ce", "Wf", "We", "wmu", "bias", "scales", "mean", "cmean", "G", "total")


def test_planes_of_by_hand():
    # 2 rows x 17 columns in a 128-row, 128-column frame (the smallest the kernels use): column 16 opens chunk 1
    R, D, Rp, Dq = 2, 17, 128, 128
    limbs = [np.zeros((R, D), np.int64) for _ in range(4)]
    limbs[0][0, 0] = 64
    limbs[0][1, 15] = -32
    limbs[1][1, 0] = -128
    limbs[2][0, 16] = 127
    limbs[3][1, 16] = -1
    limbs[3][0, 5] = 7
    img = fp.planes_of(limbs, Rp, Dq)
    assert img.dtype == np.uint8 and img.size == Rp * Dq * 4
    want = {((0 * 4 + 0) * Rp + 0) * 16 + 0: 64,            # limb 0, row 0, column 0
            ((0 * 4 + 0) * Rp + 1) * 16 + 15: 0xE0,         # limb 0, row 1, column 15: -32
            ((0 * 4 + 1) * Rp + 1) * 16 + 0: 0x80,          # limb 1, row 1, column 0: -128
            ((1 * 4 + 2) * Rp + 0) * 16 + 0: 127,           # limb 2, row 0, column 16: chunk 1, byte 0
            ((1 * 4 + 3) * Rp + 1) * 16 + 0: 0xFF,          # limb 3, row 1, column 16: -1
            ((0 * 4 + 3) * Rp + 0) * 16 + 5: 7}             # limb 3, row 0, column 5
    assert want == {2048 * 0 + 0: 64, 31: 0xE0, 2048 + 16: 0x80, 6 * 2048: 127, 7 * 2048 + 16: 0xFF, 3 * 2048 + 5: 7}
    for at, byte in want.items():
        assert img[at] == byte, (at, img[at], byte)
    assert np.count_nonzero(img) == len(want)
    back = fp.limbs_from_planes(img, Rp, Dq, R)
    for l in range(4):
        assert np.array_equal(back[l][:, :D], limbs[l]) and not back[l][:, D:].any()


def test_planes_round_trip_random():
    rs = np.random.RandomState(1)
    for R, D, Rp, Dq in ((5, 1, 128, 128), (130, 129, 256, 256), (128, 640, 128, 640)):
        limbs, _ = limbs_of(rs.standard_normal((R, D)).astype(np.float32))
        img = fp.planes_of(limbs, Rp, Dq)
        back = fp.limbs_from_planes(img, Rp, Dq, Rp)
        for l in range(4):
            assert np.array_equal(back[l][:R, :D], limbs[l])
            assert not back[l][R:].any() and not back[l][:, D:].any()
        # one byte by the formula
        r, k, l = R - 1, D - 1, 2
        assert img[(((k // 16) * 4 + l) * Rp + r) * 16 + k % 16] == (int(limbs[l][r, k]) & 0xff)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fixdot_matrix_vs_scalar_definition_on_edge_rows():
    rs = np.random.RandomState(2)
    for D in (1, 2, 17, 45):
        rows = fp.edge_rows(D, rs)
        names = list(rows)
        A = np.stack([rows[n] for n in names])
        M = np.concatenate([A, rs.uniform(-0.5, 0.5, size=(3, D)).astype(np.float32)])      # modest partners
        got = fp.fixdot_matrix(A, M)
        with np.errstate(over="ignore"):
            want = np.array([[_fixdot(a, b) for b in M] for a in A], np.float32)
        assert np.array_equal(_bits(got), _bits(want)), (D, np.argwhere(_bits(got) != _bits(want))[:4])
        # (limbs, exponents) operands give the same table
        assert np.array_equal(_bits(fp.fixdot_matrix(limbs_of(A), limbs_of(M))), _bits(got))
        # ... and so do rows against an operand read back from planes, which is padded to 128 columns
        lm, em = limbs_of(M)
        planes = (fp.limbs_from_planes(fp.planes_of(lm, 128, 128), 128, 128, len(M)), em)
        assert np.array_equal(_bits(fp.fixdot_matrix(A, planes)), _bits(got))
        i = names.index("huge_pos")
        assert got[i, i] == np.inf
        assert not got[names.index("zeros")].any() and np.isfinite(got[names.index("huge"), len(names):]).all()
        assert not np.isnan(got).any()
        # the logits: chain with wmu, lscale and bias, one fp32 operation each
        wmu = rs.standard_normal(len(M)).astype(np.float32)
        bias = rs.standard_normal(len(M)).astype(np.float32)
        ls = np.float32(1.7)
        with np.errstate(over="ignore"):
            L = ((got + wmu[None, :]).astype(np.float32) * ls).astype(np.float32) + bias[None, :]
        assert np.array_equal(_bits(fp.logits_of(A, M, wmu, ls, bias)), _bits(L))


def _limbs_row(v):
    l, e = limbs_of(v[None, :])
    return np.stack([x[0] for x in l], axis=1), int(e[0])          # [D][4], exponent


def test_edge_rows_are_what_their_names_say():
    rs = np.random.RandomState(3)
    for D in (2, 17, 130):
        rows = fp.edge_rows(D, rs)
        k = fp.EDGE_K
        q = lambda l: ((l[:, 0] * 256 + l[:, 1]) * 256 + l[:, 2]) * 256 + l[:, 3]
        l, e = _limbs_row(rows["zeros"])
        assert e == -125 and not l.any()
        l, e = _limbs_row(rows["max_pow2"])
        assert e == k + 1 and list(l[0]) == [32, 0, 0, 0] and (np.abs(q(l)[1:]) < 2 ** 29).all()
        l, e = _limbs_row(rows["max_neg_pow2"])
        assert e == k + 1 and list(l[0]) == [-32, 0, 0, 0]
        l, e = _limbs_row(rows["max_below_pow2"])
        assert e == k and q(l)[0] == 2 ** 30 - 64 and list(l[0]) == [64, 0, 0, -64]
        v = rows["denormals"]
        assert (np.abs(v) < np.finfo(np.float32).tiny).all() and v[0] != 0 and abs(float(v[0]) - 1e-42) < 1e-44
        l, e = _limbs_row(v)
        n = np.rint(v.astype(np.float64) * 2.0 ** 149).astype(np.int64)
        assert e == -125 and np.array_equal(q(l), 64 * n) and q(l)[0] == 64 * 714
        for name in ("huge", "huge_pos"):
            l, e = _limbs_row(rows[name])
            assert e == 128 and rows[name][0] == np.float32(3e38) and np.isfinite(rows[name]).all()
        assert (rows["huge_pos"] > 0).all()
        l, e = _limbs_row(rows["tiny_tail"])
        assert e == 1 and q(l)[0] == 2 ** 29 and not l[1:].any() and (rows["tiny_tail"][1:] != 0).all()
        assert (np.abs(rows["tiny_tail"][1:]) < 2.0 ** -31).all()
        v = rows["half_ties"]
        l, e = _limbs_row(v)
        s = v[1:].astype(np.float64) * 2.0 ** 29
        assert e == 1 and (s - np.floor(s) == 0.5).all()                       # exact ties ...
        assert np.array_equal(q(l)[1:], np.where(np.floor(s) % 2 == 0, np.floor(s), np.floor(s) + 1).astype(np.int64))   # ... to even
        l, e = _limbs_row(rows["limbs_m128"])
        assert e == 1 and list(l[0]) == [32, 0, 0, 0]
        assert (l[1:] == np.array([0, -128, -128, -128])).all() and (q(l)[1:] == fp.Q_M128).all()
        v = rows["wide_range"]
        assert np.abs(v).max() / np.abs(v[v != 0]).min() > (1.0 if D < 17 else 100.0)
    assert len(fp.edge_rows(1, rs)) == len(rows)


def test_sample_index_covers_every_band():
    for n in (1, 2, 31, 33, 128, 129, 2048, 2300, 4096):
        idx = fp.sample_index(n)
        assert idx[0] == 0 and idx[-1] == n - 1 and (np.diff(idx) > 0).all() and len(idx) <= 300
        for s in range(0, n, 32):
            inside = ((idx >= s) & (idx < min(s + 32, n))).sum()
            assert inside >= min(2, min(32, n - s)), (n, s)
    # the offsets inside a band differ from band to band (a fixed lane of the tile would check one lane's path only)
    assert len(set(fp.sample_index(4096) % 32)) > 16


def test_prepared_layout_hook_over_the_domain():
    from quantization_amd import _lib as m
    L = m.lib()
    off = (ctypes.c_size_t * 16)()
    seen = 0
    for D in (1, 16, 17, 512):
        Dp = (D + 15) // 16 * 16
        for K in (16, 32, 64, 128, 256, 512, 1024):
            for N in (1, 2, 4, 8, 16, 32, 64):
                if N * K > 16384:
                    assert L.mcq_test_prepared_layout(N, K, D, off, 16) == m.MCQ_EUNSUPPORTED
                    continue
                for i in range(16):
                    off[i] = 0xdead
                assert L.mcq_test_prepared_layout(N, K, D, off, 16) == len(ORDER)
                o = dict(zip(ORDER, list(off)[:len(ORDER)]))
                assert list(off)[len(ORDER):] == [0xdead] * 3
                vals = [o[n] for n in ORDER]
                assert vals[0] == 0 and all(a < b for a, b in zip(vals, vals[1:])), (N, K, D, vals)
                assert all(v % 256 == 0 for v in vals)
                assert o["mean"] == L.mcq_prepared_mean_offset(N, K, D)
                assert o["Cf"] == L.mcq_prepared_decode_bytes(N, K, D)
                assert o["total"] == L.mcq_prepared_bytes(N, K, D)
                nk, Rp, Dq = N * K, fp.round_up(N * K, 128), fp.round_up(D, 128)
                # the bias tile the product kernel copies without a bound check lies inside the blob
                assert o["total"] - o["bias"] >= 4 * (nk + 128)
                assert o["total"] - o["wmu"] >= 4 * (nk + 128)
                # every array fits before the next one starts
                room = {"C": nk * Dp * 4, "Q": nk * 4, "Cf": Rp * Dq * 4, "Ce": Rp * 4, "Wf": Rp * Dq * 4, "We": Rp * 4,
                        "wmu": nk * 4, "bias": nk * 4, "scales": 8, "mean": Dp * 4, "cmean": N * Dp * 4, "G": nk * nk * 4}
                for a, b in zip(ORDER, ORDER[1:]):
                    assert o[a] + room[a] <= o[b], (N, K, D, a)
                seen += 1
    assert seen == 4 * (5 * 7 + 6 + 5)          # K <= 256: every N; K = 512: N <= 32; K = 1024: N <= 16
    # cap limits what is written, not what is returned; rejections as the neighbouring entries give them
    off[0] = off[1] = off[2] = 0xdead
    assert L.mcq_test_prepared_layout(8, 256, 64, off, 2) == len(ORDER) and off[0] == 0 and off[1] != 0xdead and off[2] == 0xdead
    assert L.mcq_test_prepared_layout(8, 256, 64, off, 0) == len(ORDER)
    assert L.mcq_test_prepared_layout(8, 256, 64, None, 13) == m.MCQ_EINVAL
    assert L.mcq_test_prepared_layout(8, 256, 64, off, -1) == m.MCQ_EINVAL
    assert L.mcq_test_prepared_layout(3, 256, 64, off, 13) == m.MCQ_EINVAL
    assert L.mcq_test_prepared_layout(8, 8, 64, off, 13) == m.MCQ_EUNSUPPORTED
    assert L.mcq_test_prepared_layout(8, 256, 20000, off, 13) == m.MCQ_EUNSUPPORTED
    assert L.mcq_test_prepared_layout(8, 256, 0, off, 13) == m.MCQ_EINVAL
