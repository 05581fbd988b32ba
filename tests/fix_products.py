"""Host side of the value-by-value tests of the fixed-point products (quantization_amd/csrc/mcq_fix_kernels.h): the byte image of
a limb matrix, the product table and the logits of two sets of rows in exact integers (tests/logits_screen.py restates the
header's definition; nothing of it is copied here), where to look in an output too large to compare in full, and the rows at
which a fixed-point kernel goes wrong.  Plain helper module: tests/test_fix_products_host.py pins it on the CPU,
tests/test_gpu_fix_products.py compares the device with it."""
import numpy as np

from logits_screen import chain, limb_sums, limbs_of, t_exact

F = np.float32


def round_up(v, m):
    return (v + m - 1) // m * m


def planes_of(limbs, Rp, Dq):
    """byte image (uint8 [Rp * Dq * 4]) of a limb matrix (four [R][D] integer arrays, most significant first) in the layout
    of the header: limb l of row `row`, column k at ((c * 4 + l) * Rp + row) * 16 + k % 16 with c = k // 16; rows R .. Rp and
    columns D .. Dq are zeros"""
    R, D = limbs[0].shape
    assert Rp >= R and Dq >= D and Dq % 16 == 0
    img = np.zeros((Dq // 16, 4, Rp, 16), np.int8)
    for l in range(4):
        full = np.zeros((Rp, Dq), np.int64)
        full[:R, :D] = limbs[l]
        assert (full >= -128).all() and (full <= 127).all()
        img[:, l] = full.reshape(Rp, Dq // 16, 16).transpose(1, 0, 2)
    return img.reshape(-1).view(np.uint8)


def limbs_from_planes(img, Rp, Dq, R):
    """the inverse of planes_of for the first R rows: four int64 [R][Dq] limb matrices of a byte image"""
    a = np.asarray(img).view(np.int8).reshape(Dq // 16, 4, Rp, 16)
    return [a[:, l].transpose(1, 0, 2).reshape(Rp, Dq)[:R].astype(np.int64) for l in range(4)]


def _operand(v):
    """fp32 rows, or (limbs, exponents) as limbs_of / limbs_from_planes give them"""
    if isinstance(v, tuple):
        return v[0], np.asarray(v[1], np.int64)
    return limbs_of(v)


def _sums(la, lb):
    """limb_sums of two operands whose column counts may differ (rows against planes padded to Dq): the missing columns are zeros"""
    D = max(la[0].shape[1], lb[0].shape[1])
    wide = lambda ls: [np.pad(l, ((0, 0), (0, D - l.shape[1]))) for l in ls]
    return limb_sums(wide(la), wide(lb))


def fixdot_matrix(a_rows, b_rows):
    """fixdot(a_i, b_j) as fp32 [len(a)][len(b)]: ldexp(t_exact(limb_sums), ea + eb - 36), the result rounded once"""
    (la, ea), (lb, eb) = _operand(a_rows), _operand(b_rows)
    t = t_exact(_sums(la, lb))
    with np.errstate(over="ignore"):
        return np.ldexp(t.astype(np.float32), (ea[:, None] + eb[None, :] - 36).astype(np.int32)).astype(np.float32)


def logits_of(frames, w_rows, wmu, lscale, bias):
    """[B][rows] logits of (centered) frames against classifier rows: ((fixdot + wmu[r]) * lscale) + bias[r], one fp32
    operation each (logits_screen.chain)"""
    (lx, ex), (lw, ew) = _operand(frames), _operand(w_rows)
    t = t_exact(_sums(lx, lw))
    e = ex[:, None] + ew[None, :] - 36
    return chain(t, e, np.asarray(wmu, np.float32)[None, :], lscale, np.asarray(bias, np.float32)[None, :])[2]


def sample_index(n):
    """ascending indices into [0, n): two in every 32-wide band of every 128-wide tile (one where the last band has a single
    index), at offsets that differ from band to band, and the first and the last index"""
    out = {0, n - 1}
    for band, s in enumerate(range(0, n, 32)):
        width = min(32, n - s)
        out.add(s + (7 * band + 3) % width)
        out.add(s + (13 * band + 20) % width)
        if width > 1 and (7 * band + 3) % width == (13 * band + 20) % width:
            out.add(s + (7 * band + 4) % width)
    return np.array(sorted(out), np.int64)


EDGE_K = 3          # the power of two of the "max exactly 2^k" rows
Q_M128 = -8421504   # limbs (0, -128, -128, -128)


def edge_rows(D, rs):
    """named fp32 rows of D elements, all finite; element 0 carries the row's largest magnitude wherever the name speaks of one
    (D == 1 leaves only that element).  tests/test_fix_products_host.py checks the limbs and exponent each name claims."""
    u = lambda lo, hi: rs.uniform(lo, hi, size=D)
    rows = {}
    rows["zeros"] = np.zeros(D)                                   # e = -125, every product exactly 0
    v = u(-0.9, 0.9) * 2.0 ** EDGE_K
    v[0] = 2.0 ** EDGE_K
    rows["max_pow2"] = v                                          # e = k + 1, q[0] = 2^29
    rows["max_neg_pow2"] = -v                                     # q[0] = -2^29
    v = u(-0.9, 0.9) * 2.0 ** EDGE_K
    v[0] = np.nextafter(F(2.0 ** EDGE_K), F(0))
    rows["max_below_pow2"] = v                                    # e = k, q[0] = 2^30 - 64
    rows["denormals"] = rs.randint(-1000, 1001, size=D) * 2.0 ** -149     # fp32 denormals (about 1e-42): e = -125, q = 64 n
    rows["denormals"][0] = 714 * 2.0 ** -149
    v = u(-1.0, 1.0) * (3e38 / D)
    v[0] = 3e38
    rows["huge"] = v                                              # e = 128; finite products with partners below 1/2
    rows["huge_pos"] = u(0.5, 1.0) * 3e38                         # against itself every term is +: the product is +inf
    rows["huge_pos"][0] = 3e38
    v = u(0.1, 1.0) * 2.0 ** -32 * rs.choice([-1.0, 1.0], size=D)
    v[0] = 1.0
    rows["tiny_tail"] = v                                         # e = 1; the rest below 2^-31 of the max: q = 0
    m = rs.randint(-40, 40, size=D)
    v = (m + 0.5) * 2.0 ** -29
    v[0] = 1.0
    rows["half_ties"] = v                                         # e = 1; q = rint(m + 1/2): ties to even
    v = np.full(D, Q_M128 * 2.0 ** -29)
    v[0] = 1.0
    rows["limbs_m128"] = v                                        # e = 1; the rest at q = -8,421,504: the largest |T_s| there is
    rows["wide_range"] = rs.standard_normal(D) * np.exp(u(-8.0, 8.0))
    out = {k: np.asarray(v, np.float64).astype(np.float32) for k, v in rows.items()}
    assert all(np.isfinite(v).all() for v in out.values())
    return out
