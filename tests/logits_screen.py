"""Host restatement (numpy, exact integers) of the screened arg max of the logits product: k_fgemm<FG_SCREEN> in
quantization_amd/csrc/mcq_fix_kernels.h picks the winner of a (frame, codebook) pair from limbs 0-2 of both operands and
lists the pair for the exact recheck unless best' - second' > margin (with the second's row, when the third value is
clearly below: two exact logits settle it then).  This module forms, for limb matrices, the exact logits L (ten limb
products), the screened ones L' (six), the margin as the kernel forms it (fp32, same constants) and the decision; the
tests assert what the kernel's comment proves."""
import numpy as np

F = np.float32


def limbs_of(v):
    """fp32 rows -> (four int64 limb matrices, most significant first; row exponents): fix_q / limbs4 of mcq_fix_kernels.h"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    m = np.abs(v).max(axis=1) if v.shape[1] else np.zeros(len(v), np.float32)
    be = ((m.view(np.uint32) >> 23) & 0xff).astype(np.int64)
    e = np.maximum(be, 1) - 126
    q = np.rint(np.ldexp(v.astype(np.float64), (30 - e)[:, None]))
    q = np.clip(q, -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    out, r = [], q
    for _ in range(3):
        l = ((r & 0xff) + 128) % 256 - 128
        out.append(l)
        r = (r - l) >> 8
    out.append(r)
    return out[::-1], e


def rn24(n):
    """an int64 rounded to 24 significant bits, ties to even: (float)n for the integers the chains meet (all < 2^62)"""
    n = np.asarray(n, dtype=np.int64)
    a = np.abs(n)
    nb = np.zeros(a.shape, np.int64)
    t = a.copy()
    for s in (32, 16, 8, 4, 2, 1):
        big = t >= (np.int64(1) << s)
        nb += np.where(big, s, 0)
        t = np.where(big, t >> s, t)
    nb += (t > 0)
    sh = np.maximum(nb - 24, 0)
    half = np.where(sh > 0, np.int64(1) << np.maximum(sh - 1, 0), 0)
    lo = a & ((np.int64(1) << sh) - 1)
    hi = a >> sh
    up = (lo > half) | ((lo == half) & (sh > 0) & ((hi & 1) == 1))
    return np.sign(n) * ((hi + up) << sh)


def limb_sums(la, lb):
    """T_s[a_row][b_row], s = 0..3, exact (the sums stay below 2^53: float64 matrix products are exact)"""
    T = [0, 0, 0, 0]
    fa = [x.astype(np.float64) for x in la]
    fb = [x.astype(np.float64) for x in lb]
    for i in range(4):
        for j in range(4 - i):
            T[i + j] = T[i + j] + fa[i] @ fb[j].T
    return [np.asarray(t).astype(np.int64) for t in T]


def t_exact(T):
    r = rn24(T[3])
    r = rn24(rn24(T[2]) * 256 + r)
    r = rn24(rn24(T[1]) * 65536 + r)
    return rn24(rn24(T[0]) * 16777216 + r)


def t_screen(T):
    r = rn24(T[2]) * 256
    r = rn24(rn24(T[1]) * 65536 + r)
    return rn24(rn24(T[0]) * 16777216 + r)


def chain(t, e, wmu, ls, bias):
    """(y, s2, L) of the epilogue, one fp32 operation each"""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.ldexp(t.astype(np.float32), e.astype(np.int32)).astype(np.float32)
        s1 = (y + wmu).astype(np.float32)
        s2 = (s1 * F(ls)).astype(np.float32)
        return y, s2, (s2 + bias).astype(np.float32)


def screen(lx, ex, lw, ew, wmu, bias, ls, N, K):
    """frames (lx, ex) against classifier rows (lw, ew).  Returns a dict of [B][N] arrays: `winner` (screened first arg max),
    `undecided`, `exact` (first arg max of the ten-product logits), `margin`, and [B][N][K]: `L`, `Ls`."""
    B, Dq = lx[0].shape
    Dq = (Dq + 127) // 128 * 128          # the kernel's padded inner dimension
    T = limb_sums(lx, lw)
    e = (ex[:, None] + ew[None, :] - 36)
    wmu = np.asarray(wmu, np.float32)[None, :]
    bias = np.asarray(bias, np.float32)[None, :]
    _, _, L = chain(t_exact(T), e, wmu, ls, bias)
    _, s2, Ls = chain(t_screen(T), e, wmu, ls, bias)
    L, Ls, s2 = (a.reshape(B, N, K) for a in (L, Ls, s2))
    winner = Ls.argmax(axis=2)
    srt = np.sort(Ls, axis=2)
    ninf = np.full((B, N), -np.inf, np.float32)
    best, second, third = srt[:, :, -1], (srt[:, :, -2] if K > 1 else ninf), (srt[:, :, -3] if K > 2 else ninf)
    q = np.maximum(np.abs(s2), np.abs(Ls)).max(axis=2).astype(np.float32)
    em = ew.reshape(N, K).max(axis=1)
    cA = F(16.5) * F(16384.0) * F(Dq)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.ldexp(np.full((B, N), cA, np.float32), (em[None, :] + ex[:, None] - 36).astype(np.int32)).astype(np.float32)
        margin = ((d * F(ls)).astype(np.float32) + (q * F(2.0 ** -19)).astype(np.float32)).astype(np.float32)
        margin = (margin + F(2.0 ** -120)).astype(np.float32)
        undecided = ~((best - second).astype(np.float32) > margin)
        many = ~((best - third).astype(np.float32) > margin)      # more than two contenders: the recheck redoes all K rows
    return dict(winner=winner, undecided=undecided, many=many, exact=L.argmax(axis=2), margin=margin, L=L, Ls=Ls)


def assert_sound(r, what):
    """what the kernel's comment proves: |L - L'| <= margin / 2 for every row; a decided pair's screened winner is the exact first
    arg max; an undecided pair's exact winner is among its contenders (screened value within `margin` of the best)"""
    L, Ls, m = r["L"].astype(np.float64), r["Ls"].astype(np.float64), r["margin"].astype(np.float64)
    fin = np.isfinite(m)
    err = np.abs(L - Ls).max(axis=2)
    assert (err[fin] <= 0.5 * m[fin]).all(), f"{what}: |L - L'| reaches {np.max(err[fin] / m[fin]):.3f} of the margin (bound 0.5)"
    dec = ~r["undecided"]
    assert (r["winner"][dec] == r["exact"][dec]).all(), f"{what}: a decided pair's winner differs from the exact arg max"
    lw = np.take_along_axis(Ls, r["exact"][:, :, None], axis=2)[:, :, 0]
    und = r["undecided"] & fin
    assert (lw[und] >= Ls.max(axis=2)[und] - m[und]).all(), f"{what}: the exact winner is outside an undecided pair's contenders"
    # two contenders (the third value is clearly below): the exact winner is one of the two best screened rows
    two = r["undecided"] & ~r["many"]
    top2 = np.argsort(-Ls, axis=2, kind="stable")[:, :, :2]
    assert (top2 == r["exact"][:, :, None]).any(axis=2)[two].all(), f"{what}: the exact winner is neither of an undecided pair's two contenders"
    return float(r["undecided"].mean())


def state_operands(state, x):
    """limbs of the centred frames and of the classifier rows, wmu, bias, ls of a quantizer state (the data mean as the mean of
    the scaled centers summed over the codebooks, formed here in fp32: a stand-in that shifts the frames as the kernels do)"""
    scales = getattr(state, "scales_exp", None)
    cs = F(scales[0]) if scales else np.exp(F(10.0) * F(state["centers_scale"])).astype(np.float32)
    ls = F(scales[1]) if scales else np.exp(F(10.0) * F(state["logits_scale"])).astype(np.float32)
    C = (np.asarray(state["centers"], np.float32) * cs).astype(np.float32)
    mean = C.mean(axis=1, dtype=np.float32).sum(axis=0, dtype=np.float32)
    W = np.asarray(state["to_logits.weight"], np.float32)
    lw, ew = limbs_of(W)
    lm, emu = limbs_of(mean[None, :])
    tm = t_exact([t[0] for t in limb_sums(lm, lw)])
    wmu = np.ldexp(tm.astype(np.float32), (emu[0] + ew - 36).astype(np.int32)).astype(np.float32)
    lx, ex = limbs_of((np.asarray(x, np.float32) - mean[None, :]).astype(np.float32))
    return lx, ex, lw, ew, wmu, np.asarray(state["to_logits.bias"], np.float32), float(ls)
