"""The trainer's kernels one by one against float64 restatements of what they compute.

Each test calls an entry point of include/mcq.h through the C ABI on arrays it builds itself, twice (the sums have a fixed
order: the two results must be bit-identical), and compares the result with the same operation written in plain torch
float64.  No reference calls a library kernel.

Tolerance rule, per entry and never per tensor:  |got - ref| <= c * L * 2^-24 * S, where S is the same expression evaluated in
float64 on absolute values (sum |t_i| for a sum, |G|^T |x| for a product), L the longest addition chain of the kernel (from
tests/train_grid.py, which mirrors the launch arithmetic) and c <= 4, written down in each test.  Where log-probabilities enter,
the ABI stores lse in fp32 and forms z - lse, while the reference subtracts the row maximum first: those bounds carry one more
term, 2^-24 * |lse| per row (a limit of the ABI, which dominates at the common offset of 1,000; not a loosened bound).

The largest ratio of error to bound seen by each entry point is written to the JSON file that MCQ_TRAIN_RATIOS names, if set.
"""
import json
import math
import os

import pytest
import torch

import train_grid as tg

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
UFL = 2.0 ** -126      # smallest normal fp32: the absolute error of a probability that underflows
RATIOS = {}

# (K, N, B, logits regime) of mcq_loss_fwd / mcq_loss_bwd(_ex)
LOSS_CASES = [(16, 1, 1, "trained"), (16, 64, 3, "trained"), (32, 1, 63, "spread200"), (32, 64, 65, "trained"),
              (64, 1, 333, "trained"), (64, 64, 63, "offset1000"), (128, 8, 65, "spread200"), (128, 1, 3, "trained"),
              (256, 64, 333, "trained"), (256, 1, 1, "offset1000"), (16, 2, 1024, "trained"), (64, 2, 4097, "offset1000"),
              (16, 1, 65537, "trained"), (32, 1, 65537, "spread200"), (16, 1, 1_048_575, "trained")]
# (D, N, K, x 16-byte aligned) of mcq_recon_fwd
RECON_CASES = [(1, 1, 16, True), (3, 64, 16, True), (30, 8, 256, True), (130, 64, 256, True), (514, 1, 256, True),
               (777, 64, 16, True), (64, 1, 16, True), (512, 64, 256, True), (768, 8, 256, True), (64, 8, 16, False),
               (512, 1, 256, False)]
# (nparts, N, K) of mcq_loss_head / mcq_loss_tail / mcq_loss_head_tail
HT_CASES = [(1, 1, 16), (255, 3, 256), (256, 64, 16), (257, 64, 256), (100000, 3, 16), (100000, 64, 256), (257, 1, 256)]
# (D, K, B, N) of mcq_decode_backward_u8_ex
DB_CASES = [(768, 256, 4097, 8), (320, 16, 4097, 16), (512, 16, 4097, 16), (600, 16, 1, 16), (4096, 16, 1000, 4),
            (30, 16, 4097, 2), (512, 256, 0, 8), (128, 16, 4097, 4), (64, 64, 1, 4)]
# (B, M, D) of mcq_weight_grad: the shapes of test_gpu_trainer.py, empty and short splits, both sides of the bf16-piece gate
WGRAD_CASES = [(4096, 2048, 512), (600, 1024, 256), (333, 128, 40), (65, 32, 30), (2048, 1024, 1024), (8200, 128, 64),
               (16385, 1024, 128), (2047, 1024, 128), (2048, 1024, 128), (333, 16, 1), (333, 16, 3), (333, 16, 130)]
ADAM_SIZES = [1, 3, 4099, 2097152, 2097155, 2099208]
TAIL_SIZES = [0, 1, 1023, 1024, 8192, 8193, 100000]


@pytest.fixture(scope="module", autouse=True)
def _report_ratios():
    yield
    path = os.environ.get("MCQ_TRAIN_RATIOS")
    if path:
        with open(path, "w") as f:
            json.dump(RATIOS, f, indent=1, sort_keys=True)


def _lib():
    from quantization_amd import _lib as m
    return m.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _check(entry, what, got, ref, bound):
    """every entry of got (fp32) within bound (fp64) of ref (fp64); records the largest error / bound"""
    got, ref, bound = got.double().reshape(-1), ref.double().reshape(-1), bound.double().reshape(-1)
    err = (got - ref).abs()
    assert torch.isfinite(got).all(), (entry, what)
    bad = err > bound
    if bad.any():
        i = int(bad.nonzero()[0, 0])
        raise AssertionError(f"{entry} {what}: {int(bad.sum())} of {err.numel()} entries out of bound; first at {i}: "
                             f"got {float(got[i])!r} ref {float(ref[i])!r} bound {float(bound[i])!r}")
    r = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
    RATIOS[entry] = max(RATIOS.get(entry, 0.0), r)


def _same(a, b, what):
    for x, y in zip(a, b):
        assert torch.equal(x, y), f"{what}: two runs differ"


# ---------------------------------------------------------------------------------------------- softmax statistics
def _logits(B, N, K, regime, gen):
    dev = torch.device("cuda:0")
    if regime == "trained":      # row maxima about 10 to 30
        z = torch.randn(B, N, K, device=dev, generator=gen) * 4 + torch.rand(B, N, 1, device=dev, generator=gen) * 10 + 5
    elif regime == "spread200":  # most probabilities underflow in fp32
        z = torch.rand(B, N, K, device=dev, generator=gen) * 200 - 100
    else:                        # a common offset of 1,000
        z = torch.randn(B, N, K, device=dev, generator=gen) * 3 + 1000
    idx = torch.randint(0, K, (B, N), device=dev, generator=gen)
    drop = torch.rand(B, N, device=dev, generator=gen) < 0.1      # negative targets: no index here
    drop[0] = False
    idx[drop] = -1
    return z.contiguous(), idx.contiguous()


def _softmax_ref(z, K):
    """fp64 lse, log-probs, probabilities, and the error budget of a log-probability formed as z - lse (fp32 lse):
    2^-24 |lse| (the ABI term) + 4 * 2^-24 * (|lp| + row chain + log sum exp(z - max) + 2) (c = 4)"""
    z64 = z.double()
    lse = torch.logsumexp(z64, dim=-1, keepdim=True)
    lp = z64 - lse
    lse_shift = lse - z64.amax(dim=-1, keepdim=True)
    e_lp = EPS * lse.abs() + 4 * EPS * (lp.abs() + tg.row_chain(K) + lse_shift + 2)
    return lse, lp, lp.exp(), e_lp, lse_shift


@pytest.mark.parametrize("K,N,B,regime", LOSS_CASES, ids=lambda v: str(v))
def test_loss_fwd_matches_float64(K, N, B, regime):
    """mcq_loss_fwd: lse per row, chosen_sum, prob_sum and count against fp64 (log_softmax of the same fp32 logits).
    c = 4, L = tg.loss_fwd_chain (a lane's rows, the row slots and waves, the chunks); lse and every term built on z - lse
    carry the ABI's 2^-24 |lse| (module docstring).  count is exact."""
    L = _lib()
    gen = torch.Generator(device="cuda:0").manual_seed(1000 * K + 7 * N + B)
    z, idx = _logits(B, N, K, regime, gen)
    dev = z.device
    ws = torch.empty(L.mcq_loss_workspace_bytes(B, N, K), dtype=torch.uint8, device=dev)

    def run():
        lse = torch.empty(B, N, device=dev)
        ch, ps, cnt = torch.empty(N, device=dev), torch.empty(N, K, device=dev), torch.empty(N, K, device=dev)
        assert L.mcq_loss_fwd(z.data_ptr(), idx.data_ptr(), B, N, K, lse.data_ptr(), ch.data_ptr(), ps.data_ptr(),
                              cnt.data_ptr(), ws.data_ptr(), ws.numel(), _st()) == 0
        torch.cuda.synchronize()
        return lse, ch, ps, cnt

    a = run()
    _same(a, run(), "mcq_loss_fwd")
    lse, ch, ps, cnt = a
    lse_r, lp, p, e_lp, shift = _softmax_ref(z, K)
    valid = (idx >= 0).unsqueeze(-1)
    _check("mcq_loss_fwd", "lse", lse, lse_r.squeeze(-1),
           EPS * lse_r.abs().squeeze(-1) + 4 * EPS * (tg.row_chain(K) + shift.squeeze(-1) + 1))
    Lc = tg.loss_fwd_chain(B, K)
    pv = p * valid
    _check("mcq_loss_fwd", "prob_sum", ps, pv.sum(0), 4 * Lc * EPS * pv.sum(0) + (pv * (e_lp + 2 * EPS)).sum(0))
    sel = idx.clamp_min(0).unsqueeze(-1)
    lpc = lp.gather(-1, sel).squeeze(-1) * valid.squeeze(-1)
    elc = e_lp.gather(-1, sel).squeeze(-1) * valid.squeeze(-1)
    _check("mcq_loss_fwd", "chosen_sum", ch, lpc.sum(0), 4 * Lc * EPS * lpc.abs().sum(0) + elc.sum(0))
    ref_cnt = torch.zeros(N, K, dtype=torch.float64, device=dev)
    ref_cnt.scatter_add_(1, idx.clamp_min(0).t().contiguous(), valid.squeeze(-1).t().double().contiguous())
    assert torch.equal(cnt.double(), ref_cnt), "count"


@pytest.mark.parametrize("K,N,B,regime", LOSS_CASES, ids=lambda v: str(v))
def test_loss_bwd_matches_float64(K, N, B, regime):
    """mcq_loss_bwd and mcq_loss_bwd_ex: each gradient entry against fp64 gc (delta - p) + p (g_k - sum_j p_j g_j), and each
    wave's dot_part against fp64 sum G (z - bias) over its rows.  lse is handed in as the fp32 rounding of the fp64 lse; p
    carries the ABI term 2^-24 |lse| through e_lp (module docstring), and each probability the absolute 2^-126 of fp32's
    normal range (the spread of 200 underflows most of them).  c = 4, L = values per lane + butterfly depth + 3."""
    L = _lib()
    gen = torch.Generator(device="cuda:0").manual_seed(2000 * K + 7 * N + B)
    z, idx = _logits(B, N, K, regime, gen)
    dev = z.device
    lse_r, lp, p, e_lp, _ = _softmax_ref(z, K)
    lse32 = lse_r.squeeze(-1).float().contiguous()
    gprob = (torch.randn(N, K, device=dev, generator=gen) * 0.3 + torch.linspace(-1, 2, K, device=dev)).contiguous()
    gc = torch.tensor([0.37], device=dev)
    bias = (torch.randn(N, K, device=dev, generator=gen) * 0.5).contiguous()
    waves = L.mcq_loss_bwd_waves(B, N, K)

    def run():
        g1, g2 = torch.empty(B, N, K, device=dev), torch.empty(B, N, K, device=dev)
        dp = torch.empty(waves, device=dev)
        assert L.mcq_loss_bwd(z.data_ptr(), idx.data_ptr(), lse32.data_ptr(), B, N, K, gc.data_ptr(), gprob.data_ptr(),
                              g1.data_ptr(), _st()) == 0
        assert L.mcq_loss_bwd_ex(z.data_ptr(), idx.data_ptr(), lse32.data_ptr(), B, N, K, gc.data_ptr(), gprob.data_ptr(),
                                 g2.data_ptr(), bias.data_ptr(), dp.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        return g1, g2, dp

    a = run()
    _same(a, run(), "mcq_loss_bwd(_ex)")
    g1, g2, dp = a
    assert torch.equal(g1, g2), "mcq_loss_bwd and mcq_loss_bwd_ex differ"
    g64, gcv = gprob.double(), float(gc)
    valid = (idx >= 0).unsqueeze(-1).double()
    delta = torch.zeros_like(p).scatter_(-1, idx.clamp_min(0).unsqueeze(-1), 1.0)
    dot = (p * g64).sum(-1, keepdim=True)
    A = (p * g64.abs()).sum(-1, keepdim=True)
    ref = valid * (gcv * (delta - p) + p * (g64 - dot))
    Lr = tg.row_chain(K) + 3
    S = abs(gcv) * (delta + p) + p * (g64.abs() + A)
    bound = valid * (4 * Lr * EPS * S + e_lp * p * (abs(gcv) + g64.abs() + A) + p * (p * g64.abs() * e_lp).sum(-1, keepdim=True)
                     + UFL * (abs(gcv) + g64.abs() + g64.abs().sum(-1, keepdim=True)))
    _check("mcq_loss_bwd", "grad", g1, ref, bound)
    # per-wave partials of sum G (z - bias): wave w holds rows [w RPW, (w + 1) RPW) of the (b, n) rows
    zb = z.double() - bias.double()
    rows = (ref * zb).sum(-1).reshape(-1)
    rows_s = (ref.abs() * (z.double().abs() + bias.double().abs())).sum(-1).reshape(-1)
    rows_b = (bound * zb.abs()).sum(-1).reshape(-1)
    rpw = tg.rows_per_wave(K)
    pad = waves * rpw - rows.numel()
    assert pad >= 0
    per = [torch.cat([t, t.new_zeros(pad)]).reshape(waves, rpw).sum(1) for t in (rows, rows_s, rows_b)]
    Ld = K // min(K, 64) + 6 + rpw + 2
    _check("mcq_loss_bwd_ex", "dot_part", dp, per[0], 4 * Ld * EPS * per[1] + per[2])
    _check("mcq_loss_bwd_ex", "sum(dot_part)", dp.double().sum(), per[0].sum(),
           (4 * Ld * EPS * per[1] + per[2]).sum() + 4 * math.log2(max(waves, 2)) * EPS * per[1].sum())


# ---------------------------------------------------------------------------------------------- reconstruction
@pytest.mark.parametrize("D,N,K,aligned", RECON_CASES, ids=lambda v: str(v))
def test_recon_fwd_matches_float64(D, N, K, aligned):
    """mcq_recon_fwd: err = sum_n C[n][idx] - x entry by entry (c = 4, L = N + 1, S = sum_n |C| + |x|); each num_part and
    den_part against the fp64 sums over its four vectors (c = 4, L = tg.recon_chain: a lane's fmas, the butterfly, the
    waves; num_part also carries the error of err itself).  C is read back from the prepared blob: the scaled centers the
    kernel sums."""
    L = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(D * 131 + N * 7 + K)
    B = 257
    centers = torch.randn(N, K, D, device=dev, generator=gen).contiguous()
    blob = torch.empty(L.mcq_prepared_bytes(N, K, D), dtype=torch.uint8, device=dev)
    assert L.mcq_prepare(centers.data_ptr(), 0.75, None, None, N, K, D, blob.data_ptr(), _st()) == 0
    Dp = L.mcq_padded_dim(D)
    C = blob[:N * K * Dp * 4].view(torch.float32).reshape(N * K, Dp)[:, :D].double()
    buf = torch.randn(B * D + 4, device=dev, generator=gen) * 2 + 0.5
    x = buf[:B * D].view(B, D) if aligned else buf[1:1 + B * D].view(B, D)      # offset by one float: the scalar branch
    assert (x.data_ptr() % 16 == 0) == aligned or D % 4 != 0
    mean = torch.randn(D, device=dev, generator=gen)
    idx = torch.randint(0, K, (B, N), device=dev, generator=gen)
    G = (B + 3) // 4

    def run():
        err, num, den = torch.empty(B, D, device=dev), torch.empty(G, device=dev), torch.empty(G, device=dev)
        assert L.mcq_recon_fwd(x.data_ptr(), idx.data_ptr(), B, blob.data_ptr(), mean.data_ptr(), N, K, D, err.data_ptr(),
                               num.data_ptr(), den.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        return err, num, den

    a = run()
    _same(a, run(), "mcq_recon_fwd")
    err, num, den = a
    rows = (idx + torch.arange(N, device=dev) * K)
    picked = C[rows]                                  # (B, N, D)
    x64 = x.double()
    e = picked.sum(1) - x64
    be = 4 * (N + 1) * EPS * (picked.abs().sum(1) + x64.abs())
    _check("mcq_recon_fwd", "err", err, e, be)
    Lr = tg.recon_chain(D, aligned)
    pad = 4 * G - B

    def groups(t):
        return torch.cat([t, t.new_zeros(pad)]).reshape(G, 4).sum(1)

    e2 = groups((e * e).sum(1))
    _check("mcq_recon_fwd", "num_part", num, e2, 4 * Lr * EPS * e2 + groups((2 * e.abs() * be + be * be).sum(1)))
    c = x64 - mean.double()
    c2 = groups((c * c).sum(1))
    _check("mcq_recon_fwd", "den_part", den, c2, 4 * (Lr + 1) * EPS * c2)


# ---------------------------------------------------------------------------------------------- head and tail
def _tail_ref(num, den, chosen, Bt, ps, cnt, N, K, es):
    """fp64 loss_tail_body (compute_loss, quantization.py:211-242, on the batch sums), with magnitudes for the bounds"""
    ref = math.log(K)
    p = ps / Bt + 1e-20
    lp = p.log()
    gscale = es / (ref * N * Bt)
    gp = (lp + 1.0) * gscale
    c = cnt / Bt + 1e-20
    hl = -(p * lp).sum(1)
    hi = -(c * c.log()).sum(1)
    losses = torch.stack([num / (den + 1e-20), -chosen / (Bt * N), (ref - hl.sum() / N) / ref, (ref - hi.sum() / N) / ref])
    g = torch.stack([1.0 / (den + 1e-20), torch.tensor(-1.0 / (Bt * N), dtype=torch.float64, device=ps.device)])
    # |p log p| plus the error of log p itself (p = ps / Bt + 1e-20: two roundings; logf: 1 ulp)
    s_l = (p * lp).abs().sum(1) + p.sum(1) * 3
    s_i = (c * c.log()).abs().sum(1) + c.sum(1) * 3
    return losses, g, gp, lp, gscale, s_l, s_i, ref


@pytest.mark.parametrize("nparts,N,K", HT_CASES, ids=lambda v: str(v))
def test_loss_head_tail_match_float64(nparts, N, K):
    """mcq_loss_head: the three sums against fp64 (c = 4, L = strided terms per thread + 8 tree levels).  mcq_loss_tail on
    those sums: the four losses, g[0..1] and every g_prob entry against the fp64 formula of loss_tail_body (c = 4; L = 6 for
    g_prob and the scalar ratios, K / 64 + 6 + N + 4 for the entropies, which also carry the 1e-20 guard of zero entries).
    mcq_loss_head_tail equals mcq_loss_head followed by mcq_loss_tail bit for bit."""
    L = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(nparts + 17 * N + K)
    Bf, es = 4096.0, 0.37
    nump = torch.rand(nparts, device=dev, generator=gen) * 3
    denp = torch.rand(nparts, device=dev, generator=gen) * 5 + 0.1
    chosen = -torch.rand(N, device=dev, generator=gen) * 2000
    ps = torch.rand(N, K, device=dev, generator=gen) * (2 * Bf / K)
    ps[torch.rand(N, K, device=dev, generator=gen) < 0.2] = 0.0          # zero probability sums: the guard matters
    cnt = torch.randint(0, int(2 * Bf / K) + 1, (N, K), device=dev, generator=gen).float()
    cnt[torch.rand(N, K, device=dev, generator=gen) < 0.3] = 0.0

    def run():
        head, losses, g, gp = (torch.empty(4, device=dev), torch.empty(4, device=dev), torch.empty(2, device=dev),
                               torch.empty(N, K, device=dev))
        head2, losses2, g2, gp2 = (torch.empty(4, device=dev), torch.empty(4, device=dev), torch.empty(2, device=dev),
                                   torch.empty(N, K, device=dev))
        assert L.mcq_loss_head(nump.data_ptr(), denp.data_ptr(), nparts, chosen.data_ptr(), N, Bf, head.data_ptr(), _st()) == 0
        assert L.mcq_loss_tail(head.data_ptr(), ps.data_ptr(), cnt.data_ptr(), N, K, es, losses.data_ptr(), g.data_ptr(),
                               gp.data_ptr(), _st()) == 0
        assert L.mcq_loss_head_tail(nump.data_ptr(), denp.data_ptr(), nparts, chosen.data_ptr(), N, Bf, head2.data_ptr(),
                                    ps.data_ptr(), cnt.data_ptr(), K, es, losses2.data_ptr(), g2.data_ptr(), gp2.data_ptr(),
                                    _st()) == 0
        torch.cuda.synchronize()
        return head, losses, g, gp, head2, losses2, g2, gp2

    a = run()
    _same(a, run(), "mcq_loss_head / tail / head_tail")
    head, losses, g, gp, head2, losses2, g2, gp2 = a
    _same((head, losses, g, gp), (head2, losses2, g2, gp2), "mcq_loss_head_tail against mcq_loss_head + mcq_loss_tail")
    Lh = -(-nparts // 256) + 8
    sums = torch.stack([nump.double().sum(), denp.double().sum(), chosen.double().sum(), torch.tensor(Bf, device=dev).double()])
    Lc = -(-N // 256) + 8
    zero = torch.tensor(0.0, dtype=torch.float64, device=dev)
    bh = torch.stack([4 * Lh * EPS * nump.double().abs().sum(), 4 * Lh * EPS * denp.double().abs().sum(),
                      4 * Lc * EPS * chosen.double().abs().sum(), zero])
    _check("mcq_loss_head", "head", head, sums, bh)
    h = head.double()
    lr, gr, gpr, lp, gscale, s_l, s_i, ref = _tail_ref(h[0], h[1], h[2], Bf, ps.double(), cnt.double(), N, K, es)
    _check("mcq_loss_tail", "g_prob", gp, gpr, 4 * 6 * EPS * ((lp.abs() + 1) * abs(gscale) + 3 * abs(gscale)))
    Le = K // 64 + 6 + N + 4
    bl = torch.stack([4 * 6 * EPS * lr[0].abs(), 4 * 6 * EPS * lr[1].abs(),
                      (4 * Le * EPS * s_l.sum() / N + 4 * 6 * EPS * ref) / ref, (4 * Le * EPS * s_i.sum() / N + 4 * 6 * EPS * ref) / ref])
    _check("mcq_loss_tail", "losses", losses, lr, bl)
    _check("mcq_loss_tail", "g", g, gr, 4 * 6 * EPS * gr.abs())


# ---------------------------------------------------------------------------------------------- centers' gradient
@pytest.mark.parametrize("D,K,B,N", DB_CASES, ids=lambda v: str(v))
def test_decode_backward_u8_ex_matches_float64(D, K, B, N):
    """mcq_decode_backward_u8_ex: gC entry by entry against the fp64 scatter of the gradient rows times sa * sb * sc (c = 4,
    L = hits of the row + 3), and each wave's dot_part against fp64 <unscaled sums, dotw> over its feature chunk (c = 4,
    L = CW + 6, plus the error of the sums themselves)."""
    L = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(D + 3 * K + B + N)
    g = torch.randn(max(B, 1), D, device=dev, generator=gen)
    codes = torch.randint(0, K, (max(B, 1), N), device=dev, generator=gen).to(torch.uint8)
    sa, sb, sc = torch.tensor([1.7], device=dev), torch.tensor([0.3], device=dev), 2.0
    dotw = torch.randn(N, K, D, device=dev, generator=gen)
    waves = L.mcq_decode_backward_waves(N, K, D)
    cw = tg.db_cw_of(D, K)
    chunks = tg.db_chunks(D, cw)
    assert waves == N * K * chunks

    def run():
        gC, dp = torch.empty(N, K, D, device=dev), torch.empty(waves, device=dev)
        assert L.mcq_decode_backward_u8_ex(g.data_ptr(), codes.data_ptr(), B, N, K, D, gC.data_ptr(), sa.data_ptr(),
                                           sb.data_ptr(), sc, dotw.data_ptr(), dp.data_ptr(), _st()) == 0
        torch.cuda.synchronize()
        return gC, dp

    a = run()
    _same(a, run(), "mcq_decode_backward_u8_ex")
    gC, dp = a
    f = float(sa.double()) * float(sb.double()) * sc
    rows = (codes[:B].long() + torch.arange(N, device=dev) * K).reshape(-1)
    gb = g[:B].double().unsqueeze(1).expand(B, N, D).reshape(-1, D)
    S = torch.zeros(N * K, D, dtype=torch.float64, device=dev).index_add_(0, rows, gb)
    Sa = torch.zeros(N * K, D, dtype=torch.float64, device=dev).index_add_(0, rows, gb.abs())
    hits = torch.zeros(N * K, dtype=torch.float64, device=dev).index_add_(0, rows, torch.ones_like(rows, dtype=torch.float64))
    bS = 4 * (hits.unsqueeze(1) + 1) * EPS * Sa
    _check("mcq_decode_backward_u8_ex", "gC", gC.reshape(N * K, D), S * f, bS * abs(f) + 4 * 3 * EPS * (S * f).abs())
    w64 = dotw.double().reshape(N * K, D)
    width = chunks * 64 * cw

    def per_wave(t):
        return torch.cat([t, t.new_zeros(N * K, width - D)], 1).reshape(N * K, chunks, 64 * cw).sum(-1).reshape(-1)

    _check("mcq_decode_backward_u8_ex", "dot_part", dp, per_wave(S * w64),
           4 * (cw + 6) * EPS * per_wave((S * w64).abs()) + per_wave(bS * w64.abs()))


# ---------------------------------------------------------------------------------------------- scalar gradients
GT_CASES = [(n, m, sa, sb, oc, ol) for n, m, sa, sb, oc, ol in [
    (0, 100000, True, True, True, True), (1, 8193, True, False, True, True), (1023, 8192, False, True, True, True),
    (1024, 1024, False, False, True, True), (8192, 1023, True, True, False, True), (8193, 1, True, True, True, False),
    (100000, 0, True, True, True, True), (100000, 100000, False, False, True, True)]]


@pytest.mark.parametrize("n_c,n_l,use_sa,use_sb,out_c,out_l", GT_CASES, ids=lambda v: str(v))
def test_grad_tail_matches_float64(n_c, n_l, use_sa, use_sb, out_c, out_l):
    """mcq_grad_tail: (sum part_c) * sa * sb * sc * speed and (sum part_l) * speed against fp64 sums times the factors
    (c = 4, L = strided terms per thread + 10 tree levels + 4 factor roundings)."""
    L = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(n_c + 3 * n_l)
    pc = torch.randn(max(n_c, 1), device=dev, generator=gen)
    pl = torch.randn(max(n_l, 1), device=dev, generator=gen) + 0.25
    sa, sb, sc, speed = torch.tensor([1.3], device=dev), torch.tensor([-0.7], device=dev), 2.0, 10.0

    def run():
        oc, ol = torch.full((1,), 12345.0, device=dev), torch.full((1,), 12345.0, device=dev)
        assert L.mcq_grad_tail(pc.data_ptr() if n_c else None, n_c, sa.data_ptr() if use_sa else None,
                               sb.data_ptr() if use_sb else None, sc, pl.data_ptr() if n_l else None, n_l, speed,
                               oc.data_ptr() if out_c else None, ol.data_ptr() if out_l else None, _st()) == 0
        torch.cuda.synchronize()
        return oc, ol

    a = run()
    _same(a, run(), "mcq_grad_tail")
    oc, ol = a
    fc = (float(sa) if use_sa else 1.0) * (float(sb) if use_sb else 1.0) * sc * speed
    for on, n, part, fac, got, what in ((out_c, n_c, pc, fc, oc, "out_c"), (out_l, n_l, pl, speed, ol, "out_l")):
        if not on:
            assert float(got) == 12345.0, f"{what} was written through a null pointer's place"
            continue
        p64 = part[:n].double()
        Lg = -(-n // 1024) + 10 + 4
        ref = p64.sum() * fac
        _check("mcq_grad_tail", what, got, ref.reshape(1), (4 * Lg * EPS * p64.abs().sum() * abs(fac)).reshape(1))


# ---------------------------------------------------------------------------------------------- weight gradient
@pytest.mark.parametrize("B,M,D", WGRAD_CASES, ids=lambda v: str(v))
def test_weight_grad_matches_float64(B, M, D):
    """mcq_weight_grad: gW entry by entry against fp64 s G^T x (S = s |G|^T |x|) and gb against sum_b G (S = sum |G|); c = 4,
    L = tg.wgrad_chain (rows of the longest split, times six piece products on the bf16-piece kernel, plus the splits).
    G is shaped like softmax gradients whose columns range from 1 down to 2^-100 (every bf16 piece stays normal); x carries a
    common offset of 100."""
    L = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(B + 7 * M + 13 * D)
    colscale = torch.pow(2.0, -100.0 * torch.arange(M, device=dev) / max(M - 1, 1))
    G = (torch.randn(B, M, device=dev, generator=gen) * colscale).contiguous()
    x = (torch.randn(B, D, device=dev, generator=gen) + 100.0).contiguous()
    s = torch.tensor([0.8], device=dev)
    ws = torch.empty(L.mcq_weight_grad_workspace_bytes(B, M, D), dtype=torch.uint8, device=dev)

    def run():
        gW, gb = torch.empty(M, D, device=dev), torch.empty(M, device=dev)
        assert L.mcq_weight_grad(G.data_ptr(), x.data_ptr(), B, M, D, s.data_ptr(), gW.data_ptr(), gb.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _st()) == 0
        torch.cuda.synchronize()
        return gW, gb

    a = run()
    _same(a, run(), "mcq_weight_grad")
    gW, gb = a
    G64, x64, sv = G.double(), x.double(), float(s.double())
    Lw = tg.wgrad_chain(B, M, D)
    entry = "mcq_weight_grad" + ("[bf3]" if tg.wgrad_use_bf3(B, M, D) else "[f32]")
    _check(entry, "gW", gW, sv * (G64.t() @ x64), 4 * (Lw + 1) * EPS * sv * (G64.abs().t() @ x64.abs()))
    _check(entry, "gb", gb, G64.sum(0), 4 * Lw * EPS * G64.abs().sum(0))


# ---------------------------------------------------------------------------------------------- Adam
@pytest.mark.parametrize("n", ADAM_SIZES)
def test_adam_step_matches_float64(n):
    """mcq_adam_step, six steps with changing learning rates and weight decay, each against a float64 restatement of the
    update in the comment on k_adam applied to the kernel's state before the step: p, m and v within c = 4 roundings of
    the magnitudes they are formed from (for p: max(|p|, step), plus what the errors of m and v do to the step).  At the
    large sizes the result after the six steps is also compared with torch.optim.Adam."""
    L = _lib()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device="cuda:0").manual_seed(n)
    p = torch.randn(n, device=dev, generator=gen) * 0.05
    m, v = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    p0 = p.clone()
    beta1, beta2, eps = 0.9, 0.98, 1e-8
    sched = [(2e-3, 0.0), (1e-3, 1e-2), (5e-4, 0.0), (3e-3, 1e-3), (1e-3, 0.0), (2e-4, 0.5)]
    grads = [torch.randn(n, device=dev, generator=gen) * (0.1 / (t + 1)) for t in range(len(sched))]
    for t, (lr, wd) in enumerate(sched, start=1):
        bc1, bc2s = 1 - beta1 ** t, math.sqrt(1 - beta2 ** t)
        g = grads[t - 1]
        P, Mo, V = p.double(), m.double(), v.double()
        outs = []
        for _ in range(2):
            pp, mm, vv = p.clone(), m.clone(), v.clone()
            assert L.mcq_adam_step(pp.data_ptr(), g.data_ptr(), mm.data_ptr(), vv.data_ptr(), n, lr, beta1, beta2, eps, wd,
                                   bc1, bc2s, _st()) == 0
            torch.cuda.synchronize()
            outs.append((pp, mm, vv))
        _same(outs[0], outs[1], "mcq_adam_step")
        pn, mn, vn = outs[0]
        g64 = g.double()
        gg = g64 + wd * P
        sg = g64.abs() + wd * P.abs()
        Mr = Mo + (1 - beta1) * (gg - Mo)
        Vr = beta2 * V + (1 - beta2) * gg * gg
        bm = 4 * 3 * EPS * (Mo.abs() + (1 - beta1) * (sg + Mo.abs()))
        bv = 4 * 3 * EPS * (beta2 * V + (1 - beta2) * sg * sg)
        den = Vr.sqrt() / bc2s + eps
        step = (lr / bc1) * Mr / den
        Pr = P - step
        dden = bv / (2 * Vr.sqrt().clamp_min(1e-300) * bc2s) + 4 * 3 * EPS * Vr.sqrt() / bc2s
        bstep = (lr / bc1) * bm / den + step.abs() * (dden / den + 4 * 4 * EPS)
        _check("mcq_adam_step", "m", mn, Mr, bm)
        _check("mcq_adam_step", "v", vn, Vr, bv)
        _check("mcq_adam_step", "p", pn, Pr, 4 * EPS * torch.maximum(P.abs(), step.abs()) + bstep)
        p, m, v = pn, mn, vn
    if n >= 2097152:
        ref = torch.nn.Parameter(p0.clone())
        opt = torch.optim.Adam([ref], lr=1.0, betas=(beta1, beta2), eps=eps)
        for t, (lr, wd) in enumerate(sched, start=1):
            for grp in opt.param_groups:
                grp["lr"], grp["weight_decay"] = lr, wd
            ref.grad = grads[t - 1].clone()
            opt.step()
        assert float((p - ref.detach()).abs().max()) <= 3e-8, float((p - ref.detach()).abs().max())


# ---------------------------------------------------------------------------------------------- scale factors
@pytest.mark.parametrize("cs,ls", [(-0.0625, 0.03125), (0.1875, -0.5), (0.0, 0.25)])
def test_scales_exp_and_prepare_params_agree(cs, ls):
    """mcq_scales_exp's out2 and mcq_prepare_params' scales_exp_out are the same bits, each within 1 ulp of fp64
    exp(speed * scale) (speed * scale is exact in fp32 here); a blob from mcq_prepare_params and one from mcq_prepare_dev on
    those factors give bit-identical mcq_decode and mcq_logits."""
    L = _lib()
    dev = torch.device("cuda:0")
    N, K, D, B, speed = 4, 256, 72, 300, 10.0
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    csd, lsd = torch.tensor([cs], device=dev), torch.tensor([ls], device=dev)
    centers = torch.randn(N, K, D, device=dev, generator=gen)
    W = torch.randn(N * K, D, device=dev, generator=gen) * 0.1
    b = torch.randn(N * K, device=dev, generator=gen) * 0.1
    out2, so = torch.empty(2, device=dev), torch.empty(2, device=dev)
    blob1 = torch.zeros(L.mcq_prepared_bytes(N, K, D), dtype=torch.uint8, device=dev)
    blob2 = torch.zeros_like(blob1)
    assert L.mcq_scales_exp(csd.data_ptr(), lsd.data_ptr(), speed, out2.data_ptr(), _st()) == 0
    assert L.mcq_prepare_params(centers.data_ptr(), csd.data_ptr(), lsd.data_ptr(), speed, W.data_ptr(), b.data_ptr(), N, K, D,
                                blob1.data_ptr(), so.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out2, so)
    for got, sc in zip(out2.tolist(), (cs, ls)):
        ref = math.exp(speed * sc)
        ulp = 2.0 ** (math.frexp(ref)[1] - 24)      # one fp32 ulp at ref
        assert abs(got - ref) <= ulp, (sc, got, ref)
        RATIOS["mcq_scales_exp"] = max(RATIOS.get("mcq_scales_exp", 0.0), abs(got - ref) / ulp)
    assert L.mcq_prepare_dev(centers.data_ptr(), so.data_ptr(), W.data_ptr(), b.data_ptr(), N, K, D, blob2.data_ptr(), _st()) == 0
    codes = torch.randint(0, K, (B, N), device=dev, generator=gen).to(torch.uint8)
    x = torch.randn(B, D, device=dev, generator=gen)
    ws = torch.empty(L.mcq_logits_workspace_bytes(B, N, D), dtype=torch.uint8, device=dev)
    res = []
    for blob in (blob1, blob2):
        y, z = torch.empty(B, D, device=dev), torch.empty(B, N * K, device=dev)
        assert L.mcq_decode(codes.data_ptr(), 1, N, B, blob.data_ptr(), N, K, D, y.data_ptr(), _st()) == 0
        assert L.mcq_logits(x.data_ptr(), B, blob.data_ptr(), float(out2[1]), N, K, D, z.data_ptr(), ws.data_ptr(), ws.numel(),
                            _st()) == 0
        torch.cuda.synchronize()
        res.append((y, z))
    _same(res[0], res[1], "blobs of mcq_prepare_params and mcq_prepare_dev")


# ---------------------------------------------------------------------------------------------- composed, in float64
COMPOSED = [(30, 16, 4, 333, False, 0), (130, 256, 2, 257, False, 2), (768, 256, 8, 1024, False, 0), (64, 256, 1, 500, False, 2),
            (48, 16, 64, 300, False, 0), (96, 64, 4, 400, True, 2)]


@pytest.mark.parametrize("D,K,N,B,fp16,iters", COMPOSED, ids=lambda v: str(v))
def test_fused_loss_and_backward_match_float64_autograd(D, K, N, B, fp16, iters):
    """Quantizer.compute_loss on the fused kernels and its backward (what QuantizerTrainer.step runs) against float64
    autograd of the reference formula (quantization.py:211-242) evaluated on the same indexes the kernels chose (the argmax
    is discrete and pinned elsewhere).  Losses within 1e-5 relative (of max(1, |loss|)); each parameter gradient within 1e-5
    of that tensor's largest entry, the two scalar gradients within 1e-5 relative."""
    from quantization_amd import Quantizer
    from quantization_amd.quantizer import _loss_forward_kernels
    torch.manual_seed(31 + D + N)
    dev = torch.device("cuda:0")
    q = Quantizer(D, K, N).to(dev)
    with torch.no_grad():
        q.to_logits.bias.normal_(std=0.1)
        q.centers.mul_(3.0)
        q.logits_scale.fill_(0.03)
        q.centers_scale.fill_(-0.02)
    x = torch.randn(B, D, device=dev)
    if fp16:
        x = x.half()
    w = (1.0, 1.0, 0.01)
    q.zero_grad()
    lf = q.compute_loss(x, iters)
    (lf[0] * w[0] + lf[1] * w[1] + lf[2] * w[2]).backward()
    gf = {n: p.grad.detach().clone() for n, p in q.named_parameters()}
    blob = q._prepared()
    idx = _loss_forward_kernels(q, x, iters, blob, q._lscale_exp, q._scale_flags).idx
    # fp64 autograd on the same indexes
    P = {n: p.detach().double().clone().requires_grad_(True) for n, p in q.named_parameters()}
    x64 = x.double()
    C = (P["centers_scale"] * q.scale_speed).exp() * P["centers"]
    xa = C[torch.arange(N, device=dev).unsqueeze(0), idx].sum(1)
    num = ((xa - x64) ** 2).sum()
    den = ((x64 - C.detach().mean(dim=1).sum(dim=0)) ** 2).sum()
    logits = ((P["logits_scale"] * q.scale_speed).exp() * x64) @ P["to_logits.weight"].t() + P["to_logits.bias"]
    lp = logits.reshape(B, N, K).log_softmax(dim=2)
    chosen = lp.gather(2, idx.unsqueeze(2)).sum()
    counts = torch.zeros(B, N, K, dtype=torch.float64, device=dev).scatter_(2, idx.unsqueeze(2), 1.0)
    avg = counts.mean(0) + 1e-20
    probs = lp.exp().mean(0) + 1e-20
    ref_h = math.log(K)
    lr = [num / (den + 1e-20), -chosen / (B * N), (ref_h + (probs * probs.log()).sum(1).mean()) / ref_h,
          (ref_h + (avg * avg.log()).sum(1).mean()) / ref_h]
    (lr[0] * w[0] + lr[1] * w[1] + lr[2] * w[2]).backward()
    for a, b, name in zip(lf, lr, ["recon", "logprob", "logits_entropy", "index_entropy"]):
        a, b = float(a.detach()), float(b.detach())
        err, tol = abs(a - b), 1e-5 * max(1.0, abs(b))
        assert err <= tol, (name, a, b)
        RATIOS["compute_loss:losses"] = max(RATIOS.get("compute_loss:losses", 0.0), err / tol)
    for n, p in P.items():
        ref = p.grad
        tol = 1e-5 * (abs(float(ref)) if ref.dim() == 0 else float(ref.abs().max()))
        err = float((gf[n].double() - ref).abs().max())
        assert err <= tol, (n, err, tol)
        key = "compute_loss:" + ("scalars" if ref.dim() == 0 else n)
        RATIOS[key] = max(RATIOS.get(key, 0.0), err / tol)
