"""JointCodebookLoss (reference: quantization/prediction.py): drop-in surface on CPU, values and gradients against
fixtures captured from the reference (tests/golden/make_golden_jcl.py) on the GPU."""
import glob
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "jcl_*.npz")))


def _module(fx, checkpoint):
    from quantization_amd import JointCodebookLoss
    m = JointCodebookLoss(predictor_channels=int(fx["pc"]), num_codebooks=int(fx["ncb"]), hidden_channels=int(fx["hidden"]),
                          codebook_size=int(fx["K"]), reduction=str(fx["reduction"]), checkpoint=checkpoint)
    sd = {k[len("state."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("state.")}
    assert set(sd) == set(m.state_dict()) and all(tuple(sd[k].shape) == tuple(v.shape) for k, v in m.state_dict().items())
    m.load_state_dict(sd)       # a reference checkpoint loads unchanged
    return m


def test_surface_and_no_cpu_fallback():
    assert len(FIXTURES) == 4
    from quantization_amd import _lib
    fx = np.load(FIXTURES[0])
    m = _module(fx, True)
    with pytest.raises(_lib.McqError):
        m(torch.from_numpy(fx["predictor"]), torch.from_numpy(fx["indexes"]))


@pytest.mark.gpu
@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
@pytest.mark.parametrize("checkpoint", [True, False])
def test_loss_and_gradients_match_the_reference(path, checkpoint):
    fx = np.load(path)
    m = _module(fx, checkpoint).cuda()
    pred = torch.from_numpy(fx["predictor"]).cuda().requires_grad_(True)
    idx = torch.from_numpy(fx["indexes"]).cuda()
    loss = m(pred, idx)
    loss.backward()
    assert abs(float(loss.detach()) - float(fx["loss"])) <= 1e-5 * abs(float(fx["loss"])), (float(loss.detach()), float(fx["loss"]))
    got = {"grad_predictor": pred.grad}
    got.update({"grad." + k: p.grad for k, p in m.named_parameters()})
    for k, g in got.items():
        ref = fx[k]
        scale = max(np.abs(ref).max(), 1e-6)
        err = np.abs(g.cpu().numpy() - ref).max()
        assert err <= 1e-4 * scale, (k, err, scale)
    # bit-reproducible (fixed-order scatter and reductions)
    m.zero_grad()
    pred2 = pred.detach().clone().requires_grad_(True)
    loss2 = m(pred2, idx)
    loss2.backward()
    assert torch.equal(loss2.detach(), loss.detach()) and torch.equal(pred2.grad, pred.grad)


@pytest.mark.gpu
def test_uint8_codes_from_encode_feed_the_loss():
    """the step after encode in the reference's integration script (test_train_hdf5.py:120-121)"""
    from quantization_amd import JointCodebookLoss, Quantizer
    torch.manual_seed(0)
    q = Quantizer(64, 256, 4).cuda()
    x = torch.randn(300, 64, device="cuda")
    with torch.no_grad():
        codes = q.encode(x)                       # uint8 (300, 4)
    m = JointCodebookLoss(predictor_channels=64, num_codebooks=4, hidden_channels=128).cuda()
    loss = m(x, codes)
    loss.backward()
    assert torch.isfinite(loss) and float(loss.detach()) > 0 and all(p.grad is not None for p in m.parameters())


@pytest.mark.gpu
@pytest.mark.parametrize("B,P,N,H,K", [(1, 8, 2, 16, 16), (3, 20, 3, 70, 32), (130, 33, 5, 96, 128)])
def test_ragged_sizes_against_the_torch_op_sequence(B, P, N, H, K):
    """sizes the fixtures do not hold (single frame, odd channel counts, codebook counts that are not powers of two)
    against the reference's op sequence (prediction.py:38-81) written with torch ops on the same device"""
    import torch.nn.functional as F
    from quantization_amd import JointCodebookLoss
    torch.manual_seed(B)
    m = JointCodebookLoss(P, N, H, K, reduction="mean", checkpoint=False).cuda()
    pred = torch.randn(B, P, device="cuda", requires_grad=True)
    idx = torch.randint(0, K, (B, N), device="cuda")
    if B > 2:
        idx[1] = -100

    def ref():
        first = idx[:, :-1].clamp(min=0) + torch.arange(0, (N - 1) * K, step=K, device=idx.device)
        emb = F.embedding(first, m.codebook_embedding.weight) * (0.5 * ((H / N) ** 0.5))
        a = torch.relu(torch.cumsum(torch.cat((m.linear1(pred).unsqueeze(1), emb), dim=1), dim=1))
        lp = torch.matmul(a.transpose(0, 1), m.linear2_weight.transpose(1, 2)).transpose(0, 1)
        lp = lp + torch.matmul(pred, m.linear2b_weight.transpose(1, 2)).transpose(0, 1) + m.linear2_bias
        return F.cross_entropy(lp.reshape(-1, K), idx.reshape(-1), ignore_index=-100, reduction="mean")

    grads = []
    for fn in (lambda: m(pred, idx), ref):
        m.zero_grad()
        pred.grad = None
        loss = fn()
        loss.backward()
        grads.append((loss.detach(), pred.grad.clone(), {k: p.grad.clone() for k, p in m.named_parameters()}))
    (la, ga, pa), (lb, gb, pb) = grads
    assert abs(float(la) - float(lb)) <= 1e-5 * abs(float(lb))
    assert float((ga - gb).abs().max()) <= 1e-4 * float(gb.abs().max() + 1e-9)
    for k in pa:
        assert float((pa[k] - pb[k]).abs().max()) <= 1e-4 * float(pb[k].abs().max() + 1e-9), k


def _torch_rows(m, pred, idx, keep_hp=None):
    """the reference's op sequence (prediction.py:38-82) with reduction='none', in torch; hp = linear1(predictor) is
    appended to the list keep_hp, with its gradient retained, when one is given"""
    import torch.nn.functional as F
    N, K, H = m.num_codebooks, m.codebook_size, m.hidden_channels
    p2 = pred.reshape(-1, pred.shape[-1])
    i2 = idx.reshape(-1, N).to(torch.int64)
    first = i2[:, :-1].clamp(min=0) + torch.arange(0, (N - 1) * K, K, device=i2.device)
    emb = F.embedding(first, m.codebook_embedding.weight) * (0.5 * ((H / N) ** 0.5))
    hp = F.linear(p2, m.linear1.weight, m.linear1.bias)
    if keep_hp is not None:
        hp.retain_grad()
        keep_hp.append(hp)
    a = torch.relu(torch.cumsum(torch.cat((hp.unsqueeze(1), emb), dim=1), dim=1))
    z = torch.matmul(a.transpose(0, 1), m.linear2_weight.transpose(1, 2)).transpose(0, 1)
    z = z + torch.matmul(p2, m.linear2b_weight.transpose(1, 2)).transpose(0, 1) + m.linear2_bias
    return F.cross_entropy(z.reshape(-1, K), i2.reshape(-1), ignore_index=-100, reduction="none")


# ---------------------------------------------------------------------------------------------- padding, per element
PAD_SIZES = [(12, 20, 4, 24, 16), (130, 33, 5, 96, 128)]            # (B, P, N, H, K)
PAD_PATTERNS = ["single", "last_column", "whole_frames", "column0"]


def _padded_indexes(pattern, B, N, K, gen):
    """targets in [1, K): entry 0 of a codebook is then gathered, and its embedding row trained, only through the clamp
    of a negative target (prediction.py:44-50)"""
    idx = torch.randint(1, K, (B, N), generator=gen)
    if pattern == "single":            # (a) one negative per chosen frame, in a codebook j < N-1 whose later codebooks are valid
        for i, b in enumerate(range(1, B, 3)):
            idx[b, i % (N - 1)] = -100
    elif pattern == "last_column":     # (b) the last codebook is no input to any other
        idx[::3, N - 1] = -100
    elif pattern == "whole_frames":    # (c) what the fixtures of the first three files hold
        idx[::4] = -100
    elif pattern == "column0":         # (d) embedding row 0 receives a contribution from every frame
        idx[:, 0] = -100
    elif pattern == "all":             # (e)
        idx[:] = -100
    else:
        raise ValueError(pattern)
    return idx


_PAD_REFERENCES = {}


def _padded_reference(size, pattern, reduction):
    """inputs, fp32 state and the float64 CPU result of the reference's op sequence (_torch_rows); computed once per
    (size, pattern, reduction), shared by both checkpoint settings and never modified"""
    key = (size, pattern, reduction)
    if key not in _PAD_REFERENCES:
        from quantization_amd import JointCodebookLoss
        B, P, N, H, K = size
        gen = torch.Generator().manual_seed(B + 10 * PAD_SIZES.index(size) + 100 * (PAD_PATTERNS + ["all"]).index(pattern))
        torch.manual_seed(7 + B)
        m = JointCodebookLoss(P, N, H, K)
        with torch.no_grad():
            m.linear2_bias.normal_(std=0.1, generator=gen)
        state = {k: v.clone() for k, v in m.state_dict().items()}
        pred = torch.randn(B, P, generator=gen)
        idx = _padded_indexes(pattern, B, N, K, gen)
        w = torch.rand(B * N, generator=gen) + 0.5              # upstream weights of the rows of reduction='none'
        m64 = m.double()
        p64 = pred.double().requires_grad_(True)
        rows = _torch_rows(m64, p64, idx)
        valid = int((idx >= 0).sum())
        out = rows if reduction == "none" else (rows.sum() if reduction == "sum" else rows.sum() / valid)
        (rows * w.double()).sum().backward() if reduction == "none" else out.backward()
        grads = {"grad_predictor": p64.grad.clone()}
        grads.update({"grad." + k: p.grad.clone() for k, p in m64.named_parameters()})
        _PAD_REFERENCES[key] = (state, pred, idx, w, out.detach().clone(), grads)
    return _PAD_REFERENCES[key]


def _padded_device(size, state, pred, idx, w, reduction, checkpoint):
    from quantization_amd import JointCodebookLoss
    B, P, N, H, K = size
    m = JointCodebookLoss(P, N, H, K, reduction=reduction, checkpoint=checkpoint)
    m.load_state_dict(state)
    m = m.cuda()
    p = pred.cuda().requires_grad_(True)
    out = m(p, idx.cuda())
    ((out * w.cuda()).sum() if reduction == "none" else out).backward()
    grads = {"grad_predictor": p.grad}
    grads.update({"grad." + k: q.grad for k, q in m.named_parameters()})
    return out.detach().cpu().double(), {k: g.cpu().double() for k, g in grads.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("checkpoint", [True, False])
@pytest.mark.parametrize("reduction", ["sum", "mean", "none"])
@pytest.mark.parametrize("pattern", PAD_PATTERNS)
@pytest.mark.parametrize("size", PAD_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_padding_is_per_element_as_in_the_reference(size, pattern, reduction, checkpoint):
    """JointCodebookLoss on the device against the reference's op sequence in float64 on the CPU, with negative targets
    (a) alone in a codebook before the last, (b) in the last codebook only, (c) in whole frames, (d) in all of codebook
    0.  Loss (each row of reduction='none') and every gradient within 1e-4 of the reference tensor's largest entry; and
    every embedding row n*K (reached only through a clamped negative: no target is 0) that the reference trains is trained
    on the device, to the same tolerance."""
    B, P, N, H, K = size
    state, pred, idx, w, ref_out, ref = _padded_reference(size, pattern, reduction)
    out, got = _padded_device(size, state, pred, idx, w, reduction, checkpoint)
    assert out.shape == ref_out.shape
    err, scale = float((out - ref_out).abs().max()), max(float(ref_out.abs().max()), 1e-6)
    print(f"loss: err {err:.3e} of {scale:.3e}")
    assert err <= 1e-4 * scale, ("loss", err, scale)
    for k, g in got.items():
        scale = max(float(ref[k].abs().max()), 1e-6)
        err = float((g - ref[k]).abs().max())
        print(f"{k}: err {err:.3e} of {scale:.3e}")
        assert torch.isfinite(g).all() and err <= 1e-4 * scale, (k, err, scale)
    ge, re_ = got["grad.codebook_embedding.weight"], ref["grad.codebook_embedding.weight"]
    scale = max(float(re_.abs().max()), 1e-6)
    trained = [n for n in range(N - 1) if float(re_[n * K].abs().max()) > 0]
    assert bool(trained) == (pattern in ("single", "column0")), (pattern, trained)
    for n in trained:
        err = float((ge[n * K] - re_[n * K]).abs().max())
        print(f"embedding row {n}*K: norm {float(ge[n * K].norm()):.4f}, reference {float(re_[n * K].norm()):.4f}, err {err:.3e}")
        assert float(ge[n * K].abs().max()) > 0 and err <= 1e-4 * scale, (n, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("checkpoint", [True, False])
@pytest.mark.parametrize("size", PAD_SIZES, ids=lambda v: "x".join(map(str, v)))
def test_every_target_negative_gives_zero_loss_and_zero_gradients(size, checkpoint):
    """(e) reduction='sum' over no valid target: the loss is 0 and every gradient exactly 0, nothing is NaN"""
    state, pred, idx, w, ref_out, ref = _padded_reference(size, "all", "sum")
    assert float(ref_out) == 0.0 and all(float(g.abs().max()) == 0.0 for g in ref.values())
    out, got = _padded_device(size, state, pred, idx, w, "sum", checkpoint)
    assert float(out) == 0.0
    for k, g in got.items():
        assert torch.isfinite(g).all() and float(g.abs().max()) == 0.0, k


@pytest.mark.gpu
def test_reduction_none_and_autocast():
    """reduction='none' gives the per-(frame, codebook) losses in the reference's order with the right gradient; under
    torch.autocast the fp32 kernels still see fp32 tensors (same loss and gradients as without it)."""
    fx = np.load(FIXTURES[0])
    m = _module(fx, False).cuda()
    pred = torch.from_numpy(fx["predictor"]).cuda()
    idx = torch.from_numpy(fx["indexes"]).cuda()
    m.reduction = "none"
    p1 = pred.clone().requires_grad_(True)
    rows = m(p1, idx)
    ref_rows = _torch_rows(m, pred, idx)
    assert rows.shape == ref_rows.shape
    assert torch.allclose(rows, ref_rows, rtol=1e-4, atol=1e-4)
    w = torch.rand_like(rows)
    (rows * w).sum().backward()
    g1 = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad()
    p2 = pred.clone().requires_grad_(True)
    (_torch_rows(m, p2, idx) * w).sum().backward()
    assert torch.allclose(p1.grad, p2.grad, rtol=1e-3, atol=1e-4 * float(p2.grad.abs().max()))
    for k, p in m.named_parameters():
        assert torch.allclose(g1[k], p.grad, rtol=1e-3, atol=2e-4 * float(p.grad.abs().max())), k
    # autocast
    m.reduction = "sum"
    m.zero_grad()
    p3 = pred.clone().requires_grad_(True)
    plain = m(p3, idx)
    plain.backward()
    gp = {k: p.grad.clone() for k, p in m.named_parameters()}
    m.zero_grad()
    p4 = pred.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        ac = m(p4, idx)
    ac.backward()
    assert ac.dtype == torch.float32 and torch.equal(ac.detach(), plain.detach()) and torch.equal(p3.grad, p4.grad)
    assert all(torch.equal(gp[k], p.grad) for k, p in m.named_parameters())
    # the quantizer's own loss under autocast
    from quantization_amd import Quantizer
    torch.manual_seed(0)
    q = Quantizer(64, 256, 4).cuda()
    x = torch.randn(300, 64, device="cuda")
    la = q.compute_loss(x, 1)
    sum(la[:3]).backward()
    ga = {k: p.grad.clone() for k, p in q.named_parameters()}
    q.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        lb = q.compute_loss(x, 1)
        tot = sum(lb[:3])
    tot.backward()
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(la, lb))
    assert all(torch.equal(ga[k], p.grad) for k, p in q.named_parameters())


@pytest.mark.gpu
def test_downstream_scenario_follows_the_reference():
    """The reference's downstream scenario (test_train_hdf5.py:79-134) at a size the CPU reference trains in seconds: a Quantizer
    TRAINED BY THE REFERENCE encodes seeded frames on the MI355X, a JointCodebookLoss learns to predict the codes from the frames
    (Adam, lr 1e-3, StepLR as in that script).  tests/golden/make_golden_downstream.py ran the same 300 steps with the reference
    on CPU from the same initial predictor: the loss curves must coincide -- step 0 (identical parameters, the codes of 512
    frames) to 1e-5, every step to 1 %, the last 20 steps' mean to 0.3 %."""
    from quantization_amd import JointCodebookLoss, Quantizer
    from golden import gen
    fx = np.load(os.path.join(HERE, "golden", "downstream_d64_b4.npz"))
    D, NB, B, steps = int(fx["D"]), int(fx["bytes"]), int(fx["B"]), int(fx["steps"])
    dev = torch.device("cuda:0")
    q = Quantizer(D, 256, NB)
    q.load_state_dict({k[len("quantizer."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("quantizer.")})
    q = q.to(dev)
    predictor = JointCodebookLoss(predictor_channels=D, num_codebooks=NB)
    predictor.load_state_dict({k[len("predictor_init."):]: torch.from_numpy(fx[k]) for k in fx.files if k.startswith("predictor_init.")})
    predictor = predictor.to(dev)
    optim = torch.optim.Adam(predictor.parameters(), lr=0.001, betas=(0.9, 0.98), eps=1e-9, weight_decay=1.0e-06)
    scheduler = torch.optim.lr_scheduler.StepLR(optim, step_size=2000, gamma=0.5)
    losses = []
    for s in range(steps):
        x = torch.from_numpy(gen.make_x(int(fx["data_seed"]) + s, B, D)).to(dev)
        with torch.no_grad():
            encoding = q.encode(x)
        assert encoding.dtype == torch.uint8 and tuple(encoding.shape) == (B, NB)
        loss = predictor(x, encoding) / x.shape[0]
        losses.append(float(loss.detach()))
        loss.backward()
        optim.step()
        optim.zero_grad()
        scheduler.step()
    losses, ref = np.array(losses), fx["losses"]
    rel = np.abs(losses - ref) / ref
    print("downstream scenario: first %.4f (reference %.4f), last-20 mean %.4f (%.4f), largest relative deviation %.2e"
          % (losses[0], ref[0], losses[-20:].mean(), ref[-20:].mean(), rel.max()))
    assert rel[0] <= 1e-5 and rel.max() <= 1e-2, (rel[0], rel.max())
    assert abs(losses[-20:].mean() - ref[-20:].mean()) <= 3e-3 * ref[-20:].mean()
    assert losses[-20:].mean() < 0.45 * losses[0]                   # it learned to predict the codes
