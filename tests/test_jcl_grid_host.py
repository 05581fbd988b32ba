"""Host-side checks of tests/jcl_grid.py (no GPU): what its restatements of the JointCodebookLoss kernels mean (composed in
float64 they are torch autograd of the reference's op sequence, padding per element included), that the fp32 restatements
stay within the float64 bounds, and that every case of tests/test_gpu_jcl_kernels.py holds the inputs and reaches the
launch path it claims."""
import numpy as np
import pytest
import torch

import jcl_grid as jg
import train_grid as tg
from test_prediction import _torch_rows

PARTIAL = (12, 20, 4, 24, 16)       # (B, P, N, H, K)
NEGATIVES = [(1, 1), (4, 0), (7, 3)]


def _partial_problem():
    """a module in float64, a predictor and targets in [1, K) with three single negatives: rows 0*K and 1*K of the
    embedding are gathered only through the clamp"""
    from quantization_amd import JointCodebookLoss
    B, P, N, H, K = PARTIAL
    torch.manual_seed(11)
    m = JointCodebookLoss(P, N, H, K).double()
    with torch.no_grad():
        m.linear2_bias.normal_(std=0.1)
    pred = torch.randn(B, P, dtype=torch.float64)
    idx = torch.randint(1, K, (B, N))
    for b, n in NEGATIVES:
        idx[b, n] = -100
    return m, pred, idx


def _compose64(m, pred, idx, clamp=True):
    """d(sum of the cross-entropies) / d(embedding table) and / d(hp) from the float64 restatements: prefix_fwd64, a float64
    matmul and cross-entropy, prefix_bwd64, scatter_rows64 on the clamped indexes"""
    B, P, N, H, K = PARTIAL
    P_ = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    x, ix = pred.numpy(), idx.numpy()
    scale = 0.5 * ((H / N) ** 0.5)
    hp = x @ P_["linear1.weight"].T + P_["linear1.bias"]
    A, _ = jg.prefix_fwd64(hp, P_["codebook_embedding.weight"], ix, K, scale)
    gA = np.empty_like(A)
    for n in range(N):
        z = A[n] @ P_["linear2_weight"][n].T + x @ P_["linear2b_weight"][n].T + P_["linear2_bias"][n]
        z = z - z.max(axis=1, keepdims=True)
        G = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)             # d(-log softmax[target]) / dz = softmax - onehot
        valid = ix[:, n] >= 0
        G[valid, ix[valid, n]] -= 1.0
        G[~valid] = 0.0                                                   # ignore_index: per element
        gA[n] = G @ P_["linear2_weight"][n]
    g_hp, gE, _, _ = jg.prefix_bwd64(A, gA, scale)
    rows = np.maximum(ix, 0) if clamp else ix                             # k < 0 ? 0 : k, as the forward gathered
    g_emb, _, _ = jg.scatter_rows64(gE.reshape(-1), H, B * H, rows.reshape(-1), N, B, N - 1, K, H)
    return g_emb, g_hp


def _autograd64(m, pred, idx):
    kept = []
    m.zero_grad()
    _torch_rows(m, pred, idx, keep_hp=kept).sum().backward()
    return m.codebook_embedding.weight.grad.numpy(), kept[0].grad.numpy()


def test_float64_composition_is_autograd_of_the_reference_sequence():
    m, pred, idx = _partial_problem()
    g_emb, g_hp = _compose64(m, pred, idx)
    r_emb, r_hp = _autograd64(m, pred, idx)
    assert np.abs(g_emb - r_emb).max() <= 1e-12 * np.abs(r_emb).max()
    assert np.abs(g_hp - r_hp).max() <= 1e-12 * np.abs(r_hp).max()


def test_partial_padding_trains_entry_zero_through_the_clamp():
    """rows n*K of the float64 embedding gradient are non-zero only because a negative target was clamped: present with
    the clamp and in autograd, exactly 0 when negative indexes match no row, and exactly 0 with the frames wholly padded"""
    B, P, N, H, K = PARTIAL
    m, pred, idx = _partial_problem()
    assert not (idx == 0).any()
    partial = [(b, n) for b, n in NEGATIVES if n < N - 1 and (idx[b, n + 1:] >= 0).any()]
    assert {n for _, n in partial} == {0, 1}
    g_emb, _ = _compose64(m, pred, idx)
    r_emb, _ = _autograd64(m, pred, idx)
    dropped, _ = _compose64(m, pred, idx, clamp=False)
    for n in (0, 1):
        assert np.linalg.norm(r_emb[n * K]) > 0.1 and np.linalg.norm(g_emb[n * K]) > 0.1
        assert not dropped[n * K].any()
    assert not r_emb[2 * K].any() and not g_emb[2 * K].any()             # no clamped negative in codebook 2
    whole = idx.clone()
    for b, _ in NEGATIVES:
        whole[b] = -100
    w_emb, _ = _autograd64(m, pred, whole)
    assert not w_emb[0].any() and not w_emb[K].any()


def test_relu_mask_is_torchs_at_zeros_and_subnormals():
    s = torch.tensor([0.0, -0.0, float(jg.SUBNORMAL), 1.0, -1.0], requires_grad=True)
    a = torch.relu(s)
    a.sum().backward()
    assert s.grad.tolist() == [0.0, 0.0, 1.0, 1.0, 0.0]
    assert jg.relu_mask(a.detach().numpy()).tolist() == [False, False, True, True, False]


@pytest.mark.parametrize("B,N,K,H", jg.PREFIX_CASES, ids=lambda v: str(v))
def test_prefix_cases_hold_their_inputs_and_bounds(B, N, K, H):
    hp, emb, idx, gA, scale = jg.prefix_inputs(B, N, K, H)
    assert (idx < 0).any(axis=0).all(), "a negative in every column, the last included"
    assert B < 2 or (idx == 0).any(axis=0).all()
    mag = np.abs(gA[gA != 0])
    assert mag.max() / mag.min() >= 2.0 ** 20
    A32 = jg.prefix_fwd32(hp, emb, idx, K, scale)
    A64, bA = jg.prefix_fwd64(hp, emb, idx, K, scale)
    assert A32.dtype == np.float32 and (np.abs(A32.astype(np.float64) - A64) <= bA).all()
    assert B * H < 64 or ((A32 == 0).any() and (A32 > 0).any())         # both sides of the ReLU
    g32, e32 = jg.prefix_bwd32(A32, gA, scale)
    g64, e64, bg, be = jg.prefix_bwd64(A32, gA, scale)
    assert g32.dtype == e32.dtype == np.float32
    assert (np.abs(g32.astype(np.float64) - g64) <= bg).all() and (np.abs(e32.astype(np.float64) - e64) <= be).all()
    # the last index column is never gathered
    other = idx.copy()
    other[:, N - 1] = (other[:, N - 1] + 5) % K
    assert np.array_equal(jg.prefix_fwd32(hp, emb, other, K, scale), A32)
    special = jg.scale_is_power_of_two(H, N)
    assert special == ((H, N) in ((64, 16), (64, 4)))
    if special:
        for b in jg.prefix_special_frames(B, N):
            assert idx[b, 0] >= 0
            pz, nz, sub = A32[1, b, jg.H_PZERO], A32[1, b, jg.H_NZERO], A32[1, b, jg.H_SUBNORMAL]
            assert pz == 0 and nz == 0 and sub == jg.SUBNORMAL and 0 < sub < np.finfo(np.float32).tiny
            s1 = hp[b] + emb[idx[b, 0]] * np.float32(scale)
            assert s1[jg.H_PZERO] == 0 and not np.signbit(s1[jg.H_PZERO])
            assert s1[jg.H_NZERO] == 0 and np.signbit(s1[jg.H_NZERO])
            assert jg.relu_mask(A32[1, b, [jg.H_PZERO, jg.H_NZERO, jg.H_SUBNORMAL]]).tolist() == [False, False, True]


@pytest.mark.parametrize("c", jg.SCATTER_CASES, ids=lambda c: "-".join(map(str, c[:7])))
def test_scatter_cases_hold_their_inputs_paths_and_bounds(c):
    assert jg.scatter_path(c) == c.path
    sb, sn, istride, ng = jg.scatter_strides(c)
    grad, idx = jg.scatter_inputs(c)
    assert grad.size == ng and idx.size == c.B * istride and istride >= c.N
    o32 = jg.scatter_rows32(grad, sb, sn, idx, istride, c.B, c.N, c.K, c.D)
    o64, bound, hits = jg.scatter_rows64(grad, sb, sn, idx, istride, c.B, c.N, c.K, c.D)
    assert o32.dtype == np.float32 and (np.abs(o32.astype(np.float64) - o64) <= bound).all()
    used = idx.reshape(c.B, istride)[:, :c.N]
    assert (used < 0).any() and hits.sum() == (used >= 0).sum()
    assert (hits == 0).any() and not o32[hits == 0].any() and hits[(c.N - 1) * c.K + c.K - 1] == 0
    if c.same:
        assert hits[3] == c.B and c.B >= 64
    if c.layout == "loss":       # the unused column holds indexes that must not count
        unused = idx.reshape(c.B, istride)[:, c.N]
        assert istride == c.N + 1 and ((unused >= 0) & (unused < c.K)).all()
    else:
        assert sn == 0


def test_scatter_cases_reach_every_path_the_launch_has():
    assert tg.db_alignment() == (3, 15)
    C = jg.SCATTER_CASES
    assert any(c.path[0] == 4 and c.D % 4 == 0 and c.K >= 64 for c in C)
    assert any(c.path[0] == 2 and c.K == 16 and c.D == 512 for c in C)
    assert any(c.path[0] == 1 and c.D % 4 != 0 for c in C)
    assert any(c.path[0] == 1 and c.D % 4 == 0 and c.ooff == 1 and tg.db_cw_of(c.D, c.K) > 1 for c in C)
    assert any(c.path[0] == 1 and c.D % 4 == 0 and c.goff == 1 and tg.db_cw_of(c.D, c.K) > 1 for c in C)
    assert {1, 2, 4, 8} <= {c.path[1] for c in C if c.path[2]}
    assert {(1, 3, False), (1, 5, False)} <= {c.path for c in C} and {130, 260} <= {c.D for c in C if c.path[0] == 1}
    assert any(c.path[1] > 8 and c.path[0] == 1 and c.D == 600 for c in C)
    assert {1, 63, 64, 65, 513} <= {c.B for c in C}
    assert any(c.same and c.B == 64 for c in C)
    assert {"loss", "decode"} == {c.layout for c in C}
    assert all(c.path[2] == (c.path[1] <= 8 and 8 % c.path[1] == 0) for c in C)


def test_prefix_cases_cover_the_wave_and_trip_edges():
    assert jg.PREFIX_CASES == [(1, 2, 16, 1), (3, 3, 32, 63), (5, 5, 128, 65), (130, 16, 16, 64), (7, 4, 256, 130), (66, 4, 64, 64)]
    assert any(B % 4 for B, _, _, _ in jg.PREFIX_CASES)
    assert {H < 64 for _, _, _, H in jg.PREFIX_CASES} == {True, False} and any(H == 64 for _, _, _, H in jg.PREFIX_CASES)
    assert any(H > 64 and H % 64 for _, _, _, H in jg.PREFIX_CASES)
    assert {2, 16} <= {N for _, N, _, _ in jg.PREFIX_CASES}
