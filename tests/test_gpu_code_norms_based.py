"""The norms of a store of residual codes on the GPU (mcq_code_norms_based / mcq_code_rnorms_based through
Quantizer.code_norms(base=..., assign=...) and code_rnorms; include/mcq_residual.h rule 22), BIT FOR BIT against the numpy restatement
of tests/search_bias_grid.py: per feature the codebook rows n ascending, then the base element, then the lane chains and the
butterfly of rule 2 (search_grid.norms_chains counts them).

Shapes (N, K, D): (1, 16, 24) -- no row addition at all; (8, 256, 24); (64, 256, 40); (8, 256, 260) -- the padded dim is 272, 68
float4 groups: two trips of the feature loop, and a base row of 260 floats is not 16-byte aligned from the second row on.
300 stored vectors, 3 base rows, assign with -1 and L in it."""
import numpy as np
import pytest
import torch

import search_bias_grid as bg
import search_grid as sg
import search_metric_grid as mg
import test_gpu_search as base

pytestmark = pytest.mark.gpu

SHAPES = ((1, 16, 24), (8, 256, 24), (64, 256, 40), (8, 256, 260))
B, L = 300, 3


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _padded_centers(q):
    """the fp32 rows of `prepared` with their pad columns, (N, K, Dp)"""
    N, K, Dp = q.num_codebooks, q.codebook_size, sg.padded(q.dim)
    blob = q._prepared(any_flavour=True)
    torch.cuda.synchronize()
    return blob[:N * K * Dp * 4].view(torch.float32).reshape(N, K, Dp).cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_k%d_d%d" % s)
def test_based_norms_against_the_restatement(shape):
    N, K, D = shape
    case = sg.Case("based_n%d_k%d_d%d" % shape, N, K, D, 1, B, 1, state="decode_only", codes="random")
    q = base._quantizer(case)
    kept, flat = base._store(case, q)
    C = _padded_centers(q)
    trips = (sg.padded(D) // 4 + 63) // 64
    assert sg.norms_chains(N, D)[1] == 4 * trips + 6 and trips == (2 if D == 260 else 1)
    rs = np.random.RandomState(40 + N)
    scale = float(np.abs(C).max()) * max(N, 2) ** 0.5
    cen = (rs.standard_normal((L, D)) * scale).astype(np.float32)            # of the size of a decoded vector
    assign = rs.randint(0, L, size=B).astype(np.int32)
    assign[[3, 77, 299]] = -1
    assign[[0, 150]] = L
    cen_d, assign_d = torch.from_numpy(cen).cuda(), torch.from_numpy(assign).cuda()

    t = q.code_norms(kept, base=cen_d, assign=assign_d)
    r = q.code_rnorms(kept, base=cen_d, assign=assign_d)
    assert t.dtype == r.dtype == torch.float32 and tuple(t.shape) == tuple(r.shape) == (B,)
    want = bg.restate_norms_based(C, flat, cen, assign, D)
    assert np.array_equal(_u32(t.cpu().numpy()), _u32(want)), "norms differ from rule 22"
    assert np.array_equal(_u32(r.cpu().numpy()), _u32(mg.restate_rnorms(want))), "reciprocal roots differ from rules 22 and 6"
    assert torch.equal(q.rnorms_from_norms(t).view(torch.int32), r.view(torch.int32))

    # the base matters, and where assign names no row the value is rule 2's
    plain = q.code_norms(kept)
    none = np.flatnonzero((assign < 0) | (assign >= L))
    assert np.array_equal(_u32(t.cpu().numpy()[none]), _u32(plain.cpu().numpy()[none]))
    assert int((t != plain).sum()) >= B - len(none) - 2
    # against float64, within the bound form of test_gpu_search._check_norms with the base in the chain and in the magnitudes
    ok = (assign >= 0) & (assign < L)
    full = base._decode64(C[:, :, :D], flat) + np.where(ok[:, None], cen.astype(np.float64)[np.clip(assign, 0, L - 1)], 0.0)
    mag = np.where(ok[:, None], np.abs(cen).astype(np.float64)[np.clip(assign, 0, L - 1)], 0.0)
    for n in range(N):
        mag += np.abs(C[n, :, :D]).astype(np.float64)[flat[:, n]]
    chain = max(N, sg.norms_chains(N, D)[1])
    err = np.abs(t.cpu().numpy().astype(np.float64) - (full ** 2).sum(1))
    assert (err <= 4 * chain * 2.0 ** -24 * (mag ** 2).sum(1)).all()

    # a base of zeros: equal to code_norms as floats; any integer assign is narrowed; a second call returns identical bytes
    zeros = q.code_norms(kept, base=torch.zeros_like(cen_d), assign=assign_d)
    assert bool((zeros == plain).all())
    wide = assign.astype(np.int64)
    wide[3], wide[0] = -(1 << 40), 1 << 40                                    # names no row, before and after narrowing
    assert torch.equal(q.code_norms(kept, base=cen_d, assign=torch.from_numpy(wide).cuda()).view(torch.int32), t.view(torch.int32))
    assert torch.equal(q.code_norms(kept, base=cen_d.double(), assign=assign_d).view(torch.int32), t.view(torch.int32))
    far = assign.copy()
    far[3], far[0] = -2 ** 31, 2 ** 31 - 1                                    # int32 goes to the kernel as it is: its own defence
    assert torch.equal(q.code_norms(kept, base=cen_d, assign=torch.from_numpy(far).cuda()).view(torch.int32), t.view(torch.int32))
    empty = q.code_norms(kept[:0], base=cen_d, assign=assign_d[:0])
    assert tuple(empty.shape) == (0,)
