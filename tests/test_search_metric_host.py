"""Host-side checks of the inner-product and cosine metrics of the search over stored codes (no GPU): the new entry points
are exported and bound, every argument check of include/mcq.h answers before anything touches the device (null device
pointers, as tests/test_search_host.py does for the L2 entry points), the ABI version did not move, Quantizer.search refuses an
unknown metric before it looks at a tensor, and the numpy restatement the GPU tests compare with (tests/search_metric_grid.py)
agrees with a brute-force float64 ranking where every float32 operation is exact."""
import ctypes

import numpy as np
import pytest

import search_grid as sg
import search_metric_grid as mg


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


NEW = ("mcq_search_scan_metric", "mcq_code_rnorms", "mcq_rnorms_from_norms")


def test_new_entry_points_are_exported_and_bound():
    m = _lib()
    L = m.lib()
    for name in NEW:
        assert name in m.SYMBOLS
        f = getattr(L, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    assert len(L.mcq_search_scan_metric.argtypes) == 14             # mcq_search_scan's thirteen and the metric
    assert (m.MCQ_SEARCH_L2, m.MCQ_SEARCH_IP, m.MCQ_SEARCH_COS) == (0, 1, 2) == tuple(mg.CODE[x] for x in ("l2", "ip", "cosine"))
    assert L.mcq_abi_version() == 7
    hdr = open(sg.HDR.replace("quantization_amd/csrc/mcq_search_kernels.h", "include/mcq.h")).read()
    for name, v in (("MCQ_SEARCH_L2", 0), ("MCQ_SEARCH_IP", 1), ("MCQ_SEARCH_COS", 2)):
        assert f"#define {name} {v}" in hdr


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    U, I, W = m.MCQ_EUNSUPPORTED, m.MCQ_EINVAL, m.MCQ_EWORKSPACE
    scan = L.mcq_search_scan_metric
    for metric in (0, 1, 2):
        # the domain, exactly as for mcq_search_scan, before any pointer is looked at
        for K in (512, 1024, 8, 2048):
            assert scan(None, 4, None, None, 4, 4, K, 10, metric, None, None, None, 0, None) == U
        assert scan(None, 4, None, None, 4, 128, 256, 10, metric, None, None, None, 0, None) == U       # N > 64
        assert scan(None, 4, None, None, 4, 8, 256, 65, metric, None, None, None, 0, None) == U         # k > 64
        assert scan(None, 4, None, None, 1 << 31, 8, 256, 10, metric, None, None, None, 0, None) == U   # B > 2^31 - 1
        assert scan(None, 4, None, None, 4, 3, 256, 10, metric, None, None, None, 0, None) == I         # N not a power of two
        assert scan(None, 4, None, None, 4, 8, 256, 0, metric, None, None, None, 0, None) == I          # k < 1
        assert scan(None, -1, None, None, 4, 8, 256, 10, metric, None, None, None, 0, None) == I
        assert scan(None, 4, None, None, -1, 8, 256, 10, metric, None, None, None, 0, None) == I
        assert scan(None, 4, None, None, 4, 8, 256, 10, metric, None, None, None, 0, None) == I         # null pointers
        assert scan(None, 0, None, None, 4, 8, 256, 10, metric, None, None, None, 0, None) == 0         # no queries: nothing to do
    # an unknown metric, with everything else in order and with nothing to do alike
    fake = ctypes.c_void_p(1 << 20)
    need = L.mcq_search_workspace_bytes(4, 1000, 8, 256, 10)
    for metric in (-1, 3, 7, 1 << 20):
        assert scan(fake, 4, fake, fake, 1000, 8, 256, 10, metric, fake, fake, fake, need, None) == I
        assert scan(None, 0, None, None, 4, 8, 256, 10, metric, None, None, None, 0, None) == I
    # w: needed by L2 and by the cosine when there is a store, ignored by the inner product.  With w in order (or not needed)
    # the call goes on to the next check, the workspace, which is short here: still nothing touches the device
    for metric, want in ((0, I), (2, I), (1, W)):
        assert scan(fake, 4, fake, None, 1000, 8, 256, 10, metric, fake, fake, fake, need - 1, None) == want
    for metric in (0, 1, 2):
        assert scan(fake, 4, fake, fake, 1000, 8, 256, 10, metric, fake, fake, fake, need - 1, None) == W
        assert scan(fake, 4, fake, fake, 1000, 8, 256, 10, metric, fake, fake, fake, 0, None) == W
        assert scan(fake, 4, ctypes.c_void_p((1 << 20) + 4), fake, 1000, 8, 256, 10, metric, fake, fake, fake, need, None) == I
        assert scan(fake, 4, fake, fake, 1000, 8, 256, 10, metric, fake, fake, None, need, None) == I   # no workspace at all
        assert scan(fake, 4, fake, fake, 1000, 8, 256, 10, metric, None, fake, fake, need, None) == I   # no output
    # the reciprocal roots
    for K in (512, 1024, 8, 2048):
        assert L.mcq_code_rnorms(None, 4, None, 4, K, 64, None, None) == U
    assert L.mcq_code_rnorms(None, 1 << 31, None, 8, 256, 64, None, None) == U
    assert L.mcq_code_rnorms(None, 4, None, 8, 256, 20000, None, None) == U
    assert L.mcq_code_rnorms(None, -1, None, 8, 256, 64, None, None) == I
    assert L.mcq_code_rnorms(None, 4, None, 8, 256, 64, None, None) == I
    assert L.mcq_code_rnorms(None, 4, None, 3, 256, 64, None, None) == I
    assert L.mcq_code_rnorms(None, 0, None, 8, 256, 64, None, None) == 0
    assert L.mcq_rnorms_from_norms(None, -1, None, None) == I
    assert L.mcq_rnorms_from_norms(None, 4, None, None) == I
    assert L.mcq_rnorms_from_norms(fake, 4, None, None) == I
    assert L.mcq_rnorms_from_norms(None, 1 << 31, None, None) == U
    assert L.mcq_rnorms_from_norms(None, 0, None, None) == 0


def test_unknown_metric_is_a_value_error_before_any_device_work():
    _lib()
    import torch
    from quantization_amd import Quantizer
    from quantization_amd._lib import McqError
    q = Quantizer(24, 16, 4)
    x = torch.zeros(3, 24)
    codes = torch.zeros(10, 4, dtype=torch.uint8)
    for bad in ("nonsense", "L2", "cos", "", None, 1):
        with pytest.raises(ValueError):
            q.search(x, codes, k=2, metric=bad)
        with pytest.raises(ValueError):
            q._search_scan(torch.zeros(3, 4, 16), codes, torch.zeros(10), 2, metric=bad)
    # ... and a known one on CPU tensors is the device error every search entry point gives (no CPU fallback)
    for good in ("l2", "ip", "cosine"):
        with pytest.raises(McqError):
            q.search(x, codes, k=2, metric=good)
    with pytest.raises(McqError):
        q.code_rnorms(codes)
    with pytest.raises(McqError):
        q.rnorms_from_norms(torch.zeros(10))


def test_metric_cases_are_the_l2_table():
    # the claims of that table are checked by tests/test_search_host.py::test_gpu_cases_reach_what_they_claim; the plan
    # has no metric argument, in the library (mcq_search_workspace_bytes) or in the mirror
    assert mg.CASES is sg.CASES and mg.METRICS == ("ip", "cosine")
    assert {c.N for c in mg.CASES} >= {1, 2, 8, 16, 64} and {c.K for c in mg.CASES} == {16, 64, 256}
    assert any(c.B == 1 for c in mg.CASES) and any(c.packed for c in mg.CASES) and any(c.queries == "fp16" for c in mg.CASES)
    assert any(c.state == "decode_only" for c in mg.CASES) and {c.strided for c in mg.CASES if c.codes == "dup16"} == {False, True}
    for f in ("tiles", "sliced", "partial", "short", "strided"):
        assert sum(bool(getattr(c, f)) for c in mg.CASES) >= 2, f


def test_restatement_of_the_metrics():
    """dyadic tables and power-of-four norms make every float32 operation exact, so a float64 brute force must agree to the bit;
    planted duplicate codes make position decide ties under both metrics"""
    rs = np.random.RandomState(9)
    Q, N, K, B, k = 3, 4, 16, 40, 12
    T = (rs.randint(-64, 64, size=(Q, N, K)) / 8.0).astype(np.float32)
    codes = rs.randint(0, K, size=(B, N)).astype(np.uint8)
    codes[7] = codes[31] = codes[3] = codes[20]
    t = (4.0 ** rs.randint(-3, 4, size=B)).astype(np.float32)
    t[[3, 7, 20, 31]] = 4.0 ** -3                                # equal, and the largest reciprocal roots (8): equal best scores
    t[5] = 0.0                                                   # an all-zero reconstruction
    r = mg.restate_rnorms(t)
    assert r.dtype == np.float32 and r[5] == 0 and r[3] == 8
    assert np.array_equal(r[t > 0].astype(np.float64), 1.0 / np.sqrt(t[t > 0].astype(np.float64)))
    # correctly rounded where it is not exact, and finite at the ends of the range
    odd = np.array([2.0, 3.0, 1e-30, 1e30, 1e-45, 3.4e38], dtype=np.float32)
    want = (1.0 / np.sqrt(odd.astype(np.float64)).astype(np.float32).astype(np.float64)).astype(np.float32)
    assert np.array_equal(mg.restate_rnorms(odd).view(np.uint32), want.view(np.uint32))
    assert np.isnan(mg.restate_rnorms(np.array([-1.0, np.nan], dtype=np.float32))).all()
    for q in range(Q):
        for n in range(N):
            T[q, n, codes[20, n]] = -8.0                         # the duplicated row is the best of every query
    for metric in mg.METRICS:
        got_s, got_i = mg.restate_metric(T, r, codes, k, metric)
        for q in range(Q):
            S = [sum(float(T[q, n, codes[b, n]]) for n in range(N)) for b in range(B)]
            s64 = S if metric == "ip" else [S[b] * float(r[b]) for b in range(B)]
            order = sorted(range(B), key=lambda b: (s64[b], b))[:k]
            assert got_i[q].tolist() == order, metric
            assert got_s[q].astype(np.float64).tolist() == [s64[b] for b in order]
            assert got_i[q, :4].tolist() == [3, 7, 20, 31]
        s, i = mg.restate_metric(T, r[:5], codes[:5], k, metric)
        assert (i[:, 5:] == -1).all() and np.isinf(s[:, 5:]).all() and (s[:, 5:] > 0).all() and (i[:, :5] >= 0).all()
        s, i = mg.restate_metric(T, r[:0], codes[:0], k, metric)
        assert (i == -1).all() and np.isinf(s).all()
    # the sum is rule 3's without its last addition, signed zeros included; "l2" is search_grid's own restatement
    Tz = np.zeros((1, 2, 16), dtype=np.float32)
    Tz[0, :, 1] = -0.0
    cz = np.array([[0, 0], [1, 1], [0, 1]], dtype=np.uint8)
    assert mg.restate_sums(Tz, cz).view(np.uint32).tolist() == [[0, 0x80000000, 0]]
    assert np.array_equal(mg.restate_metric_scores(T, t, codes, "l2"), sg.restate_scores(T, t, codes))
