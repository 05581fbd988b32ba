"""Fixed-point skipping is the default path of mcq_encode / mcq_encode_ex / mcq_refine_indexes: the codes must equal those of
MCQ_ENCODE_ALL_PASSES (every pass on every vector) bit for bit, and the oracle's on sampled rows.  Small batches normally take
the all-passes path (they are launch-bound); MCQ_SKIP_MIN_BATCH=0 sends them through the compaction path as well."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden import fixtures, gen
from oracle.oracle import OracleQuantizer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture
def skip_small(monkeypatch):
    monkeypatch.setenv("MCQ_SKIP_MIN_BATCH", "0")


def load_quantizer(state, D, K, N, device="cuda:0"):
    from quantization_amd import Quantizer
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for k, v in state.items():
        sd[k] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    if getattr(state, "scales_exp", None) is not None:
        q.pin_scale_factors(*state.scales_exp)
    return q.to(device)


def oracle_of(state):
    return OracleQuantizer(state["centers"], float(state["centers_scale"]), state["to_logits.weight"],
                           state["to_logits.bias"], float(state["logits_scale"]), scales_exp=getattr(state, "scales_exp", None))


def both(q, x, it, as_bytes=False):
    """(default path, MCQ_ENCODE_ALL_PASSES)"""
    assert q.skip_fixed_points is True                     # the default
    got = q.encode(x, it, as_bytes=as_bytes)
    q.skip_fixed_points = False
    try:
        ref = q.encode(x, it, as_bytes=as_bytes)
    finally:
        q.skip_fixed_points = True
    return got, ref


def raw_encode(q, x, it, as_bytes, flags, ws_vectors=None):
    """mcq_encode_ex with explicit flags and, optionally, a workspace that holds only `ws_vectors` vectors (chunked batch)"""
    from quantization_amd import _lib
    L = _lib.lib()
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    B = x.shape[0]
    pack = 2 if (as_bytes and K == 16 and N >= 2) else 1
    out = torch.empty((B, N // pack), dtype=torch.uint8 if as_bytes else torch.int64, device=x.device)
    ws_b = L.mcq_encode_workspace_bytes(ws_vectors or B, N, K, D)
    ws = torch.empty(ws_b, dtype=torch.uint8, device=x.device)
    blob = q._prepared()
    rc = L.mcq_encode_ex(x.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, it,
                         out.data_ptr() if as_bytes else None, None if as_bytes else out.data_ptr(), ws.data_ptr(), ws.numel(),
                         torch.cuda.current_stream().cuda_stream, flags | q._scale_flags)
    _lib.check(rc, "mcq_encode_ex")
    torch.cuda.synchronize()
    return out


def test_bench_shape_default_equals_all_passes_and_oracle():
    D, K, N, B = 512, 256, 8, 65536
    sd = gen.synthetic_state(103, D, K, N)
    q = load_quantizer(sd, D, K, N)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(0)
    x = torch.randn(B, D, generator=g, device="cuda:0", dtype=torch.float32)
    got, ref = both(q, x, 5, as_bytes=True)
    assert torch.equal(got, ref)
    rows = np.random.RandomState(3).choice(B, 192, replace=False)
    assert np.array_equal(got.cpu().numpy()[rows], oracle_of(sd).encode(x.cpu().numpy()[rows], 5))
    got2, ref2 = both(q, x, 2)                             # few vectors converge after one pass: the skipping path has no work to save
    assert torch.equal(got2, ref2)


@pytest.mark.parametrize("small", [False, True])
def test_iteration_counts(small, monkeypatch):
    if small:
        monkeypatch.setenv("MCQ_SKIP_MIN_BATCH", "0")
    fx = fixtures.load("trained_d64_b8_p2")
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    o = oracle_of(fx["state"])
    x = torch.from_numpy(fx["x"]).cuda()
    for it in (0, 1, 2, 5, 8):
        got, ref = both(q, x, it)
        assert torch.equal(got, ref), it
        assert np.array_equal(got.cpu().numpy(), o.compute_indexes(fx["x"], it)), it


@pytest.mark.parametrize("N", [1, 2, 4, 8, 16])
def test_codebook_counts_at_256_entries(N, skip_small):
    D, K, B = 64, 256, 3001
    sd = gen.synthetic_state(700 + N, D, K, N)
    q = load_quantizer(sd, D, K, N)
    x = gen.make_x(701 + N, B, D)
    xd = torch.from_numpy(x).cuda()
    for it in (2, 5):
        got, ref = both(q, xd, it)
        assert torch.equal(got, ref), it
        rows = np.random.RandomState(N).choice(B, 64, replace=False)
        assert np.array_equal(got.cpu().numpy()[rows], oracle_of(sd).compute_indexes(x[rows], it)), it
    b8, r8 = both(q, xd, 5, as_bytes=True)
    assert torch.equal(b8, r8)


def test_sixteen_codebooks_in_chunks_of_32768():
    D, K, N, B = 64, 256, 16, 40000                        # two chunks at the default threshold
    sd = gen.synthetic_state(720, D, K, N)
    q = load_quantizer(sd, D, K, N)
    x = gen.make_gaussian(721, B, D)
    got, ref = both(q, torch.from_numpy(x).cuda(), 5)
    assert torch.equal(got, ref)
    rows = np.concatenate([np.arange(32768 - 24, 32768 + 24), np.random.RandomState(4).choice(B, 48, replace=False)])
    assert np.array_equal(got.cpu().numpy()[rows], oracle_of(sd).compute_indexes(x[rows], 5))


@pytest.mark.parametrize("N", [8, 16])
def test_sixteen_entry_codebooks_packed_nibbles(N, skip_small):
    """pass16 (its own per-wave early exit), and the separate kernels with MCQ_PASS16=0 in a fresh process"""
    D, K, B = 48, 16, 5003
    sd = gen.synthetic_state(730 + N, D, K, N)
    q = load_quantizer(sd, D, K, N)
    x = gen.make_x(731 + N, B, D)
    xd = torch.from_numpy(x).cuda()
    o = oracle_of(sd)
    for as_bytes in (True, False):
        got, ref = both(q, xd, 5, as_bytes=as_bytes)
        assert torch.equal(got, ref)
    want = o.encode(x, 5)
    assert np.array_equal(q.encode(xd, 5).cpu().numpy(), want)
    # the separate kernels (compaction, nibble-packed output written by the emitting wave and by k_compact)
    script = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "from golden import gen\n"
        "from test_gpu_fixed_point_default import load_quantizer\n"
        f"sd = gen.synthetic_state({730 + N}, {D}, {K}, {N}); q = load_quantizer(sd, {D}, {K}, {N})\n"
        f"x = torch.from_numpy(gen.make_x({731 + N}, {B}, {D})).cuda()\n"
        "a = q.encode(x, 5); q.skip_fixed_points = False; b = q.encode(x, 5)\n"
        "c = q.encode(x, 5, as_bytes=False); q.skip_fixed_points = True; d = q.encode(x, 5, as_bytes=False)\n"
        "assert torch.equal(a, b) and torch.equal(c, d)\n"
        "np.save(sys.argv[1], a.cpu().numpy())\n")
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"mcq_p16off_{os.getpid()}_{N}.npy")
    env = dict(os.environ, MCQ_PASS16="0", MCQ_SKIP_MIN_BATCH="0")
    r = subprocess.run([sys.executable, "-c", script, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    try:
        assert np.array_equal(np.load(out), want)
    finally:
        if os.path.exists(out):
            os.remove(out)


@pytest.mark.parametrize("name", ["k512_d32_n4", "k1024_d40_n8", "k512_d16_n16", "k1024_d24_n2"])
def test_wide_codebooks_int64(name, skip_small):
    fx = fixtures.load(name)
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    x = torch.from_numpy(fx["x"]).cuda()
    for it in (2, 5):
        got, ref = both(q, x, it)
        assert torch.equal(got, ref), it
        assert np.array_equal(got.cpu().numpy(), oracle_of(fx["state"]).compute_indexes(fx["x"], it)), it


def test_chunked_batch_single_vector_and_ragged(skip_small):
    from quantization_amd import _lib
    D, K, N = 64, 256, 8
    sd = gen.synthetic_state(740, D, K, N)
    q = load_quantizer(sd, D, K, N)
    x = torch.from_numpy(gen.make_x(741, 5000, D)).cuda()
    dense = raw_encode(q, x, 5, True, _lib.MCQ_ENCODE_ALL_PASSES)
    for ws_vectors in (None, 1024, 1920):                  # one chunk; chunks of 1,024 and 1,920 with a ragged tail
        assert torch.equal(raw_encode(q, x, 5, True, 0, ws_vectors), dense), ws_vectors
        assert torch.equal(raw_encode(q, x, 5, True, 1, ws_vectors), dense), ws_vectors      # SKIP_FIXED_POINTS: accepted, no effect
    for b in (1, 2, 255, 257, 4097):
        got, ref = both(q, x[:b], 5, as_bytes=True)
        assert torch.equal(got, ref) and torch.equal(got, dense[:b]), b


def test_fp16_and_non_finite_rows(skip_small):
    fx = fixtures.load("config_b_d512_n8")
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    xh = torch.from_numpy(fx["x"][:1500]).to(torch.float16).cuda()
    got, ref = both(q, xh, 5)
    assert torch.equal(got, ref)
    assert torch.equal(got, q.encode(xh.float(), 5, as_bytes=False))
    bad = fx["x"][:600].copy()
    bad[3] = np.nan
    bad[7, 5] = np.inf
    bad[9] = -np.inf
    bad[11] = 1e30
    got, ref = both(q, torch.from_numpy(bad).cuda(), 5)
    assert torch.equal(got, ref)
    good = np.setdiff1d(np.arange(600), [3, 7, 9, 11])
    assert np.array_equal(got.cpu().numpy()[good], oracle_of(fx["state"]).compute_indexes(bad[good], 5))


def test_logits_entry_with_codes_also_runs_all_passes_and_matches_encode():
    from quantization_amd import _lib
    L = _lib.lib()
    fx = fixtures.load("trained_d64_b8_p2")
    D, K, N, B = fx["D"], fx["K"], fx["N"], fx["B"]
    q = load_quantizer(fx["state"], D, K, N)
    x = torch.from_numpy(fx["x"]).cuda()
    logits = torch.empty((B, N * K), dtype=torch.float32, device="cuda:0")
    idx = torch.empty((B, N), dtype=torch.int64, device="cuda:0")
    codes = torch.empty((B, N), dtype=torch.uint8, device="cuda:0")
    ws = torch.empty(L.mcq_encode_workspace_bytes(B, N, K, D), dtype=torch.uint8, device="cuda:0")
    for flags in (0, _lib.MCQ_ENCODE_ALL_PASSES):
        rc = L.mcq_logits_refine_codes(x.data_ptr(), B, q._prepared().data_ptr(), q._lscale_exp, N, K, D, 5, logits.data_ptr(),
                                       idx.data_ptr(), codes.data_ptr(), ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream().cuda_stream, flags | q._scale_flags)
        _lib.check(rc, "mcq_logits_refine_codes")
        torch.cuda.synchronize()
        want = q.encode(x, 5, as_bytes=False)
        assert torch.equal(idx, want) and torch.equal(codes.to(torch.int64), want), flags


def test_refine_from_a_fixed_point_retires_every_vector_after_one_pass(skip_small):
    from quantization_amd import _lib
    L = _lib.lib()
    fx = fixtures.load("trained_d64_b8_p2")
    D, K, N = fx["D"], fx["K"], fx["N"]
    q = load_quantizer(fx["state"], D, K, N)
    x = torch.from_numpy(fx["x"]).cuda()
    idx = q.encode(x, 5, as_bytes=False)
    for _ in range(40):                                     # walk every vector to its fixed point, one pass at a time
        nxt = q._refine_indexes(x, idx)
        if torch.equal(nxt, idx):
            break
        idx = nxt
    keep = (q._refine_indexes(x, idx) == idx).all(dim=1)
    xs, start = x[keep].contiguous(), idx[keep].contiguous()
    B = xs.shape[0]
    assert B > 1000
    out = torch.empty_like(start)
    ws = torch.empty(L.mcq_encode_workspace_bytes(B, N, K, D), dtype=torch.uint8, device="cuda:0")
    rc = L.mcq_refine_indexes(xs.data_ptr(), B, q._prepared().data_ptr(), N, K, D, 5, start.data_ptr(), out.data_ptr(),
                              ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "mcq_refine_indexes")
    torch.cuda.synchronize()
    assert torch.equal(out, start)
