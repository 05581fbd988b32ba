"""The encode on two lanes (include/mcq_lanes.h) against the one-lane sequence of the same library, byte for byte.

Two lanes are forced with MCQ_ENCODE_LANES=2 MCQ_ENCODE_LANES_MIN=0, one lane with MCQ_ENCODE_LANES=1; mcq_last_encode_lanes()
says what a call actually did.  Small shapes against the CPU oracle as well, the two-byte shape against its reference fixture.

  sizes      1 (lane 1 gets nothing), 2 (one vector per lane), 129 and 257 (halves that are no multiple of the 128-row tile),
             8,320 (each lane above one wave's worth of every kernel), and 700 vectors in a workspace whose shares hold 128:
             six chunks, three per lane, so that each lane reuses its share
  shapes     8 x 256, 4 x 256 and 16 x 256 at dim 64, 16 x 16 (the LDS-resident pass, one launch per chunk), 4 x 512 (two-byte entries)
  variants   0, 1 and 5 passes; skipping on and off, with every per-chunk threshold at 0 so that each lane's 4,160 vectors take the
             skipping, lazy-table and dense E / R forms; fp16 frames; int64 and uint8 results
  ordering   on a non-default stream: a copy fills x right before the call, a torch op reads the codes right after it, no
             synchronisation in between, 20 rounds on alternating inputs (a missing fork or join wait shows as stale or torn codes)
  others     two host threads at once; encode_from_host in 4 chunks; a captured encode takes one lane and replays correctly;
             mcq_profile_encode keeps its categories and launch counts per chunk
"""
import ctypes
import threading

import numpy as np
import pytest
import torch

from golden import fixtures, gen
from test_gpu_parity import load_quantizer, oracle_of

pytestmark = pytest.mark.gpu

D = 64
SIZES = (1, 2, 129, 257, 8320)
ORACLE_ROWS = 257                    # the oracle checks the first rows of the largest batch, and the small batches whole
TWO = {"MCQ_ENCODE_LANES": "2", "MCQ_ENCODE_LANES_MIN": "0"}
ONE = {"MCQ_ENCODE_LANES": "1"}
HOOKS = ("MCQ_ENCODE_LANES", "MCQ_ENCODE_LANES_MIN")
X_FP16 = 4                           # MCQ_ENCODE_X_FP16


def _mods():
    from quantization_amd import _lib
    L = _lib.lib()
    L.mcq_last_encode_lanes.restype = ctypes.c_int
    L.mcq_last_encode_lanes.argtypes = []
    return _lib, L


def _env(monkeypatch, env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


_CACHE = {}


def _case(N, K, d=D):
    """per shape, once: state, quantizer, oracle, 8,320 frames on host and device"""
    if (N, K, d) not in _CACHE:
        sd = gen.synthetic_state(4100 + N + K, d, K, N)
        x = gen.make_gaussian(4101 + N + K, max(SIZES), d)
        _CACHE[(N, K, d)] = dict(q=load_quantizer(sd, d, K, N), o=oracle_of(sd), x=x, xd=torch.from_numpy(x).cuda())
    return _CACHE[(N, K, d)]


def _encode(q, xd, iters, flags=0, i64=False, ws_vectors=None, stream=None):
    """mcq_encode_ex on `stream` (default: the current one) -> (codes as a device tensor, lanes of the call)"""
    _lib, L = _mods()
    B, N, K, d = xd.shape[0], q.num_codebooks, q.codebook_size, q.dim
    with torch.no_grad():
        blob = q._prepared()
    pack = 2 if (not i64 and K == 16 and N >= 2) else 1
    # (empty, not zeros: a fill enqueued on the allocating thread's current stream would race an encode on another stream)
    out = torch.empty((B, N), dtype=torch.int64, device="cuda:0") if i64 else torch.empty((B, N // pack), dtype=torch.uint8, device="cuda:0")
    if ws_vectors is None:
        nws = L.mcq_encode_workspace_bytes(B, N, K, d)
    else:       # a workspace that holds exactly ws_vectors (the size is linear in the chunk)
        w1, w2 = L.mcq_encode_workspace_bytes(1, N, K, d), L.mcq_encode_workspace_bytes(2, N, K, d)
        nws = w1 + (w2 - w1) * (ws_vectors - 1)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
    st = (stream or torch.cuda.current_stream()).cuda_stream
    rc = L.mcq_encode_ex(xd.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, d, iters, None if i64 else out.data_ptr(),
                         out.data_ptr() if i64 else None, ws.data_ptr(), nws, st, flags | q._scale_flags)
    lanes = L.mcq_last_encode_lanes()
    assert rc == 0, rc
    return out, lanes, ws


def _both(monkeypatch, q, xd, iters, **kw):
    """(one-lane codes, two-lane codes) as numpy, the lane counts checked"""
    _env(monkeypatch, ONE)
    one, l1, ws1 = _encode(q, xd, iters, **kw)
    _env(monkeypatch, TWO)
    two, l2, ws2 = _encode(q, xd, iters, **kw)
    torch.cuda.synchronize()
    assert l1 == 1 and l2 == (2 if xd.shape[0] >= 2 else 1), (xd.shape[0], l1, l2)
    return one.cpu().numpy(), two.cpu().numpy()


@pytest.mark.parametrize("N,K", [(8, 256), (4, 256), (16, 256), (16, 16)])
def test_sizes_per_shape(N, K, monkeypatch):
    c = _case(N, K)
    i64 = K == 16                    # (16 x 16 as int64: the byte form packs nibbles, which the oracle row check below does not read)
    for B in SIZES:
        one, two = _both(monkeypatch, c["q"], c["xd"][:B], 5, i64=i64)
        assert np.array_equal(one, two), (N, K, B)
        rows = min(B, ORACLE_ROWS)
        assert np.array_equal(two[:rows].astype(np.int64), c["o"].compute_indexes(c["x"][:rows], 5).astype(np.int64)), (N, K, B)
    # six chunks of at most 128 vectors, three per lane; the one-lane run of the same workspace takes chunks of 256
    one, two = _both(monkeypatch, c["q"], c["xd"][:700], 5, i64=i64, ws_vectors=256)
    assert np.array_equal(one, two) and np.array_equal(one, _both(monkeypatch, c["q"], c["xd"][:700], 5, i64=i64)[0]), (N, K)


def test_packed_nibbles_of_the_lds_resident_pass(monkeypatch):
    c = _case(16, 16)
    for B in (2, 257, 8320):
        one, two = _both(monkeypatch, c["q"], c["xd"][:B], 5)
        assert one.shape == (B, 8) and np.array_equal(one, two), B
    assert np.array_equal(two[:ORACLE_ROWS], c["o"].encode(c["x"][:ORACLE_ROWS], 5, as_bytes=True))


def test_two_byte_entries_against_the_fixture(monkeypatch):
    fx = fixtures.load("k512_d32_n4")
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    o = oracle_of(fx["state"])
    xd = torch.from_numpy(fx["x"]).cuda()
    for it in fx["iters"]:
        for B in (fx["B"], 129):
            one, two = _both(monkeypatch, q, xd[:B], it, i64=True)
            assert np.array_equal(one, two), (it, B)
            assert np.array_equal(two, o.compute_indexes(fx["x"][:B], it).astype(np.int64)), (it, B)
        fixtures.check_codes(fx, it, _both(monkeypatch, q, xd, it, i64=True)[1], f"two lanes, iters={it}")


@pytest.mark.parametrize("iters", [0, 1, 5])
@pytest.mark.parametrize("all_passes", [False, True])
def test_passes_and_skipping(iters, all_passes, monkeypatch):
    """each lane's 4,160 vectors on the forms the headline's lanes of 32,768 take: skipping with compaction, lazy cousin tables,
    dense E / R (their thresholds at 0); and as shipped at this size"""
    _lib, _ = _mods()
    c = _case(8, 256)
    flags = _lib.MCQ_ENCODE_ALL_PASSES if all_passes else 0
    want = None
    for mins in (None, "0"):
        for k in ("MCQ_SKIP_MIN_BATCH", "MCQ_LAZY_TABLES_MIN", "MCQ_ER_DENSE_MIN"):
            monkeypatch.delenv(k, raising=False) if mins is None else monkeypatch.setenv(k, mins)
        for B, i64 in ((257, False), (8320, False), (8320, True)):
            one, two = _both(monkeypatch, c["q"], c["xd"][:B], iters, flags=flags, i64=i64)
            assert one.dtype == (np.int64 if i64 else np.uint8) and np.array_equal(one, two), (iters, all_passes, mins, B, i64)
            if B == 8320:
                want = two.astype(np.int64) if want is None else want
                assert np.array_equal(two.astype(np.int64), want)            # every form, both result types: the same codes
    assert np.array_equal(want[:ORACLE_ROWS], c["o"].compute_indexes(c["x"][:ORACLE_ROWS], iters).astype(np.int64))


def test_fp16_frames(monkeypatch):
    c = _case(8, 256)
    for B in (129, 8320):            # (129: the second lane's frames start at an odd row)
        xh = c["xd"][:B].half().contiguous()
        one, two = _both(monkeypatch, c["q"], xh, 5, flags=X_FP16)
        assert np.array_equal(one, two), B
        _env(monkeypatch, ONE)
        wide = _encode(c["q"], xh.float().contiguous(), 5)[0]
        assert np.array_equal(two, wide.cpu().numpy()), B


def test_ordering_on_a_busy_stream(monkeypatch):
    c = _case(8, 256)
    q, B = c["q"], 8320
    srcs = [c["xd"][:B].contiguous(), torch.from_numpy(gen.make_gaussian(4190, B, D)).cuda()]
    _env(monkeypatch, ONE)
    want = [q.encode(s, 5).to(torch.int64) for s in srcs]
    torch.cuda.synchronize()
    assert not torch.equal(want[0], want[1])
    _, L = _mods()
    _env(monkeypatch, TWO)
    s = torch.cuda.Stream()
    big = torch.randn(2048, 2048, device="cuda:0")
    x = torch.zeros_like(srcs[0])
    got = []
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for r in range(20):
            busy = big @ big                         # keeps the stream busy while the host runs ahead into the call
            x.copy_(srcs[r & 1])                     # written on the stream right before the call
            codes = q.encode(x, 5)
            assert L.mcq_last_encode_lanes() == 2
            got.append(codes.to(torch.int64) + 0)    # read on the stream right after the call
        del busy
    s.synchronize()
    for r, g in enumerate(got):                      # (the first mismatch ends it)
        assert torch.equal(g, want[r & 1]), f"round {r}: the codes are not those of the input written before the call"
    torch.cuda.current_stream().wait_stream(s)


def test_two_host_threads(monkeypatch):
    c = _case(8, 256)
    q = c["q"]
    with torch.no_grad():
        q._prepared()
    xs = [c["xd"][:4000].contiguous(), c["xd"][4000:8320].contiguous()]
    _env(monkeypatch, ONE)
    want = [_encode(q, x, 5)[0] for x in xs]
    torch.cuda.synchronize()
    _env(monkeypatch, TWO)
    res, errs = [None, None], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            keep = []
            for _ in range(5):
                out, lanes, ws = _encode(q, xs[t], 5, stream=s)
                keep.append((out, ws))
                assert lanes == 2
            s.synchronize()
            res[t] = [o for o, _ in keep]
        except Exception as e:          # noqa: BLE001 -- reported on the main thread
            errs.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for t in range(2):
        for o in res[t]:
            assert torch.equal(o, want[t]), t


def test_encode_from_host_in_four_chunks(monkeypatch):
    c = _case(8, 256)
    B = 4 * 2100 - 37
    _env(monkeypatch, ONE)
    want = c["q"].encode(c["xd"][:B], 5).cpu()
    _env(monkeypatch, TWO)
    _, L = _mods()
    got = c["q"].encode_from_host(torch.from_numpy(c["x"][:B]), 5, chunk=2100)
    assert L.mcq_last_encode_lanes() == 2
    assert torch.equal(got, want)


def test_a_captured_encode_takes_one_lane(monkeypatch):
    c = _case(8, 256)
    q = c["q"]
    _, L = _mods()
    xa, xb = c["xd"][:4160].contiguous(), c["xd"][4160:8320].contiguous()
    _env(monkeypatch, ONE)
    want_a, want_b = q.encode(xa, 5), q.encode(xb, 5)
    _env(monkeypatch, TWO)
    static_x = xa.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q.encode(static_x, 5)
        assert L.mcq_last_encode_lanes() == 2          # not capturing: two lanes (and the side stream exists before the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_codes = q.encode(static_x, 5)
        lanes = L.mcq_last_encode_lanes()
    assert lanes == 1
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_codes, want_a)
    static_x.copy_(xb)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_codes, want_b)


def test_profile_encode_keeps_its_categories(monkeypatch):
    """the profiled encode of 8,320 vectors: with two lanes it times two chunks of 4,160 on one stream -- per chunk the
    categories and interval counts of a one-lane profile of 4,160 vectors"""
    _lib, L = _mods()
    c = _case(8, 256)
    q, N, K = c["q"], 8, 256
    with torch.no_grad():
        blob = q._prepared()
    cap = 32

    def profile(B):
        nws = L.mcq_encode_workspace_bytes(B, N, K, D)
        ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
        ms, n = (ctypes.c_float * cap)(), (ctypes.c_int * cap)()
        x = c["xd"][:B].contiguous()
        ncat = L.mcq_profile_encode(x.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, 5, ws.data_ptr(), nws,
                                    torch.cuda.current_stream().cuda_stream, ms, n, cap)
        assert 0 < ncat <= cap, ncat
        assert L.mcq_last_encode_lanes() == 1
        return {L.mcq_profile_category_name(i).decode(): n[i] for i in range(ncat)}

    _env(monkeypatch, ONE)
    whole, half = profile(8320), profile(4160)
    _env(monkeypatch, TWO)
    lanes = profile(8320)
    assert set(lanes) == set(whole) == set(half)
    assert lanes == {k: 2 * v for k, v in half.items()}, (lanes, half)
    _env(monkeypatch, ONE)
    one, _, _ = _encode(q, c["xd"][:8320], 5, flags=_lib.MCQ_ENCODE_ALL_PASSES)
    _env(monkeypatch, TWO)
    two, _, _ = _encode(q, c["xd"][:8320], 5, flags=_lib.MCQ_ENCODE_ALL_PASSES)
    assert torch.equal(one, two)
