"""Fixed-point skipping where the capped, strided pass kernels really stride.  From the fourth pass on, k_tf_stage0,
k_tf_pair0s, k_tf_level1 and the last k_tf_comb of a skipping encode run at most kCapStage0 / kCapWave workgroups that walk
the virtual grid of the active vectors (tests/skip_grid.py mirrors that arithmetic).  Every case here is checked three ways:
its codes equal MCQ_ENCODE_ALL_PASSES bit for bit in every output form that applies, chosen rows equal the oracle's (the
first and last row of every chunk, up to 64 rows still active at the last pass, some random ones), and the activity measured
on the all-passes path shows that the cap of each kernel the case names binds -- and, where the case says so, that the
strided loop goes round at least twice."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import skip_grid as sg
from golden import fixtures, gen
from test_gpu_fixed_point_default import load_quantizer, oracle_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = sg.constants()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _lib():
    from quantization_amd import _lib as lib
    return lib


def raw_encode_ws(q, x, it, as_bytes, all_passes, ws_vectors):
    """mcq_encode_ex with a caller-sized workspace of exactly ws_vectors vectors (chunks beyond default_chunk allowed)"""
    lib = _lib()
    L = lib.lib()
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    B = x.shape[0]
    pack = 2 if (as_bytes and K == 16 and N >= 2) else 1
    out = torch.empty((B, N // pack), dtype=torch.uint8 if as_bytes else torch.int64, device=x.device)
    ws = torch.empty(sg.ws_bytes(L, N, K, D, ws_vectors), dtype=torch.uint8, device=x.device)
    blob = q._prepared()
    flags = (lib.MCQ_ENCODE_ALL_PASSES if all_passes else 0) | q._scale_flags | (4 if x.dtype == torch.float16 else 0)
    rc = L.mcq_encode_ex(x.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, it,
                         out.data_ptr() if as_bytes else None, None if as_bytes else out.data_ptr(), ws.data_ptr(), ws.numel(),
                         torch.cuda.current_stream().cuda_stream, flags)
    lib.check(rc, "mcq_encode_ex")
    torch.cuda.synchronize()
    return out


def run(q, x, case, it, as_bytes, all_passes):
    if case.ws is not None:
        return raw_encode_ws(q, x, it, as_bytes, all_passes, case.ws)
    q.skip_fixed_points = not all_passes
    try:
        return q.encode(x, it, as_bytes=as_bytes)
    finally:
        q.skip_fixed_points = True


def activity(q, x, passes, chunk, start=None):
    """the all-passes path one pass at a time: (indexes after `passes` passes, counts[p - 1][c] = vectors of chunk c active
    when pass p starts, rows active at the last pass).  Active at pass p: pass p - 1 changed the indexes (a fixed point stays
    one, so this is exactly what k_compact leaves in the packed list)"""
    B = x.shape[0]
    starts = np.arange(0, B, chunk)
    idx = q.encode(x, 0, as_bytes=False) if start is None else start
    counts = np.zeros((passes, len(starts)), np.int64)
    counts[0] = np.diff(np.append(starts, B))
    late = np.ones(B, bool)
    for p in range(1, passes + 1):
        nxt = q._refine_indexes(x, idx)
        if p < passes:
            ch = (nxt != idx).any(dim=1).cpu().numpy()
            counts[p] = np.add.reduceat(ch.astype(np.int64), starts)
            if p == passes - 1:
                late = ch
        idx = nxt
    return idx, counts, late


def check_profile(case, counts, chunk, pass16=True):
    """the case's precondition: the caps it names bind at a capped pass (>= 4) of a skipping chunk, and its multi-stride
    kernels loop at least twice there.  Returns {kernel: most strides seen}"""
    smb = C["skip_min_batch"] if case.skip_min_batch is None else case.skip_min_batch
    bound, most = set(), {}
    for ci, (lo, Bc) in enumerate(sg.chunks(case.B, chunk)):
        if not sg.skips(Bc, case.N, case.K, case.passes, smb, pass16):
            continue
        for p in range(4, case.passes + 1):
            for k in sg.capped_kernels(case.N, case.K):
                if sg.binds(k, Bc, case.N, case.K, C):
                    bound.add(k)
                s = sg.strides(k, int(counts[p - 1][ci]), Bc, case.N, case.K, C)
                most[k] = max(most.get(k, 0), s)
    assert set(case.binds) <= bound, (case.name, sorted(bound))
    for k in case.multi:
        assert most.get(k, 0) >= 2, (case.name, k, most, counts.tolist())
    return most


def pick_rows(B, chunk, late, seed, exclude=()):
    rs = np.random.RandomState(seed)
    rows = set()
    for lo, Bc in sg.chunks(B, chunk):
        rows |= {lo, lo + Bc - 1}
    act = np.setdiff1d(np.flatnonzero(late), exclude)
    if len(act) > 64:
        act = rs.choice(act, 64, replace=False)
    rows |= set(act.tolist())
    rows |= set(rs.choice(B, 32, replace=False).tolist())
    return np.setdiff1d(np.array(sorted(rows)), exclude), len(act)


def check(case, q, o, x, xd=None, exclude=()):
    """the three references of a case; returns (int64 codes, activity counts)"""
    xd = torch.from_numpy(x).cuda() if xd is None else xd
    forms = [False] + ([True] if case.K <= 256 else [])     # int64; u8 (nibble-packed for K = 16)
    got64 = None
    for as_bytes in forms:
        got = run(q, xd, case, case.passes, as_bytes, False)
        ref = run(q, xd, case, case.passes, as_bytes, True)
        assert torch.equal(got, ref), (case.name, as_bytes, int((got != ref).any(dim=1).sum()))
        if not as_bytes:
            got64 = got
    L = _lib().lib()
    per, _ = sg.ws_layout(L, case.N, case.K, case.D)
    chunk = case.chunk(per)
    final, counts, late = activity(q, xd, case.passes, chunk)
    assert torch.equal(final, got64), case.name            # the pass-at-a-time trace ends where the encode does
    check_profile(case, counts, chunk)
    rows, nlate = pick_rows(case.B, chunk, late, case.N * 31 + case.K, exclude)
    assert nlate >= min(64, int(np.setdiff1d(np.flatnonzero(late), exclude).size))
    want = o.compute_indexes(x[rows], case.passes).astype(np.int64)
    assert np.array_equal(got64.cpu().numpy()[rows], want), case.name
    return got64, counts


def setup(case):
    seed = 5000 + 7 * case.N + case.K + case.D
    sd = gen.synthetic_state(seed, case.D, case.K, case.N)
    q = load_quantizer(sd, case.D, case.K, case.N)
    x = gen.make_kind(case.kind, seed + 1, case.B, case.D)
    return q, oracle_of(sd), x


def _env(monkeypatch, case):
    if case.skip_min_batch is None:
        monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    else:
        monkeypatch.setenv("MCQ_SKIP_MIN_BATCH", str(case.skip_min_batch))


@pytest.mark.parametrize("case", sg.SHAPES + sg.BIG + sg.PASSES + sg.THRESHOLD, ids=lambda c: c.name)
def test_skip_equals_all_passes_and_oracle(case, monkeypatch):
    _env(monkeypatch, case)
    q, o, x = setup(case)
    check(case, q, o, x)


def _trained():
    fx = fixtures.load("trained_d512_b8_p2")
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    x = gen.make_kind(str(fx["x_kind"]), int(fx["x_seed"]) + 1000, 65536, fx["D"])
    return fx, q, oracle_of(fx["state"]), x


def test_trained_state_low_activity(monkeypatch):
    """a trained state on its own generator's frames: about 0.4 % of the vectors are still active at pass 5"""
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    fx, q, o, x = _trained()
    case = sg.Case("trained_d512", 8, 256, 512, 65536, binds=(sg.S0, sg.P0, sg.L1))
    _, counts = check(case, q, o, x)
    assert 0 < counts[4].sum() < 0.02 * case.B, counts.tolist()


def test_every_vector_fixed_before_pass_4(monkeypatch):
    """a batch whose vectors are all fixed points before pass 4: the capped kernels of passes 4 and 5 see nact = 0"""
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    fx, q, o, x = _trained()
    xd = torch.from_numpy(x).cuda()
    i2 = q.encode(xd, 2, as_bytes=False)
    fixed = (q._refine_indexes(xd, i2) == i2).all(dim=1).cpu().numpy()
    B = 20000
    rows = np.flatnonzero(fixed)
    assert rows.size >= B
    xs = np.ascontiguousarray(x[rows[:B]])
    case = sg.Case("trained_fixed", 8, 256, 512, B, binds=(sg.S0, sg.P0, sg.L1))
    _, counts = check(case, q, o, xs)
    assert counts[3].sum() == 0 and counts[4].sum() == 0, counts.tolist()


def test_refine_from_random_starts(monkeypatch):
    """mcq_refine_indexes with 5 passes (skipping) against 5 single passes (no skipping), late-active rows against the
    oracle's pass iterated from the same start"""
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    case = sg.Case("refine_n8_k256", 8, 256, 64, 65536, binds=(sg.S0, sg.P0, sg.L1), multi=(sg.S0, sg.P0, sg.L1))
    q, o, x = setup(case)
    xd = torch.from_numpy(x).cuda()
    start_np = np.random.RandomState(17).randint(0, case.K, (case.B, case.N)).astype(np.int64)
    start = torch.from_numpy(start_np).cuda()
    lib = _lib()
    L = lib.lib()
    out = torch.empty_like(start)
    ws = torch.empty(L.mcq_encode_workspace_bytes(case.B, case.N, case.K, case.D), dtype=torch.uint8, device="cuda:0")
    rc = L.mcq_refine_indexes(xd.data_ptr(), case.B, q._prepared().data_ptr(), case.N, case.K, case.D, case.passes,
                              start.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    lib.check(rc, "mcq_refine_indexes")
    torch.cuda.synchronize()
    per, _ = sg.ws_layout(L, case.N, case.K, case.D)
    chunk = case.chunk(per)
    final, counts, late = activity(q, xd, case.passes, chunk, start=start)
    assert torch.equal(out, final)
    check_profile(case, counts, chunk)
    rows, _ = pick_rows(case.B, chunk, late, 23)
    got = out.cpu().numpy()
    for r in rows:
        idx = start_np[r]
        for _ in range(case.passes):
            idx = o.refine_trace(x[r], idx)["idx"].astype(np.int64)
        assert np.array_equal(got[r], idx), r


def test_encode_from_host_default_chunk(monkeypatch):
    """encode_from_host's chunks of 32,768 (the last one below the threshold) against encode's single chunk"""
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    case = sg.Case("host_n8_k256", 8, 256, 64, 100000, binds=(sg.S0, sg.P0, sg.L1), multi=(sg.S0, sg.P0, sg.L1))
    q, o, x = setup(case)
    xd = torch.from_numpy(x).cuda()
    for as_bytes in (True, False):
        got = q.encode_from_host(torch.from_numpy(x), 5, as_bytes=as_bytes)
        assert torch.equal(got, q.encode(xd, 5, as_bytes=as_bytes).cpu()), as_bytes
        q.skip_fixed_points = False
        assert torch.equal(got, q.encode(xd, 5, as_bytes=as_bytes).cpu()), as_bytes
        q.skip_fixed_points = True
    _, counts, late = activity(q, xd, 5, 32768)
    check_profile(case, counts, 32768)
    rows, _ = pick_rows(case.B, 32768, late, 29)
    assert np.array_equal(got.numpy()[rows], o.compute_indexes(x[rows], 5).astype(np.int64))


def test_graph_capture_replays_on_other_activity(monkeypatch):
    """a captured skipping encode (its memset and compactions read nact on the device) replayed on frames whose activity
    profile differs from the captured ones"""
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    fx, q, o, xt = _trained()
    B = 20000
    xg = torch.from_numpy(gen.make_gaussian(31, B, fx["D"])).cuda()
    xtr = torch.from_numpy(xt[:B]).cuda()
    _, cg, _ = activity(q, xg, 5, B)
    _, ct, _ = activity(q, xtr, 5, B)
    assert cg[3].sum() > 2 * ct[3].sum() and cg[4].sum() > 2 * ct[4].sum(), (cg.tolist(), ct.tolist())   # two profiles
    assert sg.binds("stage0", B, 8, 256, C)
    static_x = xg.clone()
    want0 = q.encode(static_x, 5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        q.encode(static_x, 5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_codes = q.encode(static_x, 5)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_codes, want0)
    static_x.copy_(xtr)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_codes, q.encode(xtr, 5))
    q.skip_fixed_points = False
    assert torch.equal(static_codes, q.encode(xtr, 5))
    q.skip_fixed_points = True
    static_x.copy_(xg)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_codes, want0)


def test_fp16_and_non_finite_rows_in_a_multi_stride_batch(monkeypatch):
    monkeypatch.delenv("MCQ_SKIP_MIN_BATCH", raising=False)
    case = sg.Case("fp16_n8_k256", 8, 256, 512, 40000, kind="gaussian", binds=(sg.S0, sg.P0, sg.L1),
                   multi=(sg.S0, sg.P0, sg.L1))
    q, o, x = setup(case)
    xh = torch.from_numpy(x).to(torch.float16).cuda()
    for as_bytes in (True, False):
        got, ref = run(q, xh, case, 5, as_bytes, False), run(q, xh, case, 5, as_bytes, True)
        assert torch.equal(got, ref), as_bytes
        assert torch.equal(got, q.encode(xh.float(), 5, as_bytes=as_bytes)), as_bytes
    bad_rows = [3, 7, 9, 11, 17000, 25001, 39998]
    bad = x.copy()
    bad[3] = np.nan
    bad[7, 5] = np.inf
    bad[9] = -np.inf
    bad[11] = 1e30
    bad[17000, 100] = np.nan
    bad[25001] = np.inf
    bad[39998, 511] = -1e30
    check(case, q, o, bad, exclude=np.array(bad_rows))


@pytest.mark.parametrize("N", [8, 16])
def test_separate_kernels_for_16_entry_codebooks(N, tmp_path):
    """MCQ_PASS16=0 (read once per process: a child process) at 65,536 vectors.  With 16 codebooks k_tf_level1 carries the
    level-3 tables (its third range), reached only after the first stride"""
    case = sg.Case(f"p16off_n{N}", N, 16, 48, 65536, binds=(sg.L1,), multi=(sg.L1,))
    seed = 5000 + 7 * N + 16 + 48
    out = str(tmp_path / "codes.npz")
    script = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "from golden import gen\n"
        "from test_gpu_fixed_point_default import load_quantizer\n"
        f"sd = gen.synthetic_state({seed}, 48, 16, {N}); q = load_quantizer(sd, 48, 16, {N})\n"
        f"x = torch.from_numpy(gen.make_kind('make_x', {seed + 1}, 65536, 48)).cuda()\n"
        "r = {}\n"
        "with torch.no_grad():\n"
        "    for ab in (True, False):\n"
        "        r['skip%d' % ab] = q.encode(x, 5, as_bytes=ab).cpu().numpy()\n"
        "        q.skip_fixed_points = False\n"
        "        r['all%d' % ab] = q.encode(x, 5, as_bytes=ab).cpu().numpy()\n"
        "        q.skip_fixed_points = True\n"
        "np.savez(sys.argv[1], **r)\n")
    env = dict(os.environ, MCQ_PASS16="0")
    env.pop("MCQ_SKIP_MIN_BATCH", None)
    r = subprocess.run([sys.executable, "-c", script, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    q, o, x = setup(case)
    xd = torch.from_numpy(x).cuda()
    for ab in (1, 0):
        assert np.array_equal(z[f"skip{ab}"], z[f"all{ab}"]), ab
        assert np.array_equal(z[f"skip{ab}"], q.encode(xd, 5, as_bytes=bool(ab)).cpu().numpy()), ab   # (the LDS-resident pass)
    _, counts, late = activity(q, xd, 5, case.B)
    most = check_profile(case, counts, case.B, pass16=False)
    if N == 16:                    # the level-3 range starts past the first stride at every capped pass
        for p in (4, 5):
            na = int(counts[p - 1][0])
            assert na > 0 and sg.need("level1", na, N, 16) - 16 * na >= sg.grid("level1", case.B, N, 16, C), (p, na, most)
    rows, _ = pick_rows(case.B, case.B, late, 37)
    assert np.array_equal(z["skip0"][rows], o.compute_indexes(x[rows], 5).astype(np.int64))
