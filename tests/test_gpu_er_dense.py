"""E / R of a refinement pass from the dense pair of kernels (k_tf_gram_terms<N, CT, true> + k_tf_er<N, CT, true>, the form of
chunks above 8,192 vectors of 4, 8 or 16 codebooks) against the one-launch form and against the oracle, through the probe
mcq_test_er of include/mcq_probe.h, which runs the launcher the encode uses (form 0: one launch, form 1: the pair).

  bit equality   E and R of form 1 equal form 0 as uint32, for batches over the edges of a wave's 64 / N vectors, of the four-wave
                 workgroup of the sums and (1,000) of the 256-vector workgroup of the Gram terms; codes random, all 0, all
                 K - 1 and one row repeated
  oracle         32 rows per shape: OracleQuantizer.refine_trace(x, idx)["E"] / ["R"], bit for bit; x.C and |x|^2 are the
                 device's own (mcq_test_xc_xx: the limb kernel and the x.C product of an encode)
  skipping form  nact = B - 3 with a permutation as map: slots >= nact keep the sentinel the test wrote, the others equal the
                 one-launch form, and the same rows asked for without a map
  symmetry       the dense kernels gather each unordered pair once: G of each state equals its transpose bit for bit
  end to end     8 x 256, 8,320 vectors (above both the skipping and the one-launch threshold): MCQ_ER_DENSE_MIN=0 against
                 10**9, with skipping and with MCQ_ENCODE_ALL_PASSES, byte-equal codes; the launch counts of the dense path:
                 1 limb conversion + 2 screened logits + 1 x.C + 5 x (2 E / R + 4 pass kernels) = 34, with skipping one
                 k_zero_counts and four k_compact more = 39.  At 256 vectors the hook at 0 takes the same host path, where the
                 one launch serves every pass: 1 + 2 + 1 + 5 x (1 + 4) = 29, and 34 with skipping."""
import ctypes

import numpy as np
import pytest
import torch

from golden import gen

pytestmark = pytest.mark.gpu

D = 32
SHAPES = [(4, 64), (8, 256), (16, 32)]
BMAX = 1000
ORDER = ("C", "Q", "Cf", "Ce", "Wf", "We", "wmu", "bias", "scales", "mean", "cmean", "G", "total")
SENTINEL = np.float32(-12345.5)


def _L():
    from quantization_amd import _lib
    return _lib.lib()


def _st():
    return torch.cuda.current_stream().cuda_stream


def batches(N):
    vw = 64 // N
    return sorted({1, vw - 1, vw, vw + 1, 4 * vw - 1, 4 * vw, 4 * vw + 1, BMAX} - {0})


def test_batches_are_the_edges():
    assert batches(8) == [1, 7, 8, 9, 31, 32, 33, 1000]
    assert batches(16) == [1, 3, 4, 5, 15, 16, 17, 1000] and batches(4) == [1, 15, 16, 17, 63, 64, 65, 1000]


def _quantizer(N, K):
    from quantization_amd import Quantizer
    state = gen.synthetic_state(2400 + N + K, D, K, N)
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for k, v in state.items():
        sd[k] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    return state, q.to("cuda:0")


_CACHE = {}


def _case(N, K):
    """per shape, once: the prepared blob, BMAX frames, their x.C and |x|^2 from the device, random codes"""
    if (N, K) in _CACHE:
        return _CACHE[(N, K)]
    L = _L()
    with torch.no_grad():
        state, q = _quantizer(N, K)
        blob = q._prepared()
    x = gen.make_x(2401 + N + K, BMAX, D)
    xd = torch.from_numpy(x).cuda()
    xc = torch.empty((BMAX, N * K), dtype=torch.float32, device="cuda:0")
    xx = torch.empty(BMAX, dtype=torch.float32, device="cuda:0")
    nws = L.mcq_logits_workspace_bytes(BMAX, N, D)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
    rc = L.mcq_test_xc_xx(xd.data_ptr(), BMAX, blob.data_ptr(), N, K, D, xc.data_ptr(), xx.data_ptr(), ws.data_ptr(), nws, _st(), 0)
    assert rc == 0, rc
    torch.cuda.synchronize()
    codes = np.random.RandomState(2402 + N + K).randint(0, K, size=(BMAX, N)).astype(np.uint8)
    c = dict(state=state, q=q, blob=blob, x=x, xc=xc, xx=xx, codes=codes)
    _CACHE[(N, K)] = c
    return c


def _er(c, N, K, idx, B, form, xc=None, xx=None, nact=None, map_=None):
    """E, R of the first B slots as uint32 arrays; the outputs start as SENTINEL"""
    L = _L()
    idx_d = torch.from_numpy(np.ascontiguousarray(idx[:B])).cuda()
    E = torch.full((B,), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    R = torch.full((B, N), float(SENTINEL), dtype=torch.float32, device="cuda:0")
    nws = L.mcq_test_er_workspace_bytes(B, N)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
    assert idx_d.data_ptr() % 16 == 0 and ws.data_ptr() % 256 == 0
    nact_d = None if nact is None else torch.tensor([nact], dtype=torch.int32, device="cuda:0")
    map_d = None if map_ is None else torch.from_numpy(np.ascontiguousarray(map_, dtype=np.int32)).cuda()
    xc = c["xc"] if xc is None else xc
    xx = c["xx"] if xx is None else xx
    rc = L.mcq_test_er(c["blob"].data_ptr(), N, K, D, xc.data_ptr(), xx.data_ptr(), idx_d.data_ptr(), B,
                       None if nact_d is None else nact_d.data_ptr(), None if map_d is None else map_d.data_ptr(), form,
                       E.data_ptr(), R.data_ptr(), ws.data_ptr(), nws, _st())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return E.cpu().numpy().view(np.uint32), R.cpu().numpy().view(np.uint32)


def _pattern(c, K, name):
    codes = c["codes"]
    if name == "random":
        return codes
    if name == "zeros":
        return np.zeros_like(codes)
    if name == "last":
        return np.full_like(codes, K - 1)
    assert name == "one_row"
    return np.repeat(codes[5:6], codes.shape[0], axis=0)


@pytest.mark.parametrize("pattern", ["random", "zeros", "last", "one_row"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_dense_pair_equals_one_launch(N, K, pattern):
    c = _case(N, K)
    idx = _pattern(c, K, pattern)
    for B in batches(N):
        E0, R0 = _er(c, N, K, idx, B, 0)
        E1, R1 = _er(c, N, K, idx, B, 1)
        sent = SENTINEL.view(np.uint32)
        assert not (E0 == sent).any() and not (R0 == sent).any()          # every slot was written
        assert np.array_equal(E1, E0), (N, K, pattern, B, int((E1 != E0).sum()))
        assert np.array_equal(R1, R0), (N, K, pattern, B, int((R1 != R0).sum()))


@pytest.mark.parametrize("N,K", SHAPES)
def test_dense_pair_equals_oracle(N, K):
    from oracle.oracle import OracleQuantizer
    c = _case(N, K)
    sd = c["state"]
    o = OracleQuantizer(sd["centers"], float(sd["centers_scale"]), sd["to_logits.weight"], sd["to_logits.bias"],
                        float(sd["logits_scale"]))
    B = 32
    want_E, want_R = np.empty(B, np.float32), np.empty((B, N), np.float32)
    for b in range(B):
        t = o.refine_trace(c["x"][b], c["codes"][b])
        want_E[b], want_R[b] = t["E"][0], t["R"]
    for form in (1, 0):
        E, R = _er(c, N, K, c["codes"], B, form)
        assert np.array_equal(E, want_E.view(np.uint32)), (N, K, form)
        assert np.array_equal(R, want_R.view(np.uint32)), (N, K, form)


@pytest.mark.parametrize("N,K", SHAPES)
def test_skipping_form(N, K):
    """packed slots: slot s holds row map[s] of x.C / |x|^2, and only *nact slots are in use"""
    c = _case(N, K)
    sent = SENTINEL.view(np.uint32)
    for B in (4 * (64 // N) + 3, BMAX):
        nact = B - 3
        perm = np.random.RandomState(7 + B).permutation(B).astype(np.int32)
        idx = c["codes"]
        E0, R0 = _er(c, N, K, idx, B, 0, nact=nact, map_=perm)
        E1, R1 = _er(c, N, K, idx, B, 1, nact=nact, map_=perm)
        assert (E1[nact:] == sent).all() and (R1[nact:] == sent).all() and (E0[nact:] == sent).all() and (R0[nact:] == sent).all()
        assert not (E1[:nact] == sent).any() and not (R1[:nact] == sent).any()
        assert np.array_equal(E1, E0) and np.array_equal(R1, R0)
        # the same rows without a map: x.C and |x|^2 gathered by the test
        pd = torch.from_numpy(perm.astype(np.int64)).cuda()
        Ep, Rp = _er(c, N, K, idx, B, 1, xc=c["xc"][:B][pd].contiguous(), xx=c["xx"][:B][pd].contiguous())
        assert np.array_equal(E1[:nact], Ep[:nact]) and np.array_equal(R1[:nact], Rp[:nact])


@pytest.mark.parametrize("N,K", SHAPES)
def test_gram_matrix_is_symmetric(N, K):
    L = _L()
    c = _case(N, K)
    off = (ctypes.c_size_t * len(ORDER))()
    assert L.mcq_test_prepared_layout(N, K, D, off, len(ORDER)) == len(ORDER)
    off = dict(zip(ORDER, list(off)))
    nk = N * K
    G = c["blob"].view(torch.uint8)[off["G"]:off["G"] + 4 * nk * nk].cpu().numpy().view(np.uint32).reshape(nk, nk)
    assert np.array_equal(G, G.T)
    assert (G != 0).any()


# ---------------------------------------------------------------------------------------------------------- end to end
def _encode(L, q, x, iters, flags):
    B, N, K = x.shape[0], q.num_codebooks, q.codebook_size
    blob, ls = q._prepared(), q._lscale_exp
    nws = L.mcq_encode_workspace_bytes(B, N, K, D)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
    out = torch.zeros((B, N), dtype=torch.uint8, device="cuda:0")
    rc = L.mcq_encode_ex(x.data_ptr(), B, blob.data_ptr(), ls, N, K, D, iters, out.data_ptr(), None, ws.data_ptr(), nws, _st(), flags)
    n = L.mcq_last_encode_launches()
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), n


@pytest.mark.parametrize("B,skip_env,want", [(8320, None, {"dense": (39, 34), "emit": (31, 26)}),
                                             (256, "0", {"dense": (34, 29), "emit": (30, 25)})])
def test_encode_dense_path_end_to_end(B, skip_env, want, monkeypatch):
    """want: launches (with skipping, with MCQ_ENCODE_ALL_PASSES) on the dense path and with E / R in the emitting wave.  The
    latter by reading: 1 + 2 + 1, E / R ahead of the first pass (2 launches above 8,192 vectors, else 1), 5 x 4 pass kernels;
    skipping adds k_zero_counts and four k_compact"""
    from quantization_amd import _lib
    L = _L()
    N, K = 8, 256
    with torch.no_grad():
        _, q = _quantizer(N, K)
        x = torch.from_numpy(gen.make_x(2410, B, D)).cuda()
        if skip_env is not None:
            monkeypatch.setenv("MCQ_SKIP_MIN_BATCH", skip_env)
        got = {}
        for path, env in (("dense", "0"), ("emit", str(10 ** 9))):
            monkeypatch.setenv("MCQ_ER_DENSE_MIN", env)
            codes_skip, n_skip = _encode(L, q, x, 5, 0)
            codes_all, n_all = _encode(L, q, x, 5, _lib.MCQ_ENCODE_ALL_PASSES)
            print(f"ER DENSE END TO END B={B} {path}: launches {n_skip} with skipping, {n_all} without")
            got[path] = (codes_skip, codes_all, (n_skip, n_all))
    assert np.array_equal(got["dense"][0], got["emit"][0]) and np.array_equal(got["dense"][1], got["emit"][1])
    assert np.array_equal(got["dense"][0], got["dense"][1])
    assert got["dense"][2] == want["dense"] and got["emit"][2] == want["emit"]
