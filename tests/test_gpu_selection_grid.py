"""Every cell of the host's kernel-selection tables (quantization_amd/csrc/mcq_api.hip: pick / pick_bool / pick_pair) that the
encode and the register decode can reach at a small shape, launched once and compared with the CPU oracle.

Encode: 130 vectors (a 2-vector tail after the kernels that take 4 per workgroup) of dim 20, 4 passes, int64 output, at every
N x K with N in 1 .. 64, K in 16 .. 1024 (powers of two), N * K <= 4096, and at 32 x 256 and 16 x 512 (Gram matrix 256 MB).
Each cell runs by default -- 130 vectors are below the skipping threshold: every pass on the full grid, STRIDED = false --
and under MCQ_SKIP_MIN_BATCH=0: k_compact after passes 1 - 3, pass 4 on the capped grids, STRIDED = true.  8 x 16 and 16 x 16
(marked *) are k_tf_pass16<8> / <16> in this process and run their separate kernels in a child process under MCQ_PASS16=0
(the hook is read once per process).  Which cell of which table a case reaches (N x K; "mid": not the last combine):

  launch_tf_stage0   k_tf_stage0<K, N, STRIDED>: every N x K with K >= 32, and 1 x 16, 2 x 16; STRIDED in pass 4 of the skipping run
                     k_tf_stage0_k16<N>: 4 x 16, 8 x 16*, 16 x 16*, 32 x 16, 64 x 16
  launch_tf_er       k_tf_er<N, uint8_t>: N x K, K <= 256, N = 1 .. 64; k_tf_er<N, uint16_t>: N x 512, N = 1 .. 16, and N x 1024
  level 0            k_tf_pair0<8, uint8_t>: N x 16, N >= 2; k_tf_pair0s<STRIDED>: N x K, 32 <= K <= 256, N >= 2;
                     k_tf_pair0<16, uint16_t>: N x 512, N x 1024, N >= 2
  level 1            k_tf_pair1<8, 8, uint8_t>: 4 x 16; <16, 16, uint8_t>: 4 x 32 .. 4 x 256; <16, 16, uint16_t>: 4 x 512, 4 x 1024
                     k_tf_level1<8, 8, uint8_t, STRIDED>: 8 x 16*, 16 x 16*, 32 x 16, 64 x 16; <16, 16, uint8_t, STRIDED>: N x K,
                     32 <= K <= 256, N >= 8; <16, 16, uint16_t, STRIDED>: 8 x 512, 16 x 512
  tables             k_tf_table1<8, 8, uint8_t>: 32 x 16, 64 x 16; <16, 16, uint8_t>: N x K, 32 <= K <= 256, N >= 16;
                     <16, 16, uint16_t>: 16 x 512
  launch_tf_up       k_tf_up<8, 16>, <16, 16>: 32 x 16, 64 x 16; <16, 32>: 64 x 16 and N x K, K >= 32, N >= 32; <32, 32>: N x K,
                     K >= 32, N >= 32; <32, 64>: 64 x 32, 64 x 64
  k_tf_comb3         <8, 16, 16, uint8_t>: 16 x 16*; <16, 32, 32, uint8_t>: 16 x 32 .. 16 x 256; <16, 32, 32, uint16_t>: 16 x 512
  launch_tf_comb     k_tf_comb<KH, KC, LAST, CT, STRIDED>; STRIDED with LAST in pass 4 of the skipping run
                     (8, 16)  last 8 x 16*; mid 16 x 16*, 32 x 16, 64 x 16          (16, 16) mid 32 x 16, 64 x 16
                     (16, 32) last 32 x 16, 8 x K (K >= 32; uint16_t: 8 x 512); mid 64 x 16, N x K (K >= 32, N >= 16; uint16_t: 16 x 512)
                     (32, 32) last 64 x 16; mid N x K, K >= 32, N >= 32
                     (32, 64) last 32 x 32 .. 32 x 256; mid 64 x 32, 64 x 64        (64, 64) last 64 x 32, 64 x 64
  launch_pass16      k_tf_pass16<8>: 8 x 16; k_tf_pass16<16>: 16 x 16

Reachable, but not from the cells above: k_tf_gram_terms<N, CT> (batches above 8,192 vectors), k_tf_stage0<K, N> and
k_tf_er<N, CT> at N * K > 4096 other than the two added cells, k_tf_comb<32, 32, mid, uint16_t> and <32, 64, last, uint16_t>
(32 x 512: a 1 GB Gram matrix).  tests/test_gpu_parity.py, test_gpu_fixed_point_default.py and test_gpu_skip_strided.py run those.

Decode: the nine (N, J) shapes of k_decode_reg (kDecRegShapes; J = float4s per lane of a row of round_up16(D) floats) at 5
vectors of one-byte codes, bit for bit against the oracle: dim 20 -> J = 1, dim 300 -> J = 2, dim 1000 -> J = 4.

The other decode dispatchers (the cells are the tables of tests/search_selection_grid.py, which tests/test_search_selection_host.py
checks against the pick<...> lists of the source), all bit for bit against the oracle:

  launch_decode_sliced   k_decode_sliced<T, CH, LPV>: N = 1, 2, 4 (CH 4; 1 and 2 run the `n0 + j < N` tail inside a chunk), 8 (CH 8),
                         16, 32, 64 (CH 16; 32 and 64 run several chunks) x dims 100, 200, 300, 1,000, 1,100 (LPV 4, 8, 16, 32, 64;
                         none a multiple of 16: a last slice reaches into the padding), K = 32, 4,099 vectors, uint8 and int64 codes
  launch_decode_blk      k_decode_blk<4, 2>: 4 x 1,024, <8, 2>: 8 x 512 -- one-byte codes given to a quantizer of wide codebooks
                         (decode accepts any integer dtype and passes bytes through), 4,355 vectors of dim 72 under
                         MCQ_DECODE_LDS_MIN=4096 (read per call), and the same call under MCQ_DECODE_BLK=0.  The other four
                         cells, <4, 4>, <8, 4>, <16, 4> and <16, 2>, are cases of tests/test_gpu_parity.py.
  k_decode<T>            packed digits, 16 x 16: int64 codes of rep = 2, 4, 8 and 16 digits (the top digit below 8: 16^16 does not
                         fit an int64) and uint8 codes of 2, packed least significant digit first, 5 vectors at dim 20 and 300

Reachable, but not from the cells above: k_decode_lds<T> (batches from 16,384 vectors whose 64-byte slices fit the LDS, other
than the block-staged shapes) and the whole-block path of k_decode_blk (a workgroup with at least 16,384 / N vectors);
tests/test_gpu_parity.py runs both.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import search_selection_grid as ss
from golden import gen
from test_gpu_parity import load_quantizer, oracle_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, D, PASSES = 130, 20, 4
KS = (16, 32, 64, 128, 256, 512, 1024)
NS = (1, 2, 4, 8, 16, 32, 64)
CELLS = [(N, K) for K in KS for N in NS if N * K <= 4096] + [(32, 256), (16, 512)]
DECODE_REG = [(8, 2), (8, 1), (4, 1), (4, 2), (4, 4), (16, 1), (16, 2), (2, 1), (2, 2)]     # kDecRegShapes of mcq_api.hip
DIM_OF_J = {1: 20, 2: 300, 4: 1000}


def encode_cell(N, K):
    """the codes of the cell by default and under MCQ_SKIP_MIN_BATCH=0 (read per call), and the oracle's"""
    sd = gen.synthetic_state(1300 + 7 * N + K, D, K, N)
    q = load_quantizer(sd, D, K, N)
    x = gen.make_gaussian(1301 + 7 * N + K, B, D)
    xd = torch.from_numpy(x).cuda()
    old = os.environ.pop("MCQ_SKIP_MIN_BATCH", None)
    try:
        with torch.no_grad():
            dense = q.encode(xd, PASSES, as_bytes=False).cpu().numpy()
            os.environ["MCQ_SKIP_MIN_BATCH"] = "0"
            skipping = q.encode(xd, PASSES, as_bytes=False).cpu().numpy()
    finally:
        os.environ.pop("MCQ_SKIP_MIN_BATCH", None)
        if old is not None:
            os.environ["MCQ_SKIP_MIN_BATCH"] = old
    return dense, skipping, oracle_of(sd).compute_indexes(x, PASSES)


def check_cell(N, K):
    dense, skipping, want = encode_cell(N, K)
    assert dense.dtype == np.int64 and dense.shape == (B, N)
    assert np.array_equal(dense, want), f"{N} x {K}: {int((dense != want).any(axis=1).sum())} vectors differ from the oracle"
    assert np.array_equal(skipping, want), f"{N} x {K}, skipping: {int((skipping != want).any(axis=1).sum())} vectors differ from the oracle"


@pytest.mark.parametrize("N,K", CELLS)
def test_encode_cell_vs_oracle(N, K):
    check_cell(N, K)


def test_sixteen_entry_cells_separate_kernels():
    """8 x 16 and 16 x 16 through the separate kernels: MCQ_PASS16=0, read once per process, so in a fresh one"""
    script = (
        "import sys\n"
        f"sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r})\n"
        "from test_gpu_selection_grid import check_cell\n"
        "check_cell(8, 16); check_cell(16, 16)\n")
    r = subprocess.run([sys.executable, "-c", script], env=dict(os.environ, MCQ_PASS16="0"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("N,J", DECODE_REG)
def test_decode_reg_shape_vs_oracle(N, J):
    K, dim = 16, DIM_OF_J[J]
    assert ((dim + 15) // 16 * 16 // 4 + 63) // 64 == J
    sd = gen.synthetic_state(1700 + 10 * N + J, dim, K, N)
    q = load_quantizer(sd, dim, K, N)
    codes = np.random.RandomState(1701 + 10 * N + J).randint(0, K, size=(5, N)).astype(np.uint8)
    with torch.no_grad():
        got = q.decode(torch.from_numpy(codes).cuda()).cpu().numpy()
    assert np.array_equal(got, oracle_of(sd).decode(codes))


@pytest.mark.parametrize("dim", sorted(ss.SLICED_DIMS))
@pytest.mark.parametrize("N", ss.SLICED_NS)
def test_decode_sliced_cell_vs_oracle(N, dim):
    K, B, lpv = ss.SLICED_K, ss.SLICED_B, ss.SLICED_DIMS[dim]
    Dp = (dim + 15) // 16 * 16
    assert ss.decode_sliced_lpv(dim) == lpv and 8 * lpv * 4 >= Dp and (lpv == 4 or 8 * (lpv // 2) * 4 < Dp) and dim % 16
    sd = gen.synthetic_state(1900 + 10 * N + lpv, dim, K, N)
    q = load_quantizer(sd, dim, K, N)
    codes = np.random.RandomState(1901 + 10 * N + lpv).randint(0, K, size=(B, N)).astype(np.uint8)
    want = oracle_of(sd).decode(codes)
    with torch.no_grad():
        got8 = q.decode(torch.from_numpy(codes).cuda())
        got64 = q.decode(torch.from_numpy(codes.astype(np.int64)).cuda())
    assert got8.dtype == torch.float32 and tuple(got8.shape) == (B, dim)
    assert np.array_equal(got8.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{N} x {K}, dim {dim}: uint8 codes differ from the oracle"
    assert np.array_equal(got64.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{N} x {K}, dim {dim}: int64 codes differ from the oracle"
    assert torch.equal(got8, got64)


def _with_env(name, value, f):
    """f() under a per-call hook of the library, the hook restored afterwards"""
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return f()
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


@pytest.mark.parametrize("N,K", sorted(ss.BLK_CELLS))
def test_decode_blk_narrow_slices_of_wide_codebooks_vs_oracle(N, K):
    B, dim = ss.BLK_B, ss.BLK_D
    assert ss.BLK_CELLS[(N, K)] == (N, 2) and ss.decode_blk_lpv(N, K) == 2 and B >= ss.BLK_LDS_MIN and dim % 4 == 0
    sd = gen.synthetic_state(2100 + N, dim, K, N)
    q = load_quantizer(sd, dim, K, N)
    codes = np.random.RandomState(2101 + N).randint(0, 256, size=(B, N)).astype(np.uint8)      # indexes below 256 of K entries
    cd = torch.from_numpy(codes).cuda()
    want = oracle_of(sd).decode(codes)
    with torch.no_grad():
        got = _with_env("MCQ_DECODE_LDS_MIN", str(ss.BLK_LDS_MIN), lambda: q.decode(cd))
        other = _with_env("MCQ_DECODE_LDS_MIN", str(ss.BLK_LDS_MIN), lambda: _with_env("MCQ_DECODE_BLK", "0", lambda: q.decode(cd)))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"{N} x {K}: k_decode_blk differs from the oracle"
    assert torch.equal(other, got)


@pytest.mark.parametrize("dim", ss.PACKED_DIMS)
def test_decode_of_packed_digits_vs_oracle(dim):
    N, K, B = ss.PACKED_N, ss.PACKED_K, ss.PACKED_B
    sd = gen.synthetic_state(2300 + dim, dim, K, N)
    q = load_quantizer(sd, dim, K, N)
    idx = np.random.RandomState(2301 + dim).randint(0, K, size=(B, N))
    idx[:, N - 1] %= 8                                       # the top digit of a code of 16 digits stays below 8
    idx[0] = K - 1                                           # the largest digits everywhere ...
    idx[0, N - 1] = 7                                        # ... that still fit
    want = oracle_of(sd).decode(idx.astype(np.uint8))
    for rep, dtype in ss.PACKED_REPS:
        packed = ss.pack_digits(idx, rep, K, np.dtype(dtype))
        assert packed.shape == (B, N // rep)
        with torch.no_grad():
            got = q.decode(torch.from_numpy(packed).cuda())
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)), f"rep {rep}, {dtype} codes, dim {dim}"
