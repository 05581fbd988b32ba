"""Host mirror of the grid arithmetic of fixed-point skipping (quantization_amd/csrc/mcq_api.hip, mcq_tf_kernels.h), and the
case table of tests/test_gpu_skip_strided.py.

From the fourth pass of a skipping encode on, four pass kernels run a capped grid of at most kCapStage0 (k_tf_stage0) or
kCapWave (k_tf_pair0s, k_tf_level1, the last k_tf_comb) workgroups that stride over the virtual workgroups of the `nact`
active vectors.  The strided code differs from the plain grid only when the full grid exceeds the cap ("binds"), and loops
more than once only when the active part does too ("multi-stride").  The constants are read from the driver's source, so
that a moved cap makes tests/test_skip_grid_host.py fail instead of leaving the GPU cases covering nothing."""
import os
import re
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "quantization_amd", "csrc", "mcq_api.hip")

KERNELS = ("stage0", "pair0s", "level1", "root_comb")


def constants(path=API):
    """kCapStage0, kCapWave, the default of skip_min_batch() and the upper bound of default_chunk(), from the source"""
    with open(path) as f:
        src = f.read()
    caps = re.search(r"constexpr\s+unsigned\s+kCapStage0\s*=\s*(\d+)\s*,\s*kCapWave\s*=\s*(\d+)\s*;", src)
    smb = re.search(r"inline\s+long\s+skip_min_batch\(\)\s*\{[^}]*?return\s+v\s*\?\s*atol\(v\)\s*:\s*(\d+)\s*;", src, re.S)
    dch = re.search(r"long\s+default_chunk\(int N, int K, int D\)\s*\{[^}]*?c\s*=\s*c\s*>\s*(\d+)\s*\?\s*(\d+)\s*:\s*c;", src, re.S)
    assert caps and smb and dch, "the grid constants of mcq_api.hip moved: update tests/skip_grid.py"
    assert dch.group(1) == dch.group(2)
    return dict(cap_stage0=int(caps.group(1)), cap_wave=int(caps.group(2)), skip_min_batch=int(smb.group(1)),
                default_chunk_max=int(dch.group(1)))


# ------------------------------------------------------------------ workspace and chunks (run_encode_t)
def ws_layout(L, N, K, D):
    """(bytes per vector, slack) of the encode workspace, from mcq_encode_workspace_bytes (linear in the chunk)"""
    w1, w2 = L.mcq_encode_workspace_bytes(1, N, K, D), L.mcq_encode_workspace_bytes(2, N, K, D)
    return w2 - w1, 2 * w1 - w2


def default_chunk(per, chunk_max=65536):
    """default_chunk(): 65,536 vectors, fewer when the workspace of a chunk would pass 2 GB; a multiple of 128"""
    c = min((2 << 30) // per, chunk_max)
    return max(c, 1024) & ~127


def ws_bytes(L, N, K, D, vectors):
    """a caller-sized workspace that holds exactly `vectors` vectors (mcq_encode_workspace_bytes stops at default_chunk)"""
    per, slack = ws_layout(L, N, K, D)
    return slack + per * vectors


def chunk_of(B, ws_vectors):
    """the chunk run_encode_t cuts a batch of B into, for a workspace of ws_vectors vectors"""
    chunk = min(ws_vectors, B)
    if chunk < B:
        assert chunk >= 128
        chunk &= ~127
    return chunk


def chunks(B, chunk):
    return [(lo, min(chunk, B - lo)) for lo in range(0, B, chunk)]


# ------------------------------------------------------------------ which kernels run capped, and their grids
def skips(Bc, N, K, passes, skip_min_batch, pass16=True):
    """does run_encode_t take the skipping path for this chunk (u8 / int64 output alike)"""
    use_p16 = pass16 and K == 16 and N in (8, 16)
    return passes >= 3 and not use_p16 and Bc >= skip_min_batch


def capped_kernels(N, K):
    """the launches that take the capped form at this shape (run_tf_combines, launch_tf_stage0)"""
    out = []
    if not (K == 16 and N >= 4):                 # (16-entry codebooks, four or more: k_tf_stage0_k16, never capped)
        out.append("stage0")
    if 16 < K <= 256 and N >= 2:                 # (one-byte entries in lists of 16: k_tf_pair0s)
        out.append("pair0s")
    if N >= 8:
        out.append("level1")
    if N >= 8 and N != 16:                       # (16 codebooks end in k_tf_comb3)
        out.append("root_comb")
    return out


def _r8(v):
    return (v + 7) & ~7


def full_grid(kernel, Bc, N, K):
    """the workgroups of the plain launch (the virtual grid of the capped one)"""
    if kernel == "stage0":
        return (Bc + 3) // 4 * N
    if kernel == "pair0s":
        return Bc * (N >> 1)
    if kernel == "level1":
        l3 = 16 if (N == 16 and K == 16) else 0
        return Bc * (N // 4) + Bc * (N >> 3) * 4 + Bc * l3
    if kernel == "root_comb":
        return Bc
    raise ValueError(kernel)


def cap_of(kernel, c):
    return c["cap_stage0"] if kernel == "stage0" else c["cap_wave"]


def grid(kernel, Bc, N, K, c):
    """pass_grid(full, true, cap)"""
    full = full_grid(kernel, Bc, N, K)
    return min(full, cap_of(kernel, c))


def need(kernel, nact, N, K):
    """the virtual workgroups a capped launch walks for nact active vectors (the kernels' `need` / r0 + r1 + r2)"""
    if kernel == "stage0":
        return (nact + 3) // 4 * N
    if kernel == "pair0s":
        return nact * (N >> 1)
    if kernel == "level1":
        l3 = 16 if (N == 16 and K == 16) else 0
        return _r8(nact * (N // 4)) + _r8(nact * (N >> 3) * 4) + nact * l3
    if kernel == "root_comb":
        return nact
    raise ValueError(kernel)


def binds(kernel, Bc, N, K, c):
    return full_grid(kernel, Bc, N, K) > cap_of(kernel, c)


def strides(kernel, nact, Bc, N, K, c):
    """iterations of the strided loop for its first workgroup"""
    g = grid(kernel, Bc, N, K, c)
    return -(-need(kernel, nact, N, K) // g) if g else 0


# ------------------------------------------------------------------ the GPU cases
@dataclass(frozen=True)
class Case:
    """one batch through the skipping path.  ws: vectors of a caller-sized workspace (None: Quantizer.encode's own);
    binds: the capped kernels whose cap must bind at pass >= 4; multi: those whose strided loop must go round at least
    twice there (asserted from the measured activity on the GPU)"""
    name: str
    N: int
    K: int
    D: int
    B: int
    passes: int = 5
    ws: int = None
    kind: str = "make_x"
    binds: tuple = ()
    multi: tuple = ()
    skip_min_batch: int = None                   # MCQ_SKIP_MIN_BATCH (monkeypatch); None: the default
    note: str = field(default="", compare=False)

    def chunk(self, per):
        if self.ws is not None:
            return chunk_of(self.B, self.ws)
        return min(self.B, default_chunk(per))


S0, P0, L1, RC = KERNELS
SHAPES = [
    Case("n4_k16", 4, 16, 40, 65536, binds=(), note="no capped kernel: stage 0 is k_tf_stage0_k16, levels 0 / 1 the plain "
         "k_tf_pair0 / k_tf_pair1; the case checks compaction and the emit at this shape"),
    Case("n4_k64", 4, 64, 72, 262144, ws=262144, binds=(S0, P0), multi=(S0, P0)),
    Case("n4_k256", 4, 256, 64, 98304, ws=98304, binds=(S0, P0), multi=(S0, P0)),
    Case("n8_k32", 8, 32, 56, 40000, binds=(S0, P0, L1), multi=(S0, P0, L1)),
    Case("n8_k128", 8, 128, 100, 30000, kind="gaussian", binds=(S0, P0, L1), multi=(S0, P0, L1)),
    Case("n8_k512", 8, 512, 64, 20000, binds=(S0, L1), multi=(S0, L1)),
    Case("n8_k1024", 8, 1024, 48, 20000, binds=(S0, L1), multi=(S0, L1)),
    Case("n16_k512", 16, 512, 64, 12000, binds=(S0, L1), multi=(S0, L1)),
    Case("n32_k16", 32, 16, 64, 10000, binds=(L1,), multi=(L1,)),
    Case("n32_k256", 32, 256, 128, 11000, binds=(S0, P0, L1), multi=(S0, P0, L1)),
    Case("n64_k16", 64, 16, 64, 10000, binds=(L1,), multi=(L1,)),
    Case("n64_k256", 64, 256, 256, 4000, skip_min_batch=0, binds=(S0, P0, L1), multi=(S0, P0, L1),
         note="Quantizer's chunk here is 3,200 vectors (2 GB of workspace), below the default threshold"),
]
# chunks beyond Quantizer's 65,536, through a caller's workspace
BIG = [
    Case("n1_big", 1, 256, 40, 262144, ws=262144, binds=(S0,), note="one codebook converges within two passes: at pass 4 "
         "the capped stage 0 finds (almost) no active vector, so it can only show a binding cap"),
    Case("n2_big", 2, 256, 64, 262144, ws=262144, binds=(S0, P0)),
    Case("n32_k16_root", 32, 16, 64, 73000, ws=69632, binds=(L1, RC), multi=(L1, RC),
         note="the root combine loops twice past 65,536 active vectors of a chunk: 32 x 16 codebooks hold nearly every "
         "vector through pass 5; a tail of 3,368 below the threshold"),
    Case("n32_mixed_8064", 32, 256, 128, 21384, ws=8064, binds=(), note="every chunk below the threshold: all passes"),
    Case("n32_mixed_8192", 32, 256, 128, 21384, ws=8192, binds=(S0, P0, L1), multi=(S0, P0, L1),
         note="two chunks at the threshold, a ragged tail of 5,000 below it"),
]
PASSES = [Case(f"n8_k128_p{p}", 8, 128, 100, 30000, passes=p, kind="gaussian",
               binds=() if p == 3 else (S0, P0, L1), multi=() if p == 3 else (S0, P0, L1),
               note="three passes: no capped pass" if p == 3 else "") for p in (3, 4, 6, 12, 60)]
THRESHOLD = [Case(f"n16_k256_b{b}", 16, 256, 48, b, kind="gaussian", binds=(S0,) if b > 8192 else (),
                  note="stage 0's full grid passes its cap at 8,193 vectors") for b in (8191, 8192, 8193)] + [
    Case("n32_k256_default_tail", 32, 256, 128, 16392, binds=(S0, P0, L1), multi=(S0, P0, L1),
         note="Quantizer's chunk of 11,392 vectors, then a tail of 5,000 below the threshold"),
]
ALL = SHAPES + BIG + PASSES + THRESHOLD
