"""The looping (STRIDED) forms of the capped pass kernels where a workgroup goes round many times, and the rule that picks them.

MCQ_PASS_CAP_WAVE / MCQ_PASS_CAP_STAGE0 = 8 make eight workgroups walk every virtual workgroup of the active vectors: at 259
slots a workgroup of k_tf_pair0s loops 130 times, at 1 slot once (or not at all: nact = 0).  k_tf_pair0s, k_tf_pair1 and k_tf_comb
read their arguments and their lane number afresh every iteration (mcq_tf_kernels.h, tf_fresh_args / tf_fresh_lane), k_tf_stage0,
k_tf_table1 and k_tf_level1 hold them across the loop; what each computes is the dense body.

  one pass, list by list   mcq_test_pass with MCQ_TEST_PASS_CAPPED under caps of 8, dim 32, 8 x 256, 16 x 256, 8 x 32, 8 x 64 -- with
                           k_tf_level1 and, under MCQ_LAZY_TABLES_MIN=0, with k_tf_pair1 + the masked k_tf_table1 --, 1 / 5 / 67 / 259
                           slots of which 0 / 1 / 64 / 258 are active, under a permutation, three passes on the plain, tie and
                           degenerate states of tests/pass_lists.py.  Per pass: E, R, every list of every level and the codes of the
                           active slots equal the ORACLE's (pass_lists.lists_of), the whole workspace equals, byte for byte, that of
                           the same call through the plain launchers (dense kernels), slots past nact keep the 0xA5 they were
                           filled with, and so does every byte between and past the arrays
  end to end               8,320 vectors, dim 32, 8 x 256, five passes of a skipping encode under caps of 8 and under the default
                           caps: codes equal MCQ_ENCODE_ALL_PASSES and the oracle on 64 rows, same number of launches either way
  rule 2                   33,024 vectors on one lane, default caps: k_tf_stage0 and k_tf_pair1 loop (66,048 virtual workgroups
                           against caps of 32,768 / 65,536), the last k_tf_comb (33,024) takes the dense form; codes equal the
                           all-passes run"""
import numpy as np
import pytest
import torch

import pass_lists as pl
from golden import gen
from test_gpu_fixed_point_default import both, load_quantizer, oracle_of
from test_gpu_pass_lists import CAPPED, FILL, _L, _workspace, arrays_of, assert_nothing_else_written, run_pass

pytestmark = pytest.mark.gpu

D = pl.D
SLOTS = ((1, 0), (5, 1), (67, 64), (259, 258))          # (slots, active slots)
BMAX = max(b for b, _ in SLOTS)
SHAPES = [(8, 256), (16, 256), (8, 32), (8, 64)]
UNUSED = ("idxB", "idxC", "final_idx", "map0", "map1", "cnt", "gterms")


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


_REF = {}


def reference(N, K, name):
    """pass_lists.reference for BMAX vectors: the state, the frames, the start codes and the oracle's lists of pl.PASSES passes,
    once per (shape, state); vectors are independent, so a smaller batch is a prefix"""
    key = (N, K, name)
    if key not in _REF:
        sd = pl.make_state(name, N, K)
        x = pl.make_frames(name, N, K, BMAX)
        o = pl.oracle_of(sd)
        start = o.compute_indexes(x, 0).astype(np.uint16)
        idx, passes = start.copy(), []
        for _ in range(pl.PASSES):
            per = []
            for b in range(BMAX):
                t = o.refine_trace(x[b], idx[b])
                per.append(pl.lists_of(t, N, K))
                idx[b] = t["idx"]
            stacked = {k: np.stack([w[k] for w in per]) for k in per[0]}
            stacked["E"] = stacked["E"].reshape(BMAX)
            passes.append(stacked)
        q = load_quantizer(sd, D, K, N)
        _REF[key] = dict(x=x, start=start, passes=passes, q=q, blob=q._prepared())
    return _REF[key]


@pytest.mark.parametrize("name", pl.STATES)
@pytest.mark.parametrize("lazy", [False, True], ids=["level1", "pair1_table1"])
@pytest.mark.parametrize("N,K", SHAPES)
def test_looping_pass_equals_oracle_and_dense(N, K, lazy, name, monkeypatch):
    monkeypatch.setenv("MCQ_PASS_CAP_WAVE", "8")
    monkeypatch.setenv("MCQ_PASS_CAP_STAGE0", "8")
    monkeypatch.setenv("MCQ_LAZY_TABLES_MIN", "0" if lazy else str(1 << 40))
    L = _L()
    ref = reference(N, K, name)
    for B, nact in SLOTS:
        lay, ws = pl.layout(L, B, N, K), _workspace(L, B, N, K)
        perm = np.random.RandomState(41 + N + K + B).permutation(B).astype(np.int32)
        x = ref["x"][:B]
        idx = ref["start"][:B].astype(np.int64)
        for p in range(pl.PASSES):
            want = ref["passes"][p]
            what = (N, K, name, lazy, B, nact, f"pass {p}")
            raw_d, out_d, n_d = run_pass(L, ref["blob"], x, idx[perm], N, K, ws, nact=nact, map_=perm)
            raw_c, out_c, n_c = run_pass(L, ref["blob"], x, idx[perm], N, K, ws, nact=nact, map_=perm, flags=CAPPED)
            got = arrays_of(raw_c, lay, B, N)
            act = perm[:nact]
            for a in sorted(got):
                w = want[a][:B][act]
                bad = np.argwhere(got[a][:nact] != w)
                assert bad.size == 0, what + (a, f"{len(bad)} of {w.size} differ from the oracle, first at {bad[0].tolist()}")
                if a == "idx":          # (imported for every slot, refined in the active ones)
                    assert np.array_equal(got[a][nact:], idx[perm[nact:]].astype(got[a].dtype)), what
                else:
                    tail = np.ascontiguousarray(got[a][nact:]).view(np.uint8)
                    assert (tail == FILL).all(), what + (a, "a slot past nact was written")
            assert np.array_equal(out_c[act], want["idx"][:B][act].astype(np.int64)) and (out_c[perm[nact:]] == -7).all(), what
            assert_nothing_else_written(raw_c, lay, what, UNUSED)
            diff = np.flatnonzero(raw_c != raw_d)
            assert diff.size == 0, what + (f"{diff.size} bytes of the workspace differ from the plain launchers', first at {diff[:1]}",)
            assert np.array_equal(out_c, out_d) and n_c == n_d, what + (n_c, n_d)
            nxt = idx.copy()
            nxt[act] = want["idx"][:B][act]
            idx = nxt


def _setup(B, seed):
    N, K = 8, 256
    sd = gen.synthetic_state(seed, D, K, N)
    x = gen.make_gaussian(seed + 1, B, D)
    return sd, load_quantizer(sd, D, K, N), x, torch.from_numpy(x).cuda()


def test_skipping_encode_under_tiny_and_default_caps(monkeypatch):
    B = 8320                                             # (a skipping chunk: at least 8,192 vectors)
    for v in ("MCQ_SKIP_MIN_BATCH", "MCQ_LAZY_TABLES_MIN", "MCQ_ENCODE_LANES", "MCQ_ENCODE_LANES_MIN"):
        monkeypatch.delenv(v, raising=False)
    sd, q, x, xd = _setup(B, 7100)
    L = _L()
    codes, launches = {}, {}
    for cap in ("8", None):
        for v in ("MCQ_PASS_CAP_WAVE", "MCQ_PASS_CAP_STAGE0"):
            if cap is None:
                monkeypatch.delenv(v, raising=False)
            else:
                monkeypatch.setenv(v, cap)
        got = q.encode(xd, 5, as_bytes=False)
        launches[cap] = L.mcq_last_encode_launches()
        _, ref = both(q, xd, 5)
        assert torch.equal(got, ref), (cap, int((got != ref).any(dim=1).sum()))
        codes[cap] = got.cpu().numpy()
    assert np.array_equal(codes["8"], codes[None])
    assert launches["8"] == launches[None], launches
    rows = np.random.RandomState(5).choice(B, 64, replace=False)
    assert np.array_equal(codes["8"][rows], oracle_of(sd).compute_indexes(x[rows], 5).astype(np.int64))


def test_dense_form_where_the_grid_fits_the_cap(monkeypatch):
    B = 33024
    for v in ("MCQ_SKIP_MIN_BATCH", "MCQ_LAZY_TABLES_MIN", "MCQ_ENCODE_LANES_MIN", "MCQ_PASS_CAP_WAVE", "MCQ_PASS_CAP_STAGE0"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("MCQ_ENCODE_LANES", "1")
    _, q, _, xd = _setup(B, 7200)
    got, ref = both(q, xd, 5)
    assert torch.equal(got, ref), int((got != ref).any(dim=1).sum())
