"""Host-side checks of the two-lane chunk plan (include/mcq_lanes.h; no GPU): mcq_test_chunk_plan reports the plan the encode
takes, mcq_test_pass_layout where carve() puts a chunk.  The two lanes' extents are disjoint and inside the workspace the library
asks for, for every shape of tests/test_gpu_two_lanes.py and for 32 and 64 codebooks; the chunks of a plan tile the batch in order,
alternate between the lanes, none is empty, and the rounding is the one-lane rule applied per lane; the one-lane plan is the
chunking the library always had; the hooks decide as documented; the argument checks answer in the documented order."""
import ctypes

import pytest

import skip_grid as sg

HEAD = 6
SHAPES = [(8, 256, 64), (4, 256, 64), (16, 256, 64), (16, 16, 64), (4, 512, 32), (8, 256, 512), (32, 256, 64), (64, 256, 48),
          (64, 16, 64), (32, 512, 32), (1, 256, 40), (2, 1024, 24)]
LAYOUT_VALUES = 64


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    L = _lib.lib()
    L.mcq_test_chunk_plan.restype = ctypes.c_int
    L.mcq_test_chunk_plan.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_long), ctypes.c_int]
    return _lib, L


def plan(L, B, N, K, D, ws, lanes):
    head = (ctypes.c_long * HEAD)()
    rc = L.mcq_test_chunk_plan(B, N, K, D, ws, lanes, head, HEAD)
    if rc != HEAD:
        return rc
    n = head[2]
    cap = HEAD + 3 * n
    out = (ctypes.c_long * cap)()
    assert L.mcq_test_chunk_plan(B, N, K, D, ws, lanes, out, cap) == HEAD and tuple(out[:HEAD]) == tuple(head)
    return dict(lanes=out[0], chunk=out[1], n=n, off=(out[3], out[4]), lane_bytes=out[5],
                chunks=[tuple(out[HEAD + 3 * i:HEAD + 3 * i + 3]) for i in range(n)])


def carve_total(L, B, N, K, D):
    out = (ctypes.c_size_t * LAYOUT_VALUES)()
    assert L.mcq_test_pass_layout(B, N, K, D, out, LAYOUT_VALUES) == LAYOUT_VALUES
    return out[LAYOUT_VALUES - 1]


def check_tiling(p, B):
    at = 0
    for i, (lane, lo, rows) in enumerate(p["chunks"]):
        assert lane == i % p["lanes"] and lo == at == i * p["chunk"] and 0 < rows <= p["chunk"], (B, i, p)
        at += rows
    assert at == B and p["n"] == len(p["chunks"]) == -(-B // p["chunk"])
    assert all(rows == p["chunk"] for _, _, rows in p["chunks"][:-1])


@pytest.mark.parametrize("N,K,D", SHAPES)
def test_lane_extents_are_disjoint_and_inside_the_workspace(N, K, D):
    _, L = _lib()
    per, slack = sg.ws_layout(L, N, K, D)
    dc = sg.default_chunk(per, sg.constants()["default_chunk_max"])
    for B in (2, 3, 129, 257, 700, 8320, dc - 1, dc, dc + 1, 10 * dc + 77):
        for ws in (L.mcq_encode_workspace_bytes(B, N, K, D), slack + per * 256):
            p = plan(L, B, N, K, D, ws, 2)
            assert p["lanes"] == 2 and p["off"][0] == 0 and p["off"][1] % 256 == 0, (B, ws, p)
            total = carve_total(L, p["chunk"], N, K, D)              # what a lane's largest chunk occupies
            assert total <= p["lane_bytes"] <= p["off"][1], (B, ws, p, total)             # lane 0 ends before lane 1 begins
            assert p["off"][1] + p["lane_bytes"] <= ws, (B, ws, p)                           # lane 1 ends inside the workspace
            check_tiling(p, B)
            half = (B + 1) // 2
            assert p["chunk"] == half or (p["chunk"] < half and p["chunk"] % 128 == 0 and p["chunk"] >= 128), (B, ws, p)
            # the largest chunk the rule allows: a lane's share of a library-sized workspace holds half of the one-lane chunk
            if ws == L.mcq_encode_workspace_bytes(B, N, K, D):
                assert p["chunk"] == (half if B <= dc else (dc // 2) & ~127), (B, p)
    # the workspace did not grow with the lanes: the same bytes per vector, and a slack of two lanes' alignment and padding
    assert L.mcq_encode_workspace_bytes(10 ** 7, N, K, D) == slack + per * dc


def test_chunk_plan_over_small_batches_and_round_multiples():
    _, L = _lib()
    N, K, D = 8, 256, 64
    per, slack = sg.ws_layout(L, N, K, D)
    ws = slack + per * 256                       # shares of 128 vectors
    sizes = sorted(set(range(1, 301)) | {k * 128 + d for k in range(1, 12) for d in (-1, 0, 1)})
    for B in sizes:
        two, one = plan(L, B, N, K, D, ws, 2), plan(L, B, N, K, D, ws, 1)
        assert one["lanes"] == 1 and one["chunk"] == sg.chunk_of(B, 256) and one["off"] == (0, 0)        # the chunking it always had
        assert [(lo, rows) for _, lo, rows in one["chunks"]] == sg.chunks(B, one["chunk"])
        check_tiling(one, B)
        if B == 1:
            assert two == one                   # lane 1 would get nothing
            continue
        check_tiling(two, B)
        assert two["lanes"] == 2 and two["chunk"] == ((B + 1) // 2 if B <= 256 else 128), (B, two)
        assert [lane for lane, _, _ in two["chunks"]] == [i & 1 for i in range(two["n"])]
    # a whole workspace of its own for the batch: always two halves, whatever the parity
    for B in sizes[1:]:
        p = plan(L, B, N, K, D, L.mcq_encode_workspace_bytes(B, N, K, D), 2)
        assert p["n"] == 2 and [rows for _, _, rows in p["chunks"]] == [(B + 1) // 2, B // 2], (B, p)


def test_headline_and_shard_plans():
    _, L = _lib()
    N, K, D = 8, 256, 512
    ws = L.mcq_encode_workspace_bytes(65536, N, K, D)
    assert ws == L.mcq_encode_workspace_bytes(1 << 20, N, K, D)
    p = plan(L, 65536, N, K, D, ws, 2)
    assert p["chunks"] == [(0, 0, 32768), (1, 32768, 32768)]
    p = plan(L, 1 << 20, N, K, D, ws, 2)
    assert p["chunk"] == 32768 and p["n"] == 32 and sum(1 for lane, _, _ in p["chunks"] if lane == 1) == 16
    assert plan(L, 1 << 20, N, K, D, ws, 1)["chunk"] == 65536
    # config D's shape (16 x 256, dim 1024) already runs two chunks on one lane, 34,816 + 30,720: 17,408 per lane, four chunks
    ws = L.mcq_encode_workspace_bytes(65536, 16, 256, 1024)
    one, two = plan(L, 65536, 16, 256, 1024, ws, 1), plan(L, 65536, 16, 256, 1024, ws, 2)
    assert one["chunk"] == 34816 and one["n"] == 2 and two["chunk"] == 17408 and two["n"] == 4


def test_hooks_decide_the_lanes(monkeypatch):
    _, L = _lib()
    N, K, D = 8, 256, 64

    def lanes(B, **env):
        for k in ("MCQ_ENCODE_LANES", "MCQ_ENCODE_LANES_MIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        return plan(L, B, N, K, D, L.mcq_encode_workspace_bytes(B, N, K, D), 0)["lanes"]

    assert lanes(8320, MCQ_ENCODE_LANES=2, MCQ_ENCODE_LANES_MIN=0) == 2 and lanes(2, MCQ_ENCODE_LANES=2, MCQ_ENCODE_LANES_MIN=0) == 2
    assert lanes(1, MCQ_ENCODE_LANES=2, MCQ_ENCODE_LANES_MIN=0) == 1
    assert lanes(8320, MCQ_ENCODE_LANES=1, MCQ_ENCODE_LANES_MIN=0) == 1 and lanes(1 << 20, MCQ_ENCODE_LANES=1) == 1
    assert lanes(8320, MCQ_ENCODE_LANES=2, MCQ_ENCODE_LANES_MIN=8321) == 1 and lanes(8321, MCQ_ENCODE_LANES=2, MCQ_ENCODE_LANES_MIN=8321) == 2
    # the launch census and the small-batch latencies see the sequence they always saw, whatever ships as the default
    assert lanes(256) == 1 and lanes(4096) == 1 and lanes(8320) == 1


def test_argument_checks():
    m, L = _lib()
    out = (ctypes.c_long * 16)()
    big = 1 << 40
    assert L.mcq_test_chunk_plan(5, 3, 256, 32, big, 0, out, 16) == m.MCQ_EINVAL
    assert L.mcq_test_chunk_plan(0, 8, 2048, 32, big, 9, None, -1) == m.MCQ_EUNSUPPORTED            # the domain first
    for bad in (dict(B=0), dict(B=-1), dict(lanes=-1), dict(lanes=3), dict(out=None), dict(cap=-1)):
        a = dict(B=5, lanes=0, out=out, cap=16)
        a.update(bad)
        assert L.mcq_test_chunk_plan(a["B"], 8, 256, 32, big, a["lanes"], a["out"], a["cap"]) == m.MCQ_EINVAL, bad
    need = L.mcq_encode_workspace_bytes(5, 8, 256, 32)
    assert L.mcq_test_chunk_plan(6, 8, 256, 32, need, 1, out, 16) == m.MCQ_EWORKSPACE
    assert L.mcq_test_chunk_plan(5, 8, 256, 32, need, 1, out, 16) == HEAD and out[1] == 5
    assert L.mcq_test_chunk_plan(5, 8, 256, 32, 0, 2, out, 16) == m.MCQ_EWORKSPACE
    out[3] = 77
    assert L.mcq_test_chunk_plan(5, 8, 256, 32, need, 2, out, 3) == HEAD and out[3] == 77 and tuple(out[:3]) == (2, 3, 2)      # cap is honoured
