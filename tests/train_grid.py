"""Host mirror of the launch arithmetic of the trainer's kernels (quantization_amd/csrc/mcq_api.hip, mcq_loss_kernels.h,
mcq_train_kernels.h, mcq_kernels.h), and the lengths of their addition chains that tests/test_gpu_train_kernels.py builds
its tolerances from.

Which code path a launch takes (rows per chunk of k_loss_fwd, the wave mapping and width of k_decode_backward, the batch
splits of the weight gradient, the grid-stride trips of k_adam) depends on a handful of constants.  They are read from the
source, so that a moved constant makes tests/test_train_grid_host.py fail instead of leaving a GPU case covering nothing."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantization_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _body(src, signature):
    """the text of the function whose definition starts with `signature`, up to its closing brace at column 0"""
    i = src.index(signature)
    return src[i:src.index("\n}", i)]


def _int(pattern, text, what):
    m = re.search(pattern, text, re.S)
    assert m, f"{what} moved in the kernel sources: update tests/train_grid.py"
    return [int(g) for g in m.groups()]


def constants():
    api, loss, train = _src("mcq_api.hip"), _src("mcq_loss_kernels.h"), _src("mcq_train_kernels.h")
    c = {}
    c["loss_waves"], = _int(r"constexpr int kLossWaves = (\d+);", loss, "kLossWaves")
    c["reduce_unroll"], = _int(r"k_loss_reduce\(.*?constexpr int U = (\d+);", loss, "k_loss_reduce's unroll")
    rpc = _body(api, "long loss_rows_per_chunk(long B)")
    a, b, lo, lo2, r16, r16b = _int(r"r = \(B \+ (\d+)\) / (\d+);\s*r = r < (\d+) \? (\d+) : r;\s*return \(r \+ (\d+)\) / (\d+) \* \d+;",
                                    rpc, "loss_rows_per_chunk")
    assert a + 1 == b and lo == lo2 and r16 + 1 == r16b
    c["loss_chunks_max"], c["loss_rows_min"], c["loss_rows_round"] = b, lo, r16b
    c["wg_m"], c["wg_n"] = _int(r"constexpr int kWgM = (\d+), kWgN = (\d+);", train, "kWgM / kWgN")
    c["wb_m"], c["wb_n"] = _int(r"constexpr int kWbM = (\d+), kWbN = (\d+);", train, "kWbM / kWbN")
    c["bf3_min_m"], c["bf3_min_b"] = _int(r"M >= (\d+) && B >= (\d+);", _body(api, "bool wgrad_use_bf3("), "wgrad_use_bf3")
    c["bf3_target"], c["bf3_rows_min"] = _int(r"long s = \((\d+) \+ tiles / 2\) / tiles;.*?max_s = B / (\d+);",
                                              _body(api, "int wgrad_splits_bf3("), "wgrad_splits_bf3")
    c["f32_target"], c["f32_rows_min"], c["f32_splits_max"] = _int(
        r"long s = (\d+) / tiles;.*?max_s = \(B \+ \d+\) / (\d+);.*?s > (\d+) \?", _body(api, "int wgrad_splits("), "wgrad_splits")
    c["split_round"], = _int(r"rps = \(rps \+ \d+\) / (\d+) \* \d+;", _body(api, "int mcq_weight_grad("), "rows_per_split rounding")
    c["db_k_wide"], c["db_d4"], c["db_d2"] = _int(r"if \(K >= (\d+)\) return 4;\s*return D >= (\d+) \? 4 : \(D >= (\d+) \? 2 : 1\);",
                                                  _body(api, "int db_cw_of("), "db_cw_of")
    c["adam_blocks_max"], = _int(r"blocks > (\d+) \? \d+ : blocks", _body(api, "int mcq_adam_step("), "the Adam block cap")
    return c


C = None


def _c():
    global C
    if C is None:
        C = constants()
    return C


# ------------------------------------------------------------------ k_loss_fwd / k_loss_reduce / k_loss_bwd
def loss_rows_per_chunk(B):
    c = _c()
    r = max((B + c["loss_chunks_max"] - 1) // c["loss_chunks_max"], c["loss_rows_min"])
    return (r + c["loss_rows_round"] - 1) // c["loss_rows_round"] * c["loss_rows_round"]


def loss_chunks(B):
    r = loss_rows_per_chunk(B)
    return (B + r - 1) // r


def loss_workspace_bytes(B, N, K):
    return 256 if B <= 0 else loss_chunks(B) * N * (2 * K + 1) * 4 + 256


def rows_per_wave(K):
    """RPW: logits rows one wave works on at a time (KL = min(K, 64) lanes per row)"""
    return 64 // min(K, 64)


def loss_bwd_waves(B, N, K):
    rpw, w = rows_per_wave(K), _c()["loss_waves"]
    return (B * N + w * rpw - 1) // (w * rpw) * w


def loss_fwd_rows_per_lane(B, K):
    """rows of one chunk that one lane's accumulator adds (a chunk's rows are dealt to loss_waves * RPW row slots)"""
    slots = _c()["loss_waves"] * rows_per_wave(K)
    return (min(loss_rows_per_chunk(B), B) + slots - 1) // slots


def loss_fwd_chain(B, K):
    """longest addition chain behind prob_sum / chosen_sum: a lane's rows, the row slots (chosen: the butterfly and the
    waves), the chunks"""
    slots = _c()["loss_waves"] * rows_per_wave(K)
    return loss_fwd_rows_per_lane(B, K) + slots + 6 + loss_chunks(B)


def row_chain(K):
    """values per lane plus butterfly depth of one row's softmax sums"""
    kl = min(K, 64)
    return K // kl + kl.bit_length() - 1


# ------------------------------------------------------------------ k_recon_fwd
def recon_vector_branch(D, aligned=True):
    return D % 4 == 0 and aligned


def recon_chain(D, aligned=True):
    """fmas of one lane (features lane, lane + 64, ...) + the wave butterfly + the four waves"""
    per_lane = (D + 63) // 64 if not recon_vector_branch(D, aligned) else 4 * ((D // 4 + 63) // 64)
    return per_lane + 6 + 3


# ------------------------------------------------------------------ k_decode_backward
def db_cw_of(D, K):
    c = _c()
    if D % 4:
        return 1
    if K >= c["db_k_wide"]:
        return 4
    return 4 if D >= c["db_d4"] else (2 if D >= c["db_d2"] else 1)


def db_alignment():
    """(stride mask, pointer mask) of db_cw: rows are read as float4 only when D and both strides are multiples of
    stride mask + 1 floats and grad, out and dotw start on a multiple of pointer mask + 1 bytes"""
    body = _body(_src("mcq_api.hip"), "int db_cw(")
    d, sb, sn, pg, po, pw = _int(r"\(\(D & (\d+)\) == 0\) && \(\(gsb & (\d+)\) == 0\) && \(\(gsn & (\d+)\) == 0\) && "
                                 r"\(\(reinterpret_cast<uintptr_t>\(g\) & (\d+)\) == 0\) &&\s*"
                                 r"\(\(reinterpret_cast<uintptr_t>\(out\) & (\d+)\) == 0\) && "
                                 r"\(\(reinterpret_cast<uintptr_t>\(dotw\) & (\d+)\) == 0\);\s*return al \? db_cw_of\(D, K\) : 1;",
                                 body, "db_cw's alignment rule")
    assert d == sb == sn and pg == po == pw
    return d, pg


def db_cw(D, K, gsb, gsn, g_addr=0, out_addr=0, dotw_addr=0):
    """floats per lane of a launch: db_cw_of when every row involved is 16-byte aligned (strides in floats, addresses in
    bytes), else 1"""
    sm, pm = db_alignment()
    al = not (D & sm or gsb & sm or gsn & sm or g_addr & pm or out_addr & pm or dotw_addr & pm)
    return db_cw_of(D, K) if al else 1


def db_chunks(D, cw):
    return (D + 64 * cw - 1) // (64 * cw)


def db_xcd_mapping(D, K):
    ch = db_chunks(D, db_cw_of(D, K))
    return ch <= 8 and 8 % ch == 0


def decode_backward_waves(N, K, D):
    return N * K * db_chunks(D, db_cw_of(D, K))


# ------------------------------------------------------------------ weight gradient
def wgrad_use_bf3(B, M, D):
    c = _c()
    return M % c["wb_m"] == 0 and D % c["wb_n"] == 0 and M >= c["bf3_min_m"] and B >= c["bf3_min_b"]


def wgrad_splits_bf3(B, M, D):
    c = _c()
    tiles = (M // c["wb_m"]) * (D // c["wb_n"])
    s = (c["bf3_target"] + tiles // 2) // tiles
    return max(min(s, B // c["bf3_rows_min"]), 1)


def wgrad_splits(B, M, D):
    c = _c()
    tiles = -(-M // c["wg_m"]) * -(-D // c["wg_n"])
    s = min(c["f32_target"] // tiles, (B + c["f32_rows_min"] - 1) // c["f32_rows_min"])
    return max(min(s, c["f32_splits_max"]), 1)


def weight_grad_workspace_bytes(B, M, D):
    return 256 if B <= 0 or M <= 0 or D <= 0 else wgrad_splits(B, M, D) * (M * D + M) * 4 + 256


def wgrad_plan(B, M, D):
    """(bf16-piece kernel?, splits, rows per split, rows of each split)"""
    bf3 = wgrad_use_bf3(B, M, D)
    s = wgrad_splits_bf3(B, M, D) if bf3 else wgrad_splits(B, M, D)
    r = _c()["split_round"]
    rps = (-(-B // s) + r - 1) // r * r
    return bf3, s, rps, [max(0, min(rps, B - q * rps)) for q in range(s)]


def wgrad_chain(B, M, D):
    """rows of the longest split (one accumulator adds them; the bf16 kernel six piece products each) + the splits"""
    bf3, s, rps, rows = wgrad_plan(B, M, D)
    return max(rows) * (6 if bf3 else 1) + s


# ------------------------------------------------------------------ k_adam
def adam_blocks(n):
    return max(1, min((n // 4 + 255) // 256, _c()["adam_blocks_max"]))


def adam_trips(n):
    """grid-stride trips of the last thread that has work: the floats past blocks * 256 * 4 need a second trip"""
    per = adam_blocks(n) * 256 * 4
    return -(-n // per)
