"""The workspace contract of every entry that takes `void *workspace, size_t workspace_bytes`, on the GPU (DESIGN.md,
"Workspace contract"; tests/arena.py lays the guarded memory out).  ONE case table, ROWS, one row per (entry, shape); per row:

  a. clean      a workspace of EXACTLY the size query's bytes, zero-filled: the outputs equal what the entry's own test holds it
                to -- the oracle's codes and logits bit for bit (encode family, mcq_logits*), the numpy restatements of
                tests/*_grid.py bit for bit (every search, range, wide, two-byte, shortlist and rerank entry), float64 within the
                bounds of tests/test_gpu_train_kernels.py (mcq_loss_fwd, mcq_weight_grad: hold_loss_fwd, hold_weight_grad)
  b. invariance the same call on a workspace of 0xFF bytes (NaN as float, -1 as int, 2^32 - 1 as a counter), of 0xA5 bytes and
                on the LEFTOVER of another row of the table with a larger workspace (as that row's clean run left it, copied to
                the front and repeated): every output bitwise equal to the clean run's.  No entry is left out: none is
                documented as differing between two runs
  c. bounds     after every run neither guard of the workspace nor of any output is damaged, output elements outside the
                documented extent keep their pre-fill, and every const input is bit-identical (arena.frozen)
  d. refusal    one byte less returns MCQ_EWORKSPACE with the workspace, the outputs and the inputs untouched; for the encode
                family "too small" is one byte less than the smallest workspace mcq_test_chunk_plan reports a plan for
  e. empty      B == 0 (Q == 0 for the shortlist entries) returns 0 with the workspace untouched; top-k outputs hold (+inf, -1),
                an empty range call writes lims and nothing else, the encode family writes nothing

A count / fill pair is one row: count then fill share the workspace (rules 9 and 20), and (b) compares the pair's outputs.  The
probes mcq_test_xc, mcq_test_xc_xx, mcq_test_er, mcq_test_pass and mcq_test_pass16 get (b) and (c) only.  mcq_profile_encode is left out: it
times, it does not compute (tests/test_workspace_contract_host.py keeps the list of entries complete and checks, without a
GPU, what every row CLAIMS: parts, lanes, chunks, merge side)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import arena as ar
import rerank_grid as rr
import search_bias_grid as bg
import search_grid as sg
import search_lists_grid as lg
import search_mask_grid as kg
import search_metric_grid as mg
import search_range_grid as rg
import search_range_lists_grid as rl
import search_shortlist_grid as hg
import search_wide_grid as wg
import skip_grid as sk
import train_grid as tg

pytestmark = pytest.mark.gpu

HOOKS = ("MCQ_ENCODE_LANES", "MCQ_ENCODE_LANES_MIN", "MCQ_SKIP_MIN_BATCH", "MCQ_LAZY_TABLES_MIN", "MCQ_ER_DENSE_MIN",
         "MCQ_PASS_CAP_WAVE", "MCQ_PASS_CAP_STAGE0")
THRESHOLDS_0 = {"MCQ_SKIP_MIN_BATCH": "0", "MCQ_LAZY_TABLES_MIN": "0", "MCQ_ER_DENSE_MIN": "0"}
ONE_LANE = {"MCQ_ENCODE_LANES": "1"}
TWO_LANES = {"MCQ_ENCODE_LANES": "2", "MCQ_ENCODE_LANES_MIN": "0"}
CAPS_8 = {"MCQ_PASS_CAP_WAVE": "8", "MCQ_PASS_CAP_STAGE0": "8"}
ALL_PASSES, X_FP16, EXACT_LOGITS = 8, 4, 16
EXCLUDED = {"mcq_profile_encode": "it times the encode, it does not compute: nothing to compare between two runs"}
PLAN_HEAD = 6


@contextlib.contextmanager
def hooks(env):
    """the tuning hooks of the encode (all read per call) set to `env`, every other one unset; restored on exit"""
    saved = {k: os.environ.get(k) for k in HOOKS}
    for k in HOOKS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _mods():
    from quantization_amd import _lib
    L = _lib.lib()
    L.mcq_last_encode_lanes.restype, L.mcq_last_encode_lanes.argtypes = ctypes.c_int, []
    L.mcq_test_chunk_plan.restype = ctypes.c_int
    L.mcq_test_chunk_plan.argtypes = [ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_size_t, ctypes.c_int,
                                      ctypes.POINTER(ctypes.c_long), ctypes.c_int]
    return _lib, L


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


# ================================================================== the case table
class Row:
    """id; entries: what the row calls with the workspace; kind: the adapter (JOBS); p: its parameters; claims: what makes the
    row non-trivial, checked through the mirrors by claims_hold (host and GPU); donor: the row whose clean run leaves the
    `leftover`; checks: which of a-e apply; env: the encode's hooks"""

    def __init__(self, id, entries, kind, p, claims, donor, checks="abcde", env=None):
        self.id, self.entries, self.kind, self.p, self.claims = id, tuple(entries), kind, dict(p), dict(claims)
        self.donor, self.checks, self.env = donor, checks, dict(env or {})


def _search_rows():
    rows = []
    SMALL, BIG = (1, 16), (8, 256)

    def add(id, entries, p, claims, donor, kind="search"):
        rows.append(Row(id, entries, kind, p, claims, donor))

    # ---- the scan of the whole store: the slices of tile_plan are the parts
    for entry, extra in (("mcq_search_scan", {}), ("mcq_search_scan_metric", dict(metric="cosine")),
                         ("mcq_search_scan_masked", dict(metric="ip", mask=True))):
        short = entry[len("mcq_search_"):]
        add(f"{short}-one", [entry], dict(entry=entry, Q=1, NK=SMALL, B=300, k=1, **extra), dict(plan="scan", parts=1), f"{short}-parts")
        add(f"{short}-parts", [entry], dict(entry=entry, Q=5, NK=BIG, B=1031, k=64, **extra), dict(plan="scan", parts_min=2),
            f"{short}-k64-q1")
        add(f"{short}-k64-q1", [entry], dict(entry=entry, Q=1, NK=BIG, B=1031, k=64, **extra), dict(plan="scan", parts_min=2),
            f"{short}-parts")
    # ---- list by list: the parts depend on Q alone (1,024 / Q), so one part needs more than 512 queries
    for entry, extra in (("mcq_search_scan_lists", dict(metric="l2", mask=True)), ("mcq_search_scan_lists_bias", dict(metric="cosine", bias=True))):
        short = entry[len("mcq_search_"):]
        add(f"{short}-one", [entry], dict(entry=entry, Q=600, NK=SMALL, B=300, k=1, P=2, **extra), dict(plan="lists", parts=1),
            f"{short}-parts")
        add(f"{short}-parts", [entry], dict(entry=entry, Q=5, NK=BIG, B=1031, k=64, P=4, **extra), dict(plan="lists", parts_min=2),
            f"{short}-one")
    # ---- the four range pairs: count then fill on one workspace
    pairs = (("range", ("mcq_search_range_count", "mcq_search_range_fill"), dict(metric="l2"), "range"),
             ("range_masked", ("mcq_search_range_count_masked", "mcq_search_range_fill_masked"), dict(metric="cosine", mask=True), "range"),
             ("range_lists", ("mcq_search_range_lists_count", "mcq_search_range_lists_fill"), dict(metric="ip", P=4), "range_lists"),
             ("range_lists_bias", ("mcq_search_range_lists_bias_count", "mcq_search_range_lists_bias_fill"),
              dict(metric="l2", P=4, bias=True, mask=True), "range_lists"))
    for short, entries, extra, plan in pairs:
        one_q = 1 if plan == "range" else 1100                # (1,024 / Q parts list by list: one part needs Q > 1,024 here)
        p1 = dict(extra)
        if plan == "range_lists":
            p1["P"] = 2
        add(f"{short}-one", entries, dict(entry=entries[0], fill=entries[1], Q=one_q, NK=SMALL, B=300, **p1), dict(plan=plan, parts=1),
            f"{short}-parts")
        add(f"{short}-parts", entries, dict(entry=entries[0], fill=entries[1], Q=5, NK=BIG, B=1031, **extra), dict(plan=plan, parts_min=2),
            f"{short}-one")
    # ---- past 64 neighbours: both sides of the old cap, and a k past the small half of the wide list
    for entry, extra, big_q in (("mcq_search_wide", dict(metric="l2", mask=True), 1100), ("mcq_search_wide_lists", dict(metric="ip", P=4, bias=True), 1100),
                                ("mcq_search_topk_u16", dict(metric="cosine", u16=True), 1100)):
        short = entry[len("mcq_search_"):]
        shape = (4, 512) if extra.get("u16") else BIG
        p1 = dict(extra)
        if "P" in p1:
            p1["P"] = 2
        add(f"{short}-one-k1", [entry], dict(entry=entry, Q=big_q, NK=(1, 1024) if extra.get("u16") else SMALL, B=300, k=1, **p1),
            dict(plan="wide", parts=1, half="small"), f"{short}-k600")
        for k, half in ((64, "small"), (65, "small"), (600, "large")):
            add(f"{short}-k{k}", [entry], dict(entry=entry, Q=5, NK=shape, B=1031, k=k, **extra), dict(plan="wide", parts_min=2, half=half),
                f"{short}-k600" if k != 600 else f"{short}-k65")
    # ---- the two-byte range pair: the whole store (no probes) and list by list
    u16 = ("mcq_search_range_u16_count", "mcq_search_range_u16_fill")
    add("range_u16-one", u16, dict(entry=u16[0], fill=u16[1], Q=1100, NK=(1, 1024), B=300, metric="l2", u16=True),
        dict(plan="range_lists", parts=1), "range_u16-parts")
    add("range_u16-parts", u16, dict(entry=u16[0], fill=u16[1], Q=5, NK=(4, 512), B=1031, metric="cosine", u16=True, P=4, bias=True, mask=True),
        dict(plan="range_lists", parts_min=2), "range_u16-one")
    # ---- shortlists: the parts follow the steps of the shortlist
    for entry, shape in (("mcq_search_shortlist", BIG), ("mcq_search_shortlist_u16", (4, 512))):
        short = entry[len("mcq_search_"):]
        add(f"{short}-one-k1", [entry], dict(entry=entry, Q=1, NK=shape, B=300, S=16, k=1, metric="l2", u16=shape[1] > 256),
            dict(plan="short", parts=1, half="small"), f"{short}-k600", kind="shortlist")
        for k, half in ((64, "small"), (65, "small"), (600, "large")):
            add(f"{short}-k{k}", [entry], dict(entry=entry, Q=5, NK=shape, B=1031, S=300, k=k, metric="cosine", u16=shape[1] > 256, bias=True,
                                               row_of=True),
                dict(plan="short", parts_min=2, half=half), f"{short}-k600" if k != 600 else f"{short}-k65", kind="shortlist")
    add("rerank-one-k1", ["mcq_rerank"], dict(Q=1, D=37, B=300, S=16, k=1, metric="l2"), dict(plan="rerank", parts=1, half="small"),
        "rerank-k600", kind="rerank")
    for k, half in ((64, "small"), (65, "small"), (600, "large")):
        add(f"rerank-k{k}", ["mcq_rerank"], dict(Q=5, D=130, B=1031, S=300, k=k, metric="cosine", row_of=True),
            dict(plan="rerank", parts_min=2, half=half), "rerank-k600" if k != 600 else "rerank-k65", kind="rerank")
    return rows


def _encode_rows():
    """the encode family at B = 300 (more than one 128-row tile, a ragged last one) in an exactly sized workspace.  The leftover
    of every row comes from a row with another N x K and more vectors: enc-donor-16x256 (B = 520) or, for itself and the other
    16 x 256 rows, enc-donor-8x256 (B = 700)"""
    rows = []
    D1, D2 = "enc-donor-16x256", "enc-donor-8x256"

    def add(id, p, claims=None, env=None, entry="mcq_encode_ex", donor=D1, kind="encode", checks="abcde"):
        rows.append(Row(id, [entry], kind, dict(entry=entry, **p), {**dict(plan="encode", lanes=1, chunks=1, skips=False), **(claims or {})}, donor,
                        checks, {**ONE_LANE, **(env or {})}))

    add(D1, dict(NKD=(16, 256, 64), B=520, iters=2), donor=D2)
    add(D2, dict(NKD=(8, 256, 64), B=700, iters=2))
    for iters in (0, 1, 5):                                   # (a call of fewer than three passes never skips: skip_grid.skips)
        add(f"enc-8x256x37-it{iters}-skip", dict(NKD=(8, 256, 37), B=300, iters=iters), claims=dict(skips=iters >= 3), env=THRESHOLDS_0)
        add(f"enc-8x256x37-it{iters}-all", dict(NKD=(8, 256, 37), B=300, iters=iters, flags=ALL_PASSES), env=THRESHOLDS_0)
    add("enc-plain-mcq_encode", dict(NKD=(8, 256, 37), B=300, iters=3), entry="mcq_encode")
    add("enc-16x16-bytes", dict(NKD=(16, 16, 64), B=300, iters=5))                   # packed nibbles, the LDS-resident pass
    add("enc-16x16-i64", dict(NKD=(16, 16, 64), B=300, iters=5, i64=True))
    add("enc-8x16-bytes", dict(NKD=(8, 16, 64), B=300, iters=5))
    add("enc-8x16-i64", dict(NKD=(8, 16, 64), B=300, iters=5, i64=True))
    add("enc-4x512-two-byte", dict(NKD=(4, 512, 32), B=300, iters=3, i64=True), claims=dict(skips=True), env=THRESHOLDS_0)
    add("enc-1x256-no-lists", dict(NKD=(1, 256, 16), B=300, iters=3))
    add("enc-16x256x130", dict(NKD=(16, 256, 130), B=300, iters=3), claims=dict(skips=True), env=THRESHOLDS_0, donor=D2)
    add("enc-fp16-frames", dict(NKD=(8, 256, 37), B=300, iters=3, flags=X_FP16))
    add("enc-exact-logits", dict(NKD=(8, 256, 37), B=300, iters=3, flags=EXACT_LOGITS))
    add("enc-two-lanes", dict(NKD=(8, 256, 37), B=300, iters=5), claims=dict(lanes=2, chunks=2, skips=True), env={**TWO_LANES, **THRESHOLDS_0})
    add("enc-three-chunks", dict(NKD=(8, 256, 37), B=300, iters=5, smallest=True), claims=dict(chunks=3, chunk=128, last=44, skips=True), env=THRESHOLDS_0)
    add("enc-capped-forms", dict(NKD=(8, 256, 37), B=300, iters=5), claims=dict(skips=True, loops=True), env={**THRESHOLDS_0, **CAPS_8})
    add("refine_indexes-8x256", dict(NKD=(8, 256, 37), B=300, iters=2), entry="mcq_refine_indexes", env=THRESHOLDS_0)
    add("refine_indexes-16x16", dict(NKD=(16, 16, 64), B=300, iters=2), entry="mcq_refine_indexes")
    add("logits_refine-8x256", dict(NKD=(8, 256, 37), B=300, iters=3), entry="mcq_logits_refine")
    add("logits_refine_codes-8x256", dict(NKD=(8, 256, 37), B=300, iters=3), entry="mcq_logits_refine_codes", env=THRESHOLDS_0)
    # the logits-sized workspace (mcq_logits_workspace_bytes): limb planes of the frames
    for entry in ("mcq_logits", "mcq_logits_argmax", "mcq_test_xc", "mcq_test_xc_xx"):
        short = entry[len("mcq_"):]
        checks = "bc" if entry.startswith("mcq_test_") else "abcde"
        rows.append(Row(f"{short}-8x256x37", [entry], "logits", dict(entry=entry, NKD=(8, 256, 37), B=300), dict(plan="bytes"),
                        f"{short}-16x16x64", checks))
        rows.append(Row(f"{short}-16x16x64", [entry], "logits", dict(entry=entry, NKD=(16, 16, 64), B=520), dict(plan="bytes"),
                        f"{short}-8x256x37", checks))
    # the other probes: invariance and bounds only
    for form in (0, 1):                                       # (the one direct launch; the pair whose Gram terms cross the workspace)
        rows.append(Row(f"test_er-8x256-form{form}", ["mcq_test_er"], "er", dict(NKD=(8, 256, 37), B=300, form=form), dict(plan="bytes"),
                        f"test_er-16x16-form{form}", "bc"))
        rows.append(Row(f"test_er-16x16-form{form}", ["mcq_test_er"], "er", dict(NKD=(16, 16, 64), B=520 - 8 * form, form=form),
                        dict(plan="bytes"), f"test_er-16x16-form{1 - form}", "bc"))        # (the largest two: each other's donor)
    rows.append(Row("test_pass-8x256", ["mcq_test_pass"], "pass", dict(NKD=(8, 256, 37), B=300, flags=0), dict(plan="bytes"),
                    "test_pass-16x256-capped", "bc"))
    rows.append(Row("test_pass-16x256-capped", ["mcq_test_pass"], "pass", dict(NKD=(16, 256, 64), B=520, flags=1), dict(plan="bytes"),
                    "test_pass-8x256", "bc", CAPS_8))
    rows.append(Row("test_pass16-16x16", ["mcq_test_pass16"], "pass16", dict(NKD=(16, 16, 64), B=300, iters=3), dict(plan="bytes"),
                    "test_pass16-8x16", "bc"))
    rows.append(Row("test_pass16-8x16", ["mcq_test_pass16"], "pass16", dict(NKD=(8, 16, 64), B=520, iters=3), dict(plan="bytes"),
                    "test_pass16-16x16", "bc"))
    return rows


def _train_rows():
    return [Row("loss_fwd-8x256", ["mcq_loss_fwd"], "loss", dict(N=8, K=256, B=300), dict(plan="loss", chunks_min=2), "loss_fwd-64x16", "abcd"),
            Row("loss_fwd-64x16", ["mcq_loss_fwd"], "loss", dict(N=64, K=16, B=1031), dict(plan="loss", chunks_min=2), "loss_fwd-8x256", "abcd"),
            Row("weight_grad-f32", ["mcq_weight_grad"], "wgrad", dict(B=333, M=128, D=40), dict(plan="wgrad", bf3=False, splits_min=2),
                "weight_grad-f32-big", "abcd"),
            Row("weight_grad-f32-big", ["mcq_weight_grad"], "wgrad", dict(B=1031, M=272, D=36), dict(plan="wgrad", bf3=False, splits_min=2),
                "weight_grad-bf3", "abcd"),
            # the bf16-piece kernel (the trainer's): its launcher takes wgrad_splits_bf3 planes of a workspace sized by wgrad_splits
            Row("weight_grad-bf3", ["mcq_weight_grad"], "wgrad", dict(B=2048, M=1024, D=128), dict(plan="wgrad", bf3=True, splits_min=2),
                "weight_grad-f32-big", "abcd")]


ROWS = _search_rows() + _encode_rows() + _train_rows()
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS) and all(r.donor in BY_ID and r.donor != r.id for r in ROWS)


# ================================================================== what a row claims, through the mirrors (no GPU)
def size_query(L, row):
    """the library's size query for the row -> bytes"""
    p = row.p
    if row.kind in ("search", "shortlist"):
        (N, K), Q, B = p["NK"], p["Q"], p["B"]
        e, P = p["entry"], p.get("P", 1)
        if row.kind == "shortlist":
            return L.mcq_search_shortlist_workspace_bytes(Q, p["S"], N, K, p["k"])
        if e in ("mcq_search_scan", "mcq_search_scan_metric", "mcq_search_scan_masked"):
            return L.mcq_search_workspace_bytes(Q, B, N, K, p["k"])
        if e in ("mcq_search_scan_lists", "mcq_search_scan_lists_bias"):
            return L.mcq_search_lists_workspace_bytes(Q, P, N, K, p["k"])
        if e in ("mcq_search_range_count", "mcq_search_range_count_masked"):
            return L.mcq_search_range_workspace_bytes(Q, B, N, K)
        if e in ("mcq_search_range_lists_count", "mcq_search_range_lists_bias_count"):
            return L.mcq_search_range_lists_workspace_bytes(Q, P, N, K)
        if e == "mcq_search_wide":
            return L.mcq_search_wide_workspace_bytes(Q, B, N, K, p["k"])
        if e == "mcq_search_wide_lists":
            return L.mcq_search_wide_lists_workspace_bytes(Q, P, N, K, p["k"])
        if e == "mcq_search_topk_u16":
            return L.mcq_search_topk_u16_workspace_bytes(Q, P, N, K, p["k"])
        assert e == "mcq_search_range_u16_count", e
        return L.mcq_search_range_u16_workspace_bytes(Q, P, N, K)
    if row.kind == "rerank":
        return L.mcq_rerank_workspace_bytes(p["Q"], p["S"], p["D"], p["k"])
    if row.kind in ("encode", "pass", "pass16"):
        N, K, D = p["NKD"]
        return smallest_encode_workspace(L, row) if p.get("smallest") else L.mcq_encode_workspace_bytes(p["B"], N, K, D)
    if row.kind == "logits":
        N, K, D = p["NKD"]
        return L.mcq_logits_workspace_bytes(p["B"], N, D)
    if row.kind == "er":
        return L.mcq_test_er_workspace_bytes(p["B"], p["NKD"][0])
    if row.kind == "loss":
        return L.mcq_loss_workspace_bytes(p["B"], p["N"], p["K"])
    assert row.kind == "wgrad", row.kind
    return L.mcq_weight_grad_workspace_bytes(p["B"], p["M"], p["D"])


def chunk_plan(L, row, nbytes):
    """mcq_test_chunk_plan under the row's hooks -> None (no plan), or (lanes, chunk, chunks, [(lane, first, n), ...])"""
    N, K, D = row.p["NKD"]
    with hooks(row.env):
        head = (ctypes.c_long * PLAN_HEAD)()
        rc = L.mcq_test_chunk_plan(row.p["B"], N, K, D, nbytes, 0, head, PLAN_HEAD)
        if rc != PLAN_HEAD:
            return None
        out = (ctypes.c_long * (PLAN_HEAD + 3 * head[2]))()
        assert L.mcq_test_chunk_plan(row.p["B"], N, K, D, nbytes, 0, out, len(out)) == PLAN_HEAD
    return out[0], out[1], out[2], [tuple(out[PLAN_HEAD + 3 * i:PLAN_HEAD + 3 * i + 3]) for i in range(out[2])]


def smallest_encode_workspace(L, row):
    """the smallest workspace mcq_test_chunk_plan reports a plan for (bisection: a larger workspace always holds a plan)"""
    N, K, D = row.p["NKD"]
    lo, hi = 0, L.mcq_encode_workspace_bytes(row.p["B"], N, K, D)
    assert chunk_plan(L, row, hi) is not None and chunk_plan(L, row, lo) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if chunk_plan(L, row, mid) is not None else (mid, hi)
    return hi


_API = []


def _api_source():
    if not _API:
        with open(sk.API) as f:
            _API.append(f.read())
    return _API[0]


def claims_hold(L, row):
    """asserts what the row claims, by the mirrors of tests/*_grid.py and the library's host-only plan queries"""
    p, c, need = row.p, row.claims, size_query(L, row)
    plan = c["plan"]
    for hook in row.env:                                     # a hook that was renamed would leave the row on the plain path
        assert f'"{hook}"' in _api_source(), (row.id, hook, "is not read by mcq_api.hip")
    if plan in ("scan", "lists", "range", "range_lists", "wide", "short", "rerank"):
        k = p.get("k", 1)
        if plan == "rerank":
            m = rr.rerank_plan(p["Q"], p["S"], p["D"], k)
        else:
            (N, K), Q, B, P = p["NK"], p["Q"], p["B"], p.get("P", 1)
            m = {"scan": lambda: sg.scan_plan(Q, B, N, K, k), "lists": lambda: lg.lists_plan(Q, P, N, K, k),
                 "range": lambda: rg.range_plan(Q, B, N, K), "range_lists": lambda: rl.range_lists_plan(Q, P, N, K),
                 "wide": lambda: wg.wide_plan(Q, P, N, K, k), "short": lambda: hg.short_plan(Q, p.get("S", 0), N, K, k)}[plan]()
        parts = m.slices if plan in ("scan", "range") else m.parts
        assert m.ws_bytes == need, (row.id, m.ws_bytes, need)
        assert parts == c["parts"] if "parts" in c else parts >= c["parts_min"], (row.id, parts)
        if "half" in c:
            wc = wg.constants()
            assert wg.wide_half(k, wc) == wc["half_" + c["half"]] and (c["half"] == "small") == (k <= wc["half_small"]), row.id
    elif plan == "encode":
        lanes, chunk, chunks, each = chunk_plan(L, row, need)
        assert (lanes, chunks) == (c["lanes"], c["chunks"]), (row.id, lanes, chunks)
        assert sum(n for _, _, n in each) == p["B"]
        if "chunk" in c:
            assert chunk == c["chunk"] and each[-1][2] == c["last"], (row.id, chunk, each)
            assert chunk_plan(L, row, need - 1) is None
        if p["entry"] in ("mcq_encode", "mcq_encode_ex"):
            N, K, _ = p["NKD"]
            smb = int(row.env.get("MCQ_SKIP_MIN_BATCH", sk.constants()["skip_min_batch"]))
            skips = not p.get("flags", 0) & ALL_PASSES and all(sk.skips(n, N, K, p["iters"], smb) for _, _, n in each)
            assert skips is c["skips"], (row.id, skips)
            if c.get("loops"):      # from the fourth pass on every capped kernel of the shape has more virtual workgroups than its cap
                caps = dict(cap_stage0=int(row.env["MCQ_PASS_CAP_STAGE0"]), cap_wave=int(row.env["MCQ_PASS_CAP_WAVE"]))
                kernels = sk.capped_kernels(N, K)
                assert skips and p["iters"] >= 4 and kernels and all(sk.binds(kn, n, N, K, caps) for kn in kernels for _, _, n in each), row.id
    elif plan == "loss":
        assert tg.loss_chunks(p["B"]) >= c["chunks_min"] and tg.loss_workspace_bytes(p["B"], p["N"], p["K"]) == need, row.id
    elif plan == "wgrad":
        bf3, splits, _, _ = tg.wgrad_plan(p["B"], p["M"], p["D"])
        assert bf3 is c["bf3"] and splits >= c["splits_min"] and tg.weight_grad_workspace_bytes(p["B"], p["M"], p["D"]) == need, row.id
        if bf3:         # the planes the launcher writes are no more than the size query counted
            assert splits == tg.wgrad_splits_bf3(p["B"], p["M"], p["D"]) <= tg.wgrad_splits(p["B"], p["M"], p["D"]), row.id
    else:
        assert plan == "bytes" and need > 256, row.id         # (no mirror: the workspace is more than the floor of 256 bytes)
    return need


# ================================================================== adapters: one Job per row
class Job:
    """need; consts (the const inputs); outputs() -> fresh guarded outputs; call(L, ws_ptr, ws_bytes, outs) -> status;
    verify(outs): the clean run against the independent answer; extent(outs): pre-fill kept outside the documented extent;
    empty(L, arena): the empty call, or None where the header defines none"""
    refuse = None                                            # bytes of the refused workspace (default: need - 1)

    def extent(self, outs):
        pass

    def verify(self, outs):
        raise NotImplementedError

    def empty(self, L, arena):
        return None


def _lists_for(B, Q, P, rs):
    """seven ragged lists covering [0, B) (lengths 1, 63, 0, 65, ...), and a row of P distinct probes per query, one entry -1"""
    cuts = sorted({0, 1, 64, 129, 129, B // 2 + 3, B - 7, B})
    offs = np.array(cuts[:3] + [cuts[2]] + cuts[3:], dtype=np.int64)      # (an empty list)
    nl = len(offs) - 1
    probes = np.stack([rs.permutation(nl)[:P] for _ in range(Q)]).astype(np.int32)
    if P >= 3:
        probes[0, 1] = -1
    return offs, probes


class SearchJob(Job):
    """every top-k, range, wide and two-byte entry over tables, codes and w drawn from a seed (the restatements take the
    tables and w as given: no quantizer is needed)"""

    def __init__(self, L, row):
        p = self.p = row.p
        (N, K), Q, B = p["NK"], p["Q"], p["B"]
        self.N, self.K, self.Q, self.B, self.k = N, K, Q, B, p.get("k")
        self.metric, self.e, self.fill_e = p["metric"] if "metric" in p else "l2", p["entry"], p.get("fill")
        rs = np.random.RandomState(1000 * N + K + 7 * Q + B)
        self.T = rs.standard_normal((Q, N, K)).astype(np.float32)
        self.codes = rs.randint(0, K, size=(B, N)).astype(np.uint16 if p.get("u16") else np.uint8)
        self.w = (rs.rand(B) + 0.5).astype(np.float32)
        self.keep = kg.keep_for("half", B, 1, self.k or 1) if p.get("mask") else None
        self.P = p.get("P")
        self.offs, self.probes = _lists_for(B, Q, self.P, rs) if self.P else (None, None)
        self.bias = rs.standard_normal((Q, self.P)).astype(np.float32) if p.get("bias") else None
        s = mg.restate_metric_scores(self.T, self.w, self.codes, self.metric)
        if self.bias is not None:
            s = bg.biased_scores(mg.restate_sums(self.T, self.codes), self.offs, self.probes, self.bias, self.w, self.metric)
        self.s = s
        self.range = self.fill_e is not None
        if self.range:
            with np.errstate(invalid="ignore"):
                self.thr = np.nanquantile(s.astype(np.float64), 0.2, axis=1).astype(np.float32)
            self.want = self._restate_range()
            self.total = int(self.want[0][-1])
            assert self.total > 0
        else:
            self.want = self._restate_topk()
        d = self.d = dict(T=_dev(self.T), codes=_dev(self.codes.view(np.int16) if p.get("u16") else self.codes), w=_dev(self.w),
                          mask=None if self.keep is None else _dev(kg.pack(self.keep)),
                          offs=None if self.offs is None else _dev(self.offs), probes=None if self.probes is None else _dev(self.probes),
                          bias=None if self.bias is None else _dev(self.bias), thr=_dev(self.thr) if self.range else None)
        self.consts = [t for t in d.values() if t is not None]
        self.need = size_query(L, row)

    # ---- the independent answers
    def _restate_topk(self):
        if self.P:
            return lg.restate_lists(self.s, self.offs, self.probes, self.k, self.keep)
        if self.e in ("mcq_search_wide", "mcq_search_topk_u16"):
            return wg.restate_topk_valid(self.s, self.k, self.keep)
        if self.keep is not None:
            return kg.restate_topk_masked(self.s, self.keep, self.k)
        if self.e == "mcq_search_scan":
            return sg.restate(self.T, self.w, self.codes, self.k)
        return mg.restate_metric(self.T, self.w, self.codes, self.k, self.metric)

    def _restate_range(self):
        if self.P and self.bias is not None:
            S = mg.restate_sums(self.T, self.codes)
            return bg.restate_range_lists_bias(S, self.offs, self.probes, self.bias, self.w, self.metric, self.thr, self.keep)
        if self.P:
            return rl.restate_range_lists(self.s, self.offs, self.probes, self.thr, self.keep)
        if self.keep is not None:
            return kg.restate_range_masked(self.s, self.keep, self.thr)
        _, lims, pos, val = rg.restate(self.T, self.w, self.codes, self.metric, thr=self.thr)
        return lims, pos, val

    # ---- the call
    SPARE = 7                                                # slots of a range result past lims[Q]: inside capacity, never written

    def outputs(self):
        if self.range:
            n = self.total + self.SPARE
            return [ar.guarded((self.Q + 1,), torch.int64), ar.guarded((n,), torch.float32), ar.guarded((n,), torch.int64)]
        return [ar.guarded((self.Q, self.k), torch.float32), ar.guarded((self.Q, self.k), torch.int64)]

    def _head(self, B, Q):
        d = self.d
        return (d["T"].data_ptr(), Q, d["codes"].data_ptr(), d["w"].data_ptr(), B, self.N, self.K)

    def _middle(self):
        """the operands between the metric and the outputs, as the entry takes them"""
        d, e = self.d, self.e
        lists = (_ptr(d["offs"]), 0 if self.offs is None else len(self.offs) - 1, _ptr(d["probes"]), self.P or 1)
        if e in ("mcq_search_scan", "mcq_search_scan_metric", "mcq_search_range_count"):
            return ()
        if e in ("mcq_search_scan_masked", "mcq_search_range_count_masked", "mcq_search_wide"):
            return (_ptr(d["mask"]),)
        if e in ("mcq_search_scan_lists", "mcq_search_range_lists_count"):
            return (_ptr(d["mask"]),) + lists
        return (_ptr(d["mask"]),) + lists + (_ptr(d["bias"]),)

    def call(self, L, ws, nbytes, outs, B=None, Q=None):
        head = self._head(self.B if B is None else B, self.Q if Q is None else Q)
        code = mg.CODE[self.metric]
        if not self.range:
            metric = () if self.e == "mcq_search_scan" else (code,)
            return getattr(L, self.e)(*head, self.k, *metric, *self._middle(), outs[0].ptr, outs[1].ptr, ws, nbytes, _st())
        thr = self.d["thr"].data_ptr()
        rc = getattr(L, self.e)(*head, code, *self._middle(), thr, outs[0].ptr, ws, nbytes, _st())
        if rc:
            return rc
        return getattr(L, self.fill_e)(*head, code, *self._middle(), thr, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                       self.total + self.SPARE, ws, nbytes, _st())

    def verify(self, outs):
        if self.range:
            lims, pos, val = self.want
            assert np.array_equal(outs[0].t.cpu().numpy(), lims), "lims differ from rule 8"
            assert np.array_equal(outs[2].t.cpu().numpy()[:self.total], pos), "positions differ"
            assert np.array_equal(outs[1].t.cpu().numpy()[:self.total].view(np.uint32), val.view(np.uint32)), "scores differ"
        else:
            assert np.array_equal(outs[1].t.cpu().numpy(), self.want[1]), "positions differ from the restatement"
            assert np.array_equal(outs[0].t.cpu().numpy().view(np.uint32), self.want[0].view(np.uint32)), "scores differ"

    def extent(self, outs):
        if self.range:
            spare = torch.arange(self.total + self.SPARE) >= self.total
            assert outs[1].untouched(spare) and outs[2].untouched(spare), "fill wrote past lims[Q]"

    def empty(self, L, arena):
        """B == 0, then Q == 0 (rules 5, 9, 16 and 19) -> every output block of the two calls"""
        both = []
        for B, Q in ((0, None), (None, 0)):
            outs = self.outputs()
            with ar.frozen(*self.consts):
                rc = self.call(L, arena.ptr, arena.bytes, outs, B=B, Q=Q)
                torch.cuda.synchronize()
            assert rc == 0, (rc, B, Q)
            if self.range and Q == 0:                        # lims is int64[Q + 1]: its one element, zero
                rest = torch.arange(self.Q + 1) >= 1
                assert int(outs[0].t[0]) == 0 and outs[0].untouched(rest) and outs[1].untouched() and outs[2].untouched(), "Q == 0: lims[0]"
            elif self.range:
                assert not bool(outs[0].t.any()) and outs[1].untouched() and outs[2].untouched(), "an empty range call: lims only"
            elif Q == 0:
                assert outs[0].untouched() and outs[1].untouched(), "no query: no row of the outputs is written"
            else:
                assert bool(torch.isposinf(outs[0].t).all()) and bool((outs[1].t == -1).all()), "an empty store: (+inf, -1)"
            both += outs
        return both


class ShortlistJob(Job):
    """mcq_search_shortlist(_u16) and mcq_rerank: a shortlist per query with -1 entries, entries past the store and duplicates"""

    def __init__(self, L, row):
        p = self.p = row.p
        self.rerank = row.kind == "rerank"
        Q, B, S, k = p["Q"], p["B"], p["S"], p["k"]
        self.Q, self.B, self.S, self.k, self.metric = Q, B, S, k, p["metric"]
        rs = np.random.RandomState(77 + Q + B + S + k)
        Bs = B + 5 if p.get("row_of") else B
        self.short = rs.randint(-2, Bs + 2, size=(Q, S)).astype(np.int64)
        self.short[0, :2] = self.short[0, 2]                  # a duplicate
        self.row_of = rs.randint(-1, B + 1, size=Bs).astype(np.int64) if p.get("row_of") else None
        if self.rerank:
            self.q = rs.standard_normal((Q, p["D"])).astype(np.float32)
            self.X = rs.standard_normal((B, p["D"])).astype(np.float32)
            self.want = rr.restate(self.q, self.X, self.short, k, self.metric, self.row_of)[:2]
            host = dict(q=self.q, X=self.X)
        else:
            N, K = p["NK"]
            self.N, self.K = N, K
            self.T = rs.standard_normal((Q, N, K)).astype(np.float32)
            self.codes = rs.randint(0, K, size=(B, N)).astype(np.uint16 if p.get("u16") else np.uint8)
            self.w = (rs.rand(B) + 0.5).astype(np.float32)
            self.bias = rs.standard_normal((Q, S)).astype(np.float32) if p.get("bias") else None
            self.want = hg.restate(self.T, self.w, self.codes, self.short, k, self.metric, self.row_of, self.bias)[:2]
            host = dict(T=self.T, codes=self.codes.view(np.int16) if p.get("u16") else self.codes, w=self.w, bias=self.bias)
        host.update(short=self.short, row_of=self.row_of)
        self.d = {n: None if a is None else _dev(a) for n, a in host.items()}
        self.consts = [t for t in self.d.values() if t is not None]
        self.need = size_query(L, row)

    def outputs(self):
        return [ar.guarded((self.Q, self.k), torch.float32), ar.guarded((self.Q, self.k), torch.int64)]

    def call(self, L, ws, nbytes, outs, Q=None, S=None, B=None, Bs=None):
        d, Q, S, B = self.d, self.Q if Q is None else Q, self.S if S is None else S, self.B if B is None else B
        nrow = (0 if self.row_of is None else len(self.row_of)) if Bs is None else Bs
        code = mg.CODE[self.metric]
        if self.rerank:
            return L.mcq_rerank(d["q"].data_ptr(), 0, Q, d["X"].data_ptr(), 0, B, self.p["D"], d["short"].data_ptr(), S,
                                _ptr(d["row_of"]), nrow, self.k, code, outs[0].ptr, outs[1].ptr, ws, nbytes, _st())
        return getattr(L, self.p["entry"])(d["T"].data_ptr(), Q, d["codes"].data_ptr(), d["w"].data_ptr(), B, self.N, self.K, self.k,
                                           code, d["short"].data_ptr(), S, _ptr(d["row_of"]), nrow, _ptr(d["bias"]),
                                           outs[0].ptr, outs[1].ptr, ws, nbytes, _st())

    def verify(self, outs):
        assert np.array_equal(outs[1].t.cpu().numpy(), self.want[1]), "positions differ from the restatement"
        assert np.array_equal(outs[0].t.cpu().numpy().view(np.uint32), self.want[0].view(np.uint32)), "scores differ"

    def empty(self, L, arena):
        """Q == 0 does nothing; S, B or (with row_of) Bs == 0 writes (+inf, -1) (rules 28 and 36) -> every output block"""
        every = []
        cases = [dict(Q=0), dict(S=0), dict(B=0)] + ([dict(Bs=0)] if self.row_of is not None else [])
        for kw in cases:
            outs = self.outputs()
            with ar.frozen(*self.consts):
                rc = self.call(L, arena.ptr, arena.bytes, outs, **kw)
                torch.cuda.synchronize()
            assert rc == 0, (rc, kw)
            if "Q" in kw:
                assert outs[0].untouched() and outs[1].untouched(), "Q == 0 does nothing"
            else:
                assert bool(torch.isposinf(outs[0].t).all()) and bool((outs[1].t == -1).all()), (kw, "no candidate: (+inf, -1)")
            every += outs
        return every


_STATES = {}


def _state(N, K, D, B):
    """per shape, once: state, quantizer, oracle, prepared blob and 700 frames on host and device (the first B are used)"""
    from golden import gen
    from test_gpu_parity import load_quantizer, oracle_of
    if (N, K, D) not in _STATES:
        sd = gen.synthetic_state(5200 + N + K + D, D, K, N)
        x = gen.make_gaussian(5201 + N + K + D, 700, D)
        q = load_quantizer(sd, D, K, N)
        with torch.no_grad():
            blob = q._prepared()
        _STATES[(N, K, D)] = dict(q=q, o=oracle_of(sd), x=x, xd=_dev(x), blob=blob, ref={})
    assert B <= 700
    return _STATES[(N, K, D)]


class EncodeJob(Job):
    """mcq_encode, mcq_encode_ex, mcq_refine_indexes, mcq_logits_refine(_codes) against the oracle's codes and logits"""

    def __init__(self, L, row):
        p = self.p = row.p
        self.row, self.e = row, p["entry"]
        (N, K, D), B = p["NKD"], p["B"]
        self.N, self.K, self.D, self.B, self.iters, self.flags = N, K, D, B, p["iters"], p.get("flags", 0)
        c = self.c = _state(N, K, D, B)
        x = c["x"][:B]
        self.xd = c["xd"][:B].contiguous()
        if self.flags & X_FP16:
            self.xd = self.xd.half().contiguous()
            x = self.xd.float().cpu().numpy()
        self.x, self.i64 = x, bool(p.get("i64")) or self.e != "mcq_encode" and self.e != "mcq_encode_ex"
        self.pack = 2 if (not self.i64 and K == 16 and N >= 2) else 1
        self.start = None
        if self.e == "mcq_refine_indexes":
            self.start = np.random.RandomState(3 + N + K).randint(0, K, size=(B, N)).astype(np.int64)
            self.start_d = _dev(self.start)
        self.consts = [self.xd, c["blob"]] + ([self.start_d] if self.start is not None else [])
        self.need = size_query(L, row)
        self.refuse = smallest_encode_workspace(L, row) - 1
        self.want_lanes = row.claims["lanes"]

    def outputs(self):
        B, N, K = self.B, self.N, self.K
        if self.e in ("mcq_encode", "mcq_encode_ex"):
            return [ar.guarded((B, N), torch.int64) if self.i64 else ar.guarded((B, N // self.pack), torch.uint8)]
        if self.e == "mcq_refine_indexes":
            return [ar.guarded((B, N), torch.int64)]
        outs = [ar.guarded((B, N * K), torch.float32), ar.guarded((B, N), torch.int64)]
        return outs + ([ar.guarded((B, N), torch.uint8)] if self.e == "mcq_logits_refine_codes" else [])

    def call(self, L, ws, nbytes, outs, B=None, flags=0):
        B = self.B if B is None else B
        q, c, N, K, D = self.c["q"], self.c, self.N, self.K, self.D
        head = (self.xd.data_ptr(), B, c["blob"].data_ptr())
        flags |= self.flags | q._scale_flags
        if self.e == "mcq_encode":
            assert q._scale_flags == 0
            rc = L.mcq_encode(*head, q._lscale_exp, N, K, D, self.iters, None if self.i64 else outs[0].ptr,
                              outs[0].ptr if self.i64 else None, ws, nbytes, _st())
        elif self.e == "mcq_encode_ex":
            rc = L.mcq_encode_ex(*head, q._lscale_exp, N, K, D, self.iters, None if self.i64 else outs[0].ptr,
                                 outs[0].ptr if self.i64 else None, ws, nbytes, _st(), flags)
        elif self.e == "mcq_refine_indexes":
            rc = L.mcq_refine_indexes(*head, N, K, D, self.iters, self.start_d.data_ptr(), outs[0].ptr, ws, nbytes, _st())
        elif self.e == "mcq_logits_refine":
            rc = L.mcq_logits_refine(*head, q._lscale_exp, N, K, D, self.iters, outs[0].ptr, outs[1].ptr, ws, nbytes, _st(), flags)
        else:
            rc = L.mcq_logits_refine_codes(*head, q._lscale_exp, N, K, D, self.iters, outs[0].ptr, outs[1].ptr, outs[2].ptr, ws,
                                           nbytes, _st(), flags)
        if rc == 0 and B > 0 and self.e in ("mcq_encode", "mcq_encode_ex"):
            self.launches = L.mcq_last_encode_launches()       # (of the call just made, on this thread)
            assert L.mcq_last_encode_lanes() == self.want_lanes, (L.mcq_last_encode_lanes(), self.want_lanes)
        return rc

    def _codes(self):
        """the oracle's indexes (B, N) int64, once per (state, frames, passes)"""
        key = ("idx", self.iters, bool(self.flags & X_FP16), self.B, self.e == "mcq_refine_indexes")
        ref = self.c["ref"]
        if key not in ref:
            o = self.c["o"]
            if self.start is None:
                ref[key] = o.compute_indexes(self.x, self.iters).astype(np.int64)
            else:
                idx = self.start.copy()
                for _ in range(self.iters):
                    idx = np.stack([o.refine_trace(self.x[b], idx[b])["idx"] for b in range(self.B)]).astype(np.int64)
                ref[key] = idx
        return ref[key]

    def verify(self, outs):
        want = self._codes()
        if self.e in ("mcq_encode", "mcq_encode_ex") and not self.i64:
            got = outs[0].t.cpu().numpy()
            if self.pack == 2:
                got = np.stack([got & 15, got >> 4], axis=2).reshape(self.B, self.N)
            assert np.array_equal(got.astype(np.int64), want), "codes differ from the oracle's"
            return
        if self.e in ("mcq_encode", "mcq_encode_ex", "mcq_refine_indexes"):
            assert np.array_equal(outs[0].t.cpu().numpy(), want), "indexes differ from the oracle's"
            return
        assert np.array_equal(outs[0].t.cpu().numpy().view(np.uint32), self.c["o"].logits(self.x).view(np.uint32)), "logits"
        assert np.array_equal(outs[1].t.cpu().numpy(), want), "indexes differ from the oracle's"
        if len(outs) == 3:
            assert np.array_equal(outs[2].t.cpu().numpy().astype(np.int64), want), "byte codes differ from the indexes"

    def empty(self, L, arena):
        outs = self.outputs()
        with ar.frozen(*self.consts):
            rc = self.call(L, arena.ptr, arena.bytes, outs, B=0)
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert all(o.untouched() for o in outs), "B == 0 wrote an output"
        return outs


class LogitsJob(Job):
    """mcq_logits, mcq_logits_argmax (the oracle's logits, bit for bit, and their first maximum) and the probes mcq_test_xc, mcq_test_xc_xx"""

    def __init__(self, L, row):
        p = self.p = row.p
        (N, K, D), B = p["NKD"], p["B"]
        self.e, self.N, self.K, self.D, self.B = p["entry"], N, K, D, B
        self.c = _state(N, K, D, B)
        self.xd = self.c["xd"][:B].contiguous()
        self.consts = [self.xd, self.c["blob"]]
        self.need = size_query(L, row)

    def outputs(self):
        outs = [ar.guarded((self.B, self.N * self.K), torch.float32)]
        if self.e == "mcq_test_xc_xx":
            return outs + [ar.guarded((self.B,), torch.float32)]
        return outs + ([ar.guarded((self.B, self.N), torch.int64)] if self.e == "mcq_logits_argmax" else [])

    def call(self, L, ws, nbytes, outs, B=None):
        B = self.B if B is None else B
        q, N, K, D = self.c["q"], self.N, self.K, self.D
        head = (self.xd.data_ptr(), B, self.c["blob"].data_ptr())
        if self.e == "mcq_test_xc":
            return L.mcq_test_xc(*head, N, K, D, outs[0].ptr, ws, nbytes, _st(), 0)
        if self.e == "mcq_test_xc_xx":
            return L.mcq_test_xc_xx(*head, N, K, D, outs[0].ptr, outs[1].ptr, ws, nbytes, _st(), 0)
        if self.e == "mcq_logits":
            assert q._scale_flags == 0
            return L.mcq_logits(*head, q._lscale_exp, N, K, D, outs[0].ptr, ws, nbytes, _st())
        return L.mcq_logits_argmax(*head, q._lscale_exp, N, K, D, outs[0].ptr, outs[1].ptr, ws, nbytes, _st(), q._scale_flags)

    def verify(self, outs):
        want = self.c["o"].logits(self.c["x"][:self.B])
        assert np.array_equal(outs[0].t.cpu().numpy().view(np.uint32), want.view(np.uint32)), "logits differ from the oracle's"
        if len(outs) == 2:
            first = want.reshape(self.B, self.N, self.K).argmax(axis=2)              # numpy: the first maximum
            assert np.array_equal(outs[1].t.cpu().numpy(), first), "the arg max is not the first maximum"

    def empty(self, L, arena):
        outs = self.outputs()
        with ar.frozen(*self.consts):
            rc = self.call(L, arena.ptr, arena.bytes, outs, B=0)
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert all(o.untouched() for o in outs), "B == 0 wrote an output"
        return outs


class ProbeJob(Job):
    """mcq_test_er (both forms; in form 1 the Gram terms go through the workspace), mcq_test_pass and mcq_test_pass16: invariance and bounds"""

    def __init__(self, L, row):
        p = self.p = row.p
        (N, K, D), B = p["NKD"], p["B"]
        self.kind, self.N, self.K, self.D, self.B = row.kind, N, K, D, B
        c = self.c = _state(N, K, D, B)
        self.xd = c["xd"][:B].contiguous()
        rs = np.random.RandomState(9 + N + K + B)
        self.consts = [self.xd, c["blob"]]
        if self.kind == "er":
            self.xc = torch.empty((B, N * K), dtype=torch.float32, device="cuda:0")
            self.xx = torch.empty(B, dtype=torch.float32, device="cuda:0")
            nws = L.mcq_logits_workspace_bytes(B, N, D)
            ws = torch.empty(nws, dtype=torch.uint8, device="cuda:0")
            rc = L.mcq_test_xc_xx(self.xd.data_ptr(), B, c["blob"].data_ptr(), N, K, D, self.xc.data_ptr(), self.xx.data_ptr(),
                                  ws.data_ptr(), nws, _st(), 0)
            assert rc == 0, rc
            torch.cuda.synchronize()
            self.idx = _dev(rs.randint(0, K, size=(B, N)).astype(np.uint8))
            assert self.idx.data_ptr() % 16 == 0
            self.consts = [c["blob"], self.xc, self.xx, self.idx]
        else:
            self.idx = _dev(rs.randint(0, K, size=(B, N)).astype(np.int64))
            self.consts.append(self.idx)
        self.need = size_query(L, row)

    def outputs(self):
        if self.kind == "er":
            return [ar.guarded((self.B,), torch.float32), ar.guarded((self.B, self.N), torch.float32)]
        return [ar.guarded((self.B, self.N), torch.int64)]

    def call(self, L, ws, nbytes, outs):
        c, N, K, D, B = self.c, self.N, self.K, self.D, self.B
        if self.kind == "er":
            return L.mcq_test_er(c["blob"].data_ptr(), N, K, D, self.xc.data_ptr(), self.xx.data_ptr(), self.idx.data_ptr(), B, None,
                                 None, self.p["form"], outs[0].ptr, outs[1].ptr, ws, nbytes, _st())
        if self.kind == "pass":
            return L.mcq_test_pass(self.xd.data_ptr(), B, c["blob"].data_ptr(), N, K, D, self.idx.data_ptr(), outs[0].ptr, None, None,
                                   self.p["flags"], ws, nbytes, _st())
        return L.mcq_test_pass16(self.xd.data_ptr(), B, c["blob"].data_ptr(), N, D, self.p["iters"], self.idx.data_ptr(), outs[0].ptr,
                                 None, 0, 0, ws, nbytes, _st())


class TrainJob(Job):
    """mcq_loss_fwd and mcq_weight_grad against float64 within the bounds of tests/test_gpu_train_kernels.py"""

    def __init__(self, L, row):
        import test_gpu_train_kernels as tk
        p = self.p = row.p
        self.kind, self.tk = row.kind, tk
        dev = torch.device("cuda:0")
        if self.kind == "loss":
            N, K, B = p["N"], p["K"], p["B"]
            gen = torch.Generator(device="cuda:0").manual_seed(1000 * K + 7 * N + B)
            self.z, self.idx = tk._logits(B, N, K, "trained", gen)
            self.consts = [self.z, self.idx]
        else:
            B, M, D = p["B"], p["M"], p["D"]
            gen = torch.Generator(device="cuda:0").manual_seed(B + 7 * M + 13 * D)
            colscale = torch.pow(2.0, -100.0 * torch.arange(M, device=dev) / max(M - 1, 1))
            self.G = (torch.randn(B, M, device=dev, generator=gen) * colscale).contiguous()
            self.x = (torch.randn(B, D, device=dev, generator=gen) + 100.0).contiguous()
            self.s = torch.tensor([0.8], device=dev)
            self.consts = [self.G, self.x, self.s]
        self.need = size_query(L, row)

    def outputs(self):
        p = self.p
        if self.kind == "loss":
            return [ar.guarded((p["B"], p["N"]), torch.float32), ar.guarded((p["N"],), torch.float32),
                    ar.guarded((p["N"], p["K"]), torch.float32), ar.guarded((p["N"], p["K"]), torch.float32)]
        return [ar.guarded((p["M"], p["D"]), torch.float32), ar.guarded((p["M"],), torch.float32)]

    def call(self, L, ws, nbytes, outs):
        p = self.p
        if self.kind == "loss":
            return L.mcq_loss_fwd(self.z.data_ptr(), self.idx.data_ptr(), p["B"], p["N"], p["K"], outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                  outs[3].ptr, ws, nbytes, _st())
        return L.mcq_weight_grad(self.G.data_ptr(), self.x.data_ptr(), p["B"], p["M"], p["D"], self.s.data_ptr(), outs[0].ptr,
                                 outs[1].ptr, ws, nbytes, _st())

    def verify(self, outs):
        got = [o.t.clone() for o in outs]
        if self.kind == "loss":
            self.tk.hold_loss_fwd(self.z, self.idx, *got)
        else:
            self.tk.hold_weight_grad(self.G, self.x, self.s, *got)


JOBS = {"search": SearchJob, "shortlist": ShortlistJob, "rerank": ShortlistJob, "encode": EncodeJob, "logits": LogitsJob,
        "er": ProbeJob, "pass": ProbeJob, "pass16": ProbeJob, "loss": TrainJob, "wgrad": TrainJob}
# what stays on the device between rows: the state of a shape (_STATES), and of the workspaces only the leftovers that a later
# row still takes (_LEFT, dropped after their last user); a row's Job lives for that row
_JOB, _LEFT = {}, {}
_USERS = {}
for _r in ROWS:
    _USERS[_r.donor] = _USERS.get(_r.donor, 0) + 1


def _job(L, row):
    if row.id not in _JOB:
        with hooks(row.env):
            _JOB[row.id] = JOBS[row.kind](L, row)
    return _JOB[row.id]


# ================================================================== the runs
def _run(L, row, job, fill, what, **kw):
    """one valid call on an exactly sized, guarded workspace -> (arena, outputs); (c) is asserted here"""
    arena, outs = ar.Arena(job.need, fill), job.outputs()
    with hooks(row.env), ar.frozen(*job.consts):
        rc = job.call(L, arena.ptr, arena.bytes, outs, **kw)
        torch.cuda.synchronize()
    assert rc == 0, (row.id, what, rc)
    assert arena.damage() is None, (row.id, what, "a guard of the workspace was written at", arena.damage(), "of", job.need)
    for i, o in enumerate(outs):
        assert o.damage() is None, (row.id, what, f"a guard of output {i} was written at", o.damage(), "of", o.extent)
    job.extent(outs)
    return arena, outs


def _leftover(L, row):
    """the workspace of the donor row as its clean run left it"""
    donor = BY_ID[row.donor]
    if donor.id not in _LEFT:
        arena, _ = _run(L, donor, _job(L, donor), "zeros", "the donor's clean run")
        _LEFT[donor.id] = arena.region.clone()
        _JOB.pop(donor.id, None)
    left = _LEFT[donor.id]
    _USERS[donor.id] -= 1
    if _USERS[donor.id] <= 0:
        del _LEFT[donor.id]
    return left


@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_row(row):
    _lib, L = _mods()
    with torch.no_grad():
        job = _job(L, row)
        assert claims_hold(L, row) == job.need and job.need >= 256
        # a. the clean run
        arena, clean = _run(L, row, job, "zeros", "zeros")
        if "a" in row.checks:
            job.verify(clean)
        if _USERS.get(row.id, 0) > 0:
            _LEFT.setdefault(row.id, arena.region.clone())
        bits = [o.bits() for o in clean]
        if row.claims.get("skips"):                          # the skipping path was taken: not the launches of every pass on every vector
            took = job.launches
            _run(L, row, job, "zeros", "all passes", flags=ALL_PASSES)
            assert job.launches != took, (row.id, took, "launches with and without MCQ_ENCODE_ALL_PASSES")
        # b. the same bits whatever the workspace held
        for name, fill in (("ones", "ones"), ("a5", "a5"), ("leftover", _leftover(L, row))):
            _, outs = _run(L, row, job, fill, name)
            for i, (o, was) in enumerate(zip(outs, bits)):
                assert torch.equal(o.bits(), was), (row.id, f"output {i} on a workspace of `{name}` differs from the clean run's")
        # d. one byte less is refused before anything is touched
        if "d" in row.checks:
            short = job.need - 1 if job.refuse is None else job.refuse
            arena, outs = ar.Arena(short, "a5"), job.outputs()
            with hooks(row.env), ar.frozen(*job.consts):
                rc = job.call(L, arena.ptr, arena.bytes, outs)
                torch.cuda.synchronize()
            assert rc == _lib.MCQ_EWORKSPACE, (row.id, rc)
            assert arena.untouched() and arena.damage() is None and all(o.untouched() and o.damage() is None for o in outs), row.id
        # e. the empty call
        if "e" in row.checks:
            arena = ar.Arena(job.need, "a5")
            with hooks(row.env):
                outs = job.empty(L, arena)
            assert outs is not None, (row.id, "the header defines an empty call for this entry")
            assert arena.untouched() and arena.damage() is None and all(o.damage() is None for o in outs), row.id
    _JOB.pop(row.id, None)
