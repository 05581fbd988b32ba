"""The search over a store of two-byte codes (codebook_size 1,024; include/mcq_code16.h) against the only path a user of wide
codebooks had before it, and against the one-byte calls of a 256-entry quantizer as orientation.  Writes one JSON line per cell
to profiles/search_code16.jsonl (--out).

Shape: 1,048,576 stored codes, dim 512, 8 x 1,024 (synthetic_state(103, ...)), kept in the order of the 1,024 toy lists of
tools/exp_search_lists.py (a random sample of decoded vectors and a few Lloyd steps), L2.
Cells: Q in --queries x {search(k=10), search_wide(k=100), search_wide(k=1,024), search_lists_wide(k=100) at 8 probes,
range_search at the radius of each query's 10th neighbour}.  Per cell, timed in ONE process, alternated, --runs runs of --reps
calls each after two warm-up calls (wall clock round a device synchronise); each contender's line holds every run, their
median, min .. max, and the peak of device memory the call allocated beyond what was held before it:
  code16  : the call on the int16 store of pack_codes
  matmul  : (whole store) decode(int64 digits) + matmul + torch.topk(k) on the same quantizer -- the parent's only path, and it
            runs the parent's code; for the range cell a comparison and nonzero in place of the topk
  byte256 : the same call of an 8 x 256 quantizer on a one-byte store of the same length: what the second byte and the four
            times larger table cost beside it (another quantizer, other codes: orientation, not a ratio to hold)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from exp_search_lists import timed, toy_centroids
from quantization_amd import Quantizer, build_lists, probe_lists
from quantization_amd import synthetic as gen


def quantizer(D, K, N):
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for name, v in gen.synthetic_state(103, D, K, N).items():
        sd[name] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    return q.cuda().requires_grad_(False)


def store_of(q, B, L, lloyd, rs, random_codes):
    """(the store in list order as the searches take it, the int64 digits in the same order, centroids, list_offsets, norms)"""
    D, K, N = q.dim, q.codebook_size, q.num_codebooks
    if random_codes:
        digits = torch.randint(0, K, (B, N), device="cuda")
    else:
        digits = torch.cat([q.encode(torch.from_numpy(gen.make_gaussian(8 + a, min(65536, B - a), D)).cuda(), as_bytes=False)
                            for a in range(0, B, 65536)])
    cen = toy_centroids(q, digits, L, lloyd, rs)
    assign = torch.cat([torch.cdist(q.decode(digits[a:a + 65536]), cen).argmin(dim=1) for a in range(0, B, 65536)])
    order, off = build_lists(assign, L)
    digits = digits[order].contiguous()
    store = q.pack_codes(digits)
    return store, digits, cen, off, q.code_norms(store)


def measured(fs, runs, reps):
    """{name: fn} -> ({name: [ms per run]}, {name: peak extra bytes}, {name: last result}), the contenders alternated"""
    ts, peak, outs = {name: [] for name in fs}, {}, {}
    for name, f in fs.items():
        f()
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        f()
        torch.cuda.synchronize()
        peak[name] = int(torch.cuda.max_memory_allocated() - held)
    for _ in range(runs):
        for name, f in fs.items():
            ms, outs[name] = timed(f, reps)
            ts[name].append(round(ms, 4))
    return ts, peak, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--lloyd", type=int, default=5)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_code16.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "exp_search_code16.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    D, N, B, L = 512, 8, args.store, args.lists
    out = open(args.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    with torch.no_grad():
        q16, q8 = quantizer(D, 1024, N), quantizer(D, 256, N)
        s16, digits, cen16, off16, norms16 = store_of(q16, B, L, args.lloyd, np.random.RandomState(5), args.random_codes)
        s8, _, cen8, off8, norms8 = store_of(q8, B, L, args.lloyd, np.random.RandomState(5), args.random_codes)
        assert s16.dtype == torch.int16 and s8.dtype == torch.uint8
        emit({"B": B, "lists": L, "dim": D, "codebooks": N, "codebook_size": 1024, "orientation_codebook_size": 256,
              "runs": args.runs, "reps": args.reps, "random_codes": bool(args.random_codes),
              "store_bytes": {"int16": s16.numel() * 2, "int64_digits": digits.numel() * 8, "uint8_256": s8.numel()}})
        for Q in args.queries:
            xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
            p16, p8 = probe_lists(xq, cen16, args.nprobe), probe_lists(xq, cen8, args.nprobe)
            r16 = q16.search(xq, s16, k=10, norms=norms16)[0][:, -1].contiguous()      # the 10th neighbour: about 10 hits
            r8 = q8.search(xq, s8, k=10, norms=norms8)[0][:, -1].contiguous()
            qq = (xq * xq).sum(dim=1, keepdim=True)

            def matmul_topk(k):
                dec = q16.decode(digits)
                s = norms16[None, :] - 2.0 * (xq @ dec.T)
                v, i = torch.topk(s, k, dim=1, largest=False)
                return v + qq, i

            def matmul_range():
                dec = q16.decode(digits)
                s = norms16[None, :] - 2.0 * (xq @ dec.T) + qq
                hit = torch.nonzero(s <= r16[:, None])
                return hit, s[hit[:, 0], hit[:, 1]]

            cells = {
                "search_k10": {"code16": lambda: q16.search(xq, s16, k=10, norms=norms16),
                               "matmul": lambda: matmul_topk(10),
                               "byte256": lambda: q8.search(xq, s8, k=10, norms=norms8)},
                "search_wide_k100": {"code16": lambda: q16.search_wide(xq, s16, 100, norms=norms16),
                                     "matmul": lambda: matmul_topk(100),
                                     "byte256": lambda: q8.search_wide(xq, s8, 100, norms=norms8)},
                "search_wide_k1024": {"code16": lambda: q16.search_wide(xq, s16, 1024, norms=norms16),
                                      "matmul": lambda: matmul_topk(1024),
                                      "byte256": lambda: q8.search_wide(xq, s8, 1024, norms=norms8)},
                f"search_lists_wide_k100_p{args.nprobe}": {
                    "code16": lambda: q16.search_lists_wide(xq, s16, off16, p16, 100, norms=norms16),
                    "byte256": lambda: q8.search_lists_wide(xq, s8, off8, p8, 100, norms=norms8)},
                "range_search_10_hits": {"code16": lambda: q16.range_search(xq, s16, r16, norms=norms16),
                                         "matmul": matmul_range,
                                         "byte256": lambda: q8.range_search(xq, s8, r8, norms=norms8)},
            }
            for call, fs in cells.items():
                ts, peak, outs = measured(fs, args.runs, args.reps)
                line = {"Q": Q, "call": call, "B": B, "ms": ts,
                        "median_ms": {name: float(np.median(v)) for name, v in ts.items()},
                        "min_max_ms": {name: [min(v), max(v)] for name, v in ts.items()},
                        "peak_extra_bytes": peak}
                if "matmul" in fs:
                    line["matmul_over_code16"] = round(line["median_ms"]["matmul"] / line["median_ms"]["code16"], 2)
                line["code16_over_byte256"] = round(line["median_ms"]["code16"] / line["median_ms"]["byte256"], 3)
                if call.startswith("range"):
                    n = outs["code16"][0][1:] - outs["code16"][0][:-1]
                    line["hits_min_max"] = [int(n.min()), int(n.max())]
                elif "matmul" in fs:                                    # the same neighbours, but for fp32 near-ties
                    line["positions_equal_matmul"] = float((outs["code16"][1] == outs["matmul"][1]).float().mean())
                emit(line)
    out.close()


if __name__ == "__main__":
    main()
