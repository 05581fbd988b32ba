"""Search under a mask against what a user had before it: gather the kept codes into a second store, search that, map back.

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), k = 10, 64 queries, the three
metrics (--store / --queries / --metrics change them); the range search lists what lies within the 10th value of the unmasked
top-k of each query.  Mask patterns (tests/search_mask_grid.py has the same ones): all, half (random 50 %), sparse (random
1 %: about half the steps of 64 still hold a candidate), run (one contiguous 1 %: almost no step does).
Variants, timed in ONE process, alternated, --runs runs of --reps calls each (warmed, wall clock round a device synchronise):
  unmasked : search / range_search without a mask                                       (per metric, once)
  masked   : search / range_search with mask = the packed words (pack_mask outside the timed region: a store keeps them)
  gather   : pos = nonzero(keep); search / range_search over codes[pos], norms[pos] or rnorms[pos]; positions through pos.
             The gather is inside the timed region: it is what every distinct filter costs.
Prints one JSON line per (metric, call, pattern): the times, masked against unmasked and against gather, whether masked and
gather returned the same bits, and the peak extra device memory of one call of each (torch.cuda.max_memory_allocated).
--only unmasked times the unmasked calls alone and prints one line per (metric, call): run it once per build under comparison
(MCQ_ALLOW_LIB_PATH=1 MCQ_LIB_PATH=<an older libmcq_hip.so> for the other one), alternating the processes."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from quantization_amd import Quantizer
from quantization_amd import synthetic as gen


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def keep_for(pattern, B, rs):
    keep = np.zeros(B, dtype=bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "half":
        keep = rs.rand(B) < 0.5
    elif pattern == "sparse":
        keep = rs.rand(B) < 0.01
    else:
        n = max(1, B // 100)
        a = rs.randint(B - n + 1)
        keep[a:a + n] = True
    return keep


def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--metrics", nargs="*", default=["l2", "ip", "cosine"])
    ap.add_argument("--patterns", nargs="*", default=["all", "half", "sparse", "run"])
    ap.add_argument("--only", choices=["unmasked"], default=None)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="", help="copied into every line (which build this process timed)")
    args = ap.parse_args()
    D, K, N, B, Q, k = 512, 256, 8, args.store, args.queries, 10
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for name, v in gen.synthetic_state(103, D, K, N).items():
        sd[name] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    q = q.cuda().requires_grad_(False)
    rs = np.random.RandomState(5)
    with torch.no_grad():
        if args.random_codes:
            codes = torch.randint(0, K, (B, N), dtype=torch.uint8, device="cuda")
        else:
            codes = torch.cat([q.encode(torch.from_numpy(gen.make_gaussian(8 + a, min(65536, B - a), D)).cuda())
                               for a in range(0, B, 65536)])
        norms = q.code_norms(codes)
        rnorms = q.rnorms_from_norms(norms)
        xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
        for metric in args.metrics:
            kw = dict(norms=norms, rnorms=rnorms, metric=metric)
            radius = q.search(xq, codes, k=k, **kw)[0][:, k - 1].contiguous()
            plain = {"topk": lambda: q.search(xq, codes, k=k, **kw), "range": lambda: q.range_search(xq, codes, radius, **kw)}
            for f in plain.values():
                for _ in range(3):
                    f()
            if args.only == "unmasked":
                ts = {name: [] for name in plain}
                for _ in range(args.runs):
                    for name, f in plain.items():
                        ts[name].append(round(timed(f, args.reps)[0], 4))
                for name in plain:
                    print(json.dumps({"tag": args.tag, "metric": metric, "call": name, "Q": Q, "B": B, "ms": ts[name],
                                      "median_ms": float(np.median(ts[name]))}), flush=True)
                continue
            for pattern in args.patterns:
                keep = torch.from_numpy(keep_for(pattern, B, rs)).cuda()
                words = q.pack_mask(keep)

                def gather_topk():
                    pos = torch.nonzero(keep)[:, 0]
                    v, i = q.search(xq, codes[pos], k=k, norms=norms[pos], rnorms=rnorms[pos], metric=metric)
                    return v, torch.where(i >= 0, pos[i.clamp(min=0)], i)

                def gather_range():
                    pos = torch.nonzero(keep)[:, 0]
                    lims, v, i = q.range_search(xq, codes[pos], radius, norms=norms[pos], rnorms=rnorms[pos], metric=metric)
                    return lims, v, pos[i]

                calls = {"topk": (plain["topk"], lambda: q.search(xq, codes, k=k, mask=words, **kw), gather_topk),
                         "range": (plain["range"], lambda: q.range_search(xq, codes, radius, mask=words, **kw), gather_range)}
                for call, fs in calls.items():
                    names = ("unmasked", "masked", "gather")
                    for f in fs:
                        f()
                        f()
                    ts = {name: [] for name in names}
                    outs = {}
                    for _ in range(args.runs):
                        for name, f in zip(names, fs):
                            ms, outs[name] = timed(f, args.reps)
                            ts[name].append(round(ms, 4))
                    med = {name: float(np.median(v)) for name, v in ts.items()}
                    mem = {name + "_MiB": peak(f) for name, f in zip(names, fs)}
                    print(json.dumps({"metric": metric, "call": call, "pattern": pattern, "kept": int(keep.sum()), "Q": Q, "B": B,
                                      "ms": ts, "median_ms": med,
                                      "masked_over_unmasked": round(med["masked"] / med["unmasked"], 3),
                                      "gather_over_masked": round(med["gather"] / med["masked"], 2),
                                      "same_bits_as_gather": same(outs["masked"], outs["gather"]),
                                      "mask_MiB": round(words.numel() * 8 / 2 ** 20, 3), "peak_MiB": mem}), flush=True)


if __name__ == "__main__":
    main()
