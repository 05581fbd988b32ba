"""Range search over stored codes against what a user had before it (decode + matmul + compare + nonzero) and against the
top-k search of the same build.

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), L2, Q in {64, 1, 1024}
(--store / --queries change them), radii chosen per query so that about 10 and about 1,000 stored vectors are listed:
  about 10    : the 10th distance of Quantizer.search(k=10);
  about 1,000 : the 62nd distance of a search over every 16th stored code (rank 62 of a 1/16 sample ~ rank 1,000 of the store;
                the top-k search stops at k = 64).
Variants, timed in ONE process, alternated, three runs each (warmed, wall clock round a device synchronise; the host
synchronisation between the count and the fill sweep is inside the time):
  range : Quantizer.range_search(queries, codes, radius, norms=precomputed)
  (a)   : Quantizer.decode of the whole store, |x|^2 - 2 q.x + |q|^2 in column chunks, compare, torch.nonzero
  topk  : Quantizer.search(queries, codes, k=10, norms=precomputed) of the same build
Prints per (Q, target) the times, the peak extra device memory of one call (torch.cuda.max_memory_allocated, reset before it),
the number of listed vectors, and how the listed SET differs from (a)'s: the pairs only one of them lists, and the largest
|distance - radius| / radius among them as (a) formed the distance (a pair within fp32 rounding of the radius may fall either way).
--only range runs range_search and search(k=10) alone, --reps calls per timed run, for a profiler:
rocprofv3 --kernel-trace --stats -- python tools/exp_search_range.py --only range --queries 64."""
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


def timed(fn, runs=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / runs * 1e3, out


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--queries", type=int, nargs="*", default=[64, 1, 1024])
    ap.add_argument("--targets", type=int, nargs="*", choices=[10, 1000], default=[10, 1000])
    ap.add_argument("--chunk", type=int, default=1 << 18, help="columns of the distance matrix formed at a time by (a)")
    ap.add_argument("--only", choices=["range"], default=None)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--reps", type=int, default=20, help="calls per timed run with --only range")
    args = ap.parse_args()
    D, K, N, B = 512, 256, 8, args.store
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for name, v in gen.synthetic_state(103, D, K, N).items():
        sd[name] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    q = q.cuda().requires_grad_(False)
    with torch.no_grad():
        if args.random_codes:
            codes = torch.randint(0, K, (B, N), dtype=torch.uint8, device="cuda")
        else:
            codes = torch.cat([q.encode(torch.from_numpy(gen.make_gaussian(8 + a, min(65536, B - a), D)).cuda())
                               for a in range(0, B, 65536)])
        norms = q.code_norms(codes)
        sample = codes[::16].contiguous()
        sample_norms = norms[::16].contiguous()

        def baseline(xq, radius):
            """(a): (query index, position) of every decoded vector within the radius, and its distance"""
            dec = q.decode(codes)
            qq = (xq * xq).sum(1, keepdim=True)
            qs, bs, ds = [], [], []
            for a in range(0, B, args.chunk):
                blk = dec[a:a + args.chunk]
                d = (blk * blk).sum(1)[None, :] - 2.0 * (xq @ blk.T) + qq
                hit = torch.nonzero(d <= radius[:, None])
                qs.append(hit[:, 0])
                bs.append(hit[:, 1] + a)
                ds.append(d[hit[:, 0], hit[:, 1]])
            return torch.cat(qs), torch.cat(bs), torch.cat(ds)

        for Q in args.queries:
            xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
            f_topk = lambda: q.search(xq, codes, k=10, norms=norms)
            for target in args.targets:
                if target == 10:
                    radius = q.search(xq, codes, k=10, norms=norms)[0][:, 9].contiguous()
                else:
                    radius = q.search(xq, sample, k=62, norms=sample_norms)[0][:, 61].contiguous()
                f_range = lambda: q.range_search(xq, codes, radius, norms=norms)
                if args.only == "range":
                    for f in (f_range, f_topk):
                        for _ in range(3):
                            f()
                    ts = {"range": [], "topk": []}
                    for _ in range(3):                  # alternate
                        for name, f in (("range", f_range), ("topk", f_topk)):
                            ts[name].append(round(timed(f, args.reps)[0], 4))
                    print(json.dumps({"Q": Q, "B": B, "target": target, "listed": int(f_range()[0][-1]), "ms": ts}), flush=True)
                    continue
                f_a = lambda: baseline(xq, radius)
                for f in (f_range, f_a, f_topk):        # warm every variant
                    f()
                    f()
                ts = {"range": [], "a": [], "topk": []}
                for _ in range(3):                      # alternate
                    for name, f in (("range", f_range), ("a", f_a), ("topk", f_topk)):
                        ms, out = timed(f)
                        ts[name].append(round(ms, 4))
                        if name == "range":
                            got = out
                        elif name == "a":
                            ref = out
                mem = {"range_MiB": peak(f_range), "topk_MiB": peak(f_topk)}
                torch.cuda.empty_cache()
                mem["a_MiB"] = peak(f_a)
                lims, _, idx = got
                rows = torch.repeat_interleave(torch.arange(Q, device="cuda"), lims[1:] - lims[:-1], output_size=idx.numel())
                mine, theirs = rows * B + idx, ref[0] * B + ref[1]
                only_mine = mine[~torch.isin(mine, theirs)]
                only_theirs = ~torch.isin(theirs, mine)
                rad_t = radius[ref[0][only_theirs]]
                margin = float(((ref[2][only_theirs] - rad_t).abs() / rad_t).max()) if bool(only_theirs.any()) else 0.0
                per = (lims[1:] - lims[:-1]).float()
                print(json.dumps({"Q": Q, "B": B, "target": target, "ms": ts,
                                  "listed": {"total": int(lims[-1]), "per_query_min": int(per.min()),
                                             "per_query_median": float(per.median()), "per_query_max": int(per.max())},
                                  "listed_by_a": int(theirs.numel()), "only_range": int(only_mine.numel()),
                                  "only_a": int(only_theirs.sum()), "only_a_largest_rel_margin": margin,
                                  "no_overlap_vs_a": max(ts["range"]) < min(ts["a"]),
                                  "a_over_range": round(min(ts["a"]) / max(ts["range"]), 2),
                                  "range_over_topk": round(float(np.median(ts["range"]) / np.median(ts["topk"])), 3),
                                  "peak_MiB": {k_: round(v, 1) for k_, v in mem.items()}}), flush=True)


if __name__ == "__main__":
    main()
