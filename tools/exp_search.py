"""Search over stored codes against what a user had before it: decode + matmul + topk.

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), k = 10, Q in {64, 1, 1024}
(--store / --queries / --k change them).  Three variants, timed in ONE process, alternated, three runs each (warmed,
synchronised, wall clock round a device synchronise):
  search : Quantizer.search(queries, codes, k, norms=precomputed)      -- tables + scan + merge + |q|^2
  (a)    : Quantizer.decode of the whole store, queries @ decoded.T in column chunks, torch.topk
  (b)    : the same with the decoded matrix held resident and excluded from the time
Prints per variant the three times, the peak device memory (torch.cuda.max_memory_allocated over one call, reset before it),
whether the three agree on the positions, and for the search the gathers per second Q * B * N / time of the whole call.
--only search runs the search alone (for a profiler: rocprofv3 --kernel-trace --stats -- python tools/exp_search.py --only search),
three alternating timed runs of --reps calls per metric; with MCQ_ALLOW_LIB_PATH=1 MCQ_LIB_PATH=<another build> it is one side of
an A/B of two libraries (an older build has the L2 metric only).
--metric l2 | ip | cosine (any number of them; default l2): the score of the search and of the baselines.  ip: queries @ decoded.T
and topk(largest=True); cosine: the same on the decoded rows divided by their norms ((b) holds the NORMALISED matrix resident),
the queries' norms divided out at the end; the search gets rnorms=code_rnorms(codes) precomputed, as L2 gets norms."""
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
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=1 << 18, help="columns of the score matrix formed at a time by (a) and (b)")
    ap.add_argument("--only", choices=["search"], default=None)
    ap.add_argument("--metric", nargs="*", choices=["l2", "ip", "cosine"], default=["l2"])
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames (profiler runs)")
    ap.add_argument("--reps", type=int, default=20, help="calls of the search per timed run with --only search")
    args = ap.parse_args()
    D, K, N, B, k = 512, 256, 8, args.store, args.k
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
        t_norms, _ = timed(lambda: q.code_norms(codes), 3)
        print(json.dumps({"store": B, "code_norms_ms": round(t_norms, 3)}), flush=True)

        rnorms = None
        if "cosine" in args.metric:
            rnorms = q.code_rnorms(codes)
            t_r, _ = timed(lambda: q.code_rnorms(codes), 3)
            t_c, _ = timed(lambda: q.rnorms_from_norms(norms), 3)
            print(json.dumps({"store": B, "code_rnorms_ms": round(t_r, 3), "rnorms_from_norms_ms": round(t_c, 3)}), flush=True)

        def topk_of(xq, dec, metric, normalised=False):
            best_v = best_i = None
            near = metric != "l2"                      # similarities: the largest first
            for a in range(0, B, args.chunk):
                blk = dec[a:a + args.chunk]
                if metric == "l2":
                    s = (blk * blk).sum(1)[None, :] - 2.0 * (xq @ blk.T)
                elif metric == "ip" or normalised:
                    s = xq @ blk.T
                else:
                    s = xq @ (blk / (blk * blk).sum(1, keepdim=True).sqrt()).T
                v, i = torch.topk(s, min(k, s.shape[1]), dim=1, largest=near)
                i = i + a
                if best_v is not None:
                    v, j = torch.topk(torch.cat([best_v, v], 1), k, dim=1, largest=near)
                    i = torch.cat([best_i, i], 1).gather(1, j)
                best_v, best_i = v, i
            if metric == "l2":
                return best_v + (xq * xq).sum(1, keepdim=True), best_i
            return (best_v / (xq * xq).sum(1, keepdim=True).sqrt() if metric == "cosine" else best_v), best_i

        def searcher(xq, metric):
            if metric == "l2":
                return lambda: q.search(xq, codes, k=k, norms=norms)
            return lambda: q.search(xq, codes, k=k, metric=metric, rnorms=rnorms)

        for Q in args.queries:
            xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
            if args.only == "search":
                fs = {m: searcher(xq, m) for m in args.metric}
                for f in fs.values():
                    for _ in range(3):
                        f()
                ts = {m: [] for m in fs}
                for _ in range(3):                      # alternate
                    for m, f in fs.items():
                        ts[m].append(round(timed(f, args.reps)[0], 4))
                print(json.dumps({"Q": Q, "search_ms": ts, "gathers_per_s": {m: Q * B * N / (float(np.median(v)) * 1e-3)
                                                                              for m, v in ts.items()}}), flush=True)
                continue
            for metric in args.metric:
                compare(q, xq, codes, metric, searcher(xq, metric), topk_of, args, Q, B, N, k)


def compare(q, xq, codes, metric, f_search, topk_of, args, Q, B, N, k):
    """search against (a) and (b) under one metric at one Q: three alternating runs, peak memory, agreement of positions"""
    f_a = lambda: topk_of(xq, q.decode(codes), metric)
    resident = q.decode(codes)
    if metric == "cosine":
        resident /= (resident * resident).sum(1, keepdim=True).sqrt()
    f_b = lambda: topk_of(xq, resident, metric, normalised=True)
    mem = {"b_resident_MiB": resident.numel() * 4 / 2 ** 20}
    for f in (f_search, f_a, f_b):          # warm every variant
        f()
        f()
    ts = {"search": [], "a": [], "b": []}
    for _ in range(3):                      # alternate
        for name, f in (("search", f_search), ("a", f_a), ("b", f_b)):
            ms, out = timed(f)
            ts[name].append(round(ms, 4))
            if name == "search":
                got = out
            elif name == "a":
                ref = out
    mem.update(search_MiB=peak(f_search), b_MiB=peak(f_b))
    del resident
    torch.cuda.empty_cache()
    mem["a_MiB"] = peak(f_a)
    agree = float((got[1] == ref[1]).float().mean())
    print(json.dumps({"Q": Q, "B": B, "k": k, "metric": metric, "ms": ts, "no_overlap_vs_a": max(ts["search"]) < min(ts["a"]),
                      "a_over_search": round(min(ts["a"]) / max(ts["search"]), 2),
                      "b_over_search": round(float(np.median(ts["b"]) / np.median(ts["search"])), 3),
                      "peak_MiB": {k_: round(v, 1) for k_, v in mem.items()},
                      "positions_agree_with_a": round(agree, 5),
                      "gathers_per_s": Q * B * N / (float(np.median(ts["search"])) * 1e-3)}), flush=True)


if __name__ == "__main__":
    main()
