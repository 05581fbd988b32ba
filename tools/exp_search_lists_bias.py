"""What a bias per probe slot costs the search list by list (Quantizer.search_lists / range_search_lists with probe_bias, the
residual flow of quantization_amd.ivf) against the same calls without one.

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), kept in the order of 1,024
lists (toy centroids as in tools/exp_search_lists.py: a sample of decoded vectors and a few Lloyd steps), 64 queries, 8 and 64
probes, k = 10, and the range search at the radius of each query's 10th best (about 10 hits per query).  The codes are those
of the vectors themselves, not of residuals: the kernels do the same work whatever the bytes mean, and the unbiased call over
the same store is then a meaningful call too.  The bias is ivf.probe_bias of the toy centroids.

Timed in ONE process, alternated, --runs runs of --reps calls each after a warm-up (wall clock round a device synchronise),
at two levels: `scan` is the library call alone (_search_scan / _search_range over tables formed once), `call` the public
method (tables, |q|^2, thresholds, the reported values).  One JSON line per (level, nprobe, call) with every run's time, the
median and the spread (min .. max), and per pair the ratio of the medians.
--only plain times the calls without a bias alone: run it once per build under comparison (MCQ_ALLOW_LIB_PATH=1
MCQ_LIB_PATH=<an older libmcq_hip.so>, which has no entry with a bias), alternating the processes."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from quantization_amd import Quantizer, build_lists, probe_lists
from quantization_amd import synthetic as gen

from exp_search_lists import timed, toy_centroids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--nprobe", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--lloyd", type=int, default=5)
    ap.add_argument("--only", choices=["plain"], default=None)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--tag", default="", help="copied into every line (which build this process timed)")
    args = ap.parse_args()
    D, K, N, B, L, Q, k = 512, 256, 8, args.store, args.lists, args.queries, 10
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for name, v in gen.synthetic_state(103, D, K, N).items():
        sd[name] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    q = q.cuda().requires_grad_(False)
    rs = np.random.RandomState(5)
    biased = args.only != "plain"
    with torch.no_grad():
        if args.random_codes:
            codes = torch.from_numpy(rs.randint(0, K, size=(B, N)).astype(np.uint8)).cuda()
        else:
            codes = torch.cat([q.encode(torch.from_numpy(gen.make_gaussian(8 + a, min(65536, B - a), D)).cuda())
                               for a in range(0, B, 65536)])
        cen = toy_centroids(q, codes, L, args.lloyd, rs)
        assign = torch.cat([torch.cdist(q.decode(codes[a:a + 65536]), cen).argmin(dim=1) for a in range(0, B, 65536)])
        order, off = build_lists(assign, L)
        codes = codes[order].contiguous()
        norms = q.code_norms(codes)
        xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
        tables = q.search_tables(xq)
        if biased:
            from quantization_amd import list_assign, probe_bias
            of = list_assign(off, B)
            fs = {"code_norms": lambda: q.code_norms(codes), "code_norms_based": lambda: q.code_norms(codes, base=cen, assign=of)}
            report(args, "norms", 0, fs, max(1, args.reps // 4))
        for nprobe in args.nprobe:
            probes = probe_lists(xq, cen, nprobe)
            lists = (off, probes)
            share = float((off[1:] - off[:-1])[probes.long()].sum(dim=1).float().mean()) / B
            bias = probe_bias(xq, cen, probes) if biased else None
            # thresholds at each query's 10th best score, per call: about 10 hits per query either way
            thr_plain = q._search_scan(tables, codes, norms, k, lists=lists)[0][:, k - 1].contiguous()
            rad_plain = q.search_lists(xq, codes, off, probes, k=k, norms=norms)[0][:, k - 1].contiguous()
            scan = {"topk": lambda: q._search_scan(tables, codes, norms, k, lists=lists),
                    "range": lambda: q._search_range(tables, codes, norms, thr_plain, lists=lists)}
            call = {"topk": lambda: q.search_lists(xq, codes, off, probes, k=k, norms=norms),
                    "range": lambda: q.range_search_lists(xq, codes, off, probes, rad_plain, norms=norms)}
            if biased:
                thr_bias = q._search_scan(tables, codes, norms, k, lists=lists, bias=bias)[0][:, k - 1].contiguous()
                rad_bias = q.search_lists(xq, codes, off, probes, k=k, norms=norms, probe_bias=bias)[0][:, k - 1].contiguous()
                scan.update({"topk_bias": lambda: q._search_scan(tables, codes, norms, k, lists=lists, bias=bias),
                             "range_bias": lambda: q._search_range(tables, codes, norms, thr_bias, lists=lists, bias=bias),
                             "probe_bias": lambda: probe_bias(xq, cen, probes)})
                call.update({"topk_bias": lambda: q.search_lists(xq, codes, off, probes, k=k, norms=norms, probe_bias=bias),
                             "range_bias": lambda: q.range_search_lists(xq, codes, off, probes, rad_bias, norms=norms, probe_bias=bias)})
            extra = {"probed_share": round(share, 4), "hits_plain": int(scan["range"]()[0][-1])}
            if biased:
                extra["hits_bias"] = int(scan["range_bias"]()[0][-1])
            report(args, "scan", nprobe, scan, args.reps, extra)
            report(args, "call", nprobe, call, args.reps)


def report(args, level, nprobe, fs, reps, extra=None):
    for f in fs.values():                                   # warm-up: every call twice
        f()
        f()
    ts = {name: [] for name in fs}
    for _ in range(args.runs):                              # alternated: one run of each call in turn
        for name, f in fs.items():
            ts[name].append(round(timed(f, reps)[0], 4))
    med = {name: float(np.median(v)) for name, v in ts.items()}
    line = {"tag": args.tag, "level": level, "nprobe": nprobe, "Q": args.queries, "B": args.store, "lists": args.lists,
            "runs": args.runs, "reps": reps, "ms": ts, "median_ms": med,
            "spread_ms": {name: [min(v), max(v)] for name, v in ts.items()}}
    for name in fs:
        if name.endswith("_bias") and name[:-5] in fs:
            line[name + "_over_" + name[:-5]] = round(med[name] / med[name[:-5]], 4)
    if "code_norms_based" in fs:
        line["based_over_plain"] = round(med["code_norms_based"] / med["code_norms"], 4)
    line.update(extra or {})
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
