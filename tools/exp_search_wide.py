"""The top-k search past 64 neighbours (Quantizer.search_wide / search_lists_wide) against what it costs and what a user had
before it.  Writes one JSON line per cell to profiles/search_wide.jsonl (--out).

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), kept in the order of the 1,024
toy lists of tools/exp_search_lists.py (a random sample of decoded vectors and a few Lloyd steps), L2.
Cells: Q in --queries x k in --ks x {the whole store, 8 probes, 64 probes}.  Per cell, timed in ONE process, alternated,
--runs runs of --reps calls each after two warm-up calls (wall clock round a device synchronise); each contender's line
holds every run, their median, and min .. max:
  wide    : the wide kernels (mcq_search_wide / mcq_search_wide_lists), at k = 64 too -- there against
  narrow  : search(k=64) / search_lists(k=64) of the same build: the price of the structure
  matmul  : (whole store) decode + matmul + torch.topk(k): what a user without the call does today, 2 GB of decoded vectors
  range   : range_search / range_search_lists at the radius of each query's k-th neighbour (taken from `wide`, outside the
            timed region: the user has to guess it), then a sort per query
Each line also says whether wide and narrow returned the same bits (k = 64), and whether the sorted range result holds the
positions wide returned."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from exp_search_lists import same, timed, toy_centroids
from quantization_amd import Quantizer, build_lists, probe_lists
from quantization_amd import synthetic as gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--ks", type=int, nargs="*", default=[64, 100, 256, 1024])
    ap.add_argument("--nprobe", type=int, nargs="*", default=[0, 8, 64], help="0: the whole store")
    ap.add_argument("--lloyd", type=int, default=5)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_wide.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "exp_search_wide.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    D, K, N, B, L = 512, 256, 8, args.store, args.lists
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for name, v in gen.synthetic_state(103, D, K, N).items():
        sd[name] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    q = q.cuda().requires_grad_(False)
    rs = np.random.RandomState(5)
    out = open(args.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    with torch.no_grad():
        if args.random_codes:
            codes = torch.randint(0, K, (B, N), dtype=torch.uint8, device="cuda")
        else:
            codes = torch.cat([q.encode(torch.from_numpy(gen.make_gaussian(8 + a, min(65536, B - a), D)).cuda())
                               for a in range(0, B, 65536)])
        cen = toy_centroids(q, codes, L, args.lloyd, rs)
        assign = torch.cat([torch.cdist(q.decode(codes[a:a + 65536]), cen).argmin(dim=1) for a in range(0, B, 65536)])
        order, off = build_lists(assign, L)
        codes = codes[order].contiguous()
        norms = q.code_norms(codes)
        emit({"B": B, "lists": L, "dim": D, "codebooks": N, "codebook_size": K, "runs": args.runs, "reps": args.reps,
              "random_codes": bool(args.random_codes)})
        for Q in args.queries:
            xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
            for nprobe in args.nprobe:
                lists = None if nprobe == 0 else (off, probe_lists(xq, cen, nprobe))
                for k in args.ks:
                    wide = lambda: q._topk(xq, codes, k, norms, "l2", None, None, lists, wide=True)
                    fs = {"wide": wide}
                    if k == 64:
                        fs["narrow"] = lambda: q._topk(xq, codes, k, norms, "l2", None, None, lists)
                    got = wide()
                    radius = got[0][:, -1].contiguous()
                    if lists is None:
                        def matmul():
                            dec = q.decode(codes)
                            s = norms[None, :] - 2.0 * (xq @ dec.T)
                            v, i = torch.topk(s, k, dim=1, largest=False)
                            return v + (xq * xq).sum(dim=1, keepdim=True), i
                        fs["matmul"] = matmul

                    def ranged():
                        if lists is None:
                            lims, v, i = q.range_search(xq, codes, radius, norms=norms)
                        else:
                            lims, v, i = q.range_search_lists(xq, codes, lists[0], lists[1], radius, norms=norms)
                        rows = torch.repeat_interleave(torch.arange(Q, device="cuda"), lims[1:] - lims[:-1], output_size=v.numel())
                        by = torch.argsort(v, stable=True)
                        by = by[torch.argsort(rows[by], stable=True)]
                        return lims, v[by], i[by]
                    if bool(torch.isfinite(radius).all()):
                        fs["range"] = ranged
                    for f in fs.values():
                        f()
                        f()
                    ts, outs = {name: [] for name in fs}, {}
                    for _ in range(args.runs):
                        for name, f in fs.items():
                            ms, outs[name] = timed(f, args.reps)
                            ts[name].append(round(ms, 4))
                    line = {"Q": Q, "k": k, "nprobe": nprobe, "B": B, "ms": ts,
                            "median_ms": {name: float(np.median(v)) for name, v in ts.items()},
                            "min_max_ms": {name: [min(v), max(v)] for name, v in ts.items()}}
                    if "narrow" in fs:
                        line["same_bits_as_narrow"] = same(outs["wide"], outs["narrow"])
                        line["wide_over_narrow"] = round(line["median_ms"]["wide"] / line["median_ms"]["narrow"], 3)
                    if "range" in fs:
                        lims, _, ri = outs["range"]
                        n = lims[1:] - lims[:-1]
                        line["range_hits_min_max"] = [int(n.min()), int(n.max())]
                        line["range_holds_wide"] = bool((n >= k).all()) and all(
                            torch.equal(ri[lims[j]:lims[j] + k], outs["wide"][1][j]) for j in range(min(Q, 4)))
                    emit(line)
    out.close()


if __name__ == "__main__":
    main()
