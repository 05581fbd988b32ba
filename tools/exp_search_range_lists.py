"""Range search list by list (Quantizer.range_search_lists) against what a user had before it: the range search of the whole
store, and the range search under the union mask of a query's lists, one query at a time.

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), kept in the order of 1,024
lists (--store / --lists change them), L2.  The coarse centroids are the toy ones of tools/exp_search_lists.py (a random sample
of decoded vectors and a few Lloyd steps).  Radii per query, chosen against the WHOLE store as tools/exp_search_range.py does:
  about 10    : the 10th distance of Quantizer.search(k=10);
  about 1,000 : the 62nd distance of a search over every 16th stored code.
Per (Q, nprobe, target) of --queries x --nprobe x --targets, timed in ONE process, alternated, --runs runs of --reps calls each
(warmed, wall clock round a device synchronise; the host synchronisation between count and fill is inside the time):
  lists  : range_search_lists with the probes of probe_lists (formed outside the timed region)
  full   : range_search over the whole store -- what a user does today, and what lists is reported as a ratio of
  masked : for the first --masked-queries queries, range_search(mask=the union of the query's lists) one query at a time
           (the masks packed outside); reported per query
Prints one JSON line per (Q, nprobe, target): the times, the share of the store a query probes, how many vectors lists and
full list, lists over full, masked per query over lists per call, and whether lists and masked returned the same bits."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from quantization_amd import Quantizer, build_lists, probe_lists
from quantization_amd import synthetic as gen

from exp_search_lists import toy_centroids


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 64, 1024])
    ap.add_argument("--targets", type=int, nargs="*", choices=[10, 1000], default=[10, 1000])
    ap.add_argument("--masked-queries", type=int, default=4)
    ap.add_argument("--lloyd", type=int, default=5)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="", help="copied into every line (which build this process timed)")
    args = ap.parse_args()
    D, K, N, B, L = 512, 256, 8, args.store, args.lists
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
        cen = toy_centroids(q, codes, L, args.lloyd, rs)
        assign = torch.cat([torch.cdist(q.decode(codes[a:a + 65536]), cen).argmin(dim=1) for a in range(0, B, 65536)])
        order, off = build_lists(assign, L)
        codes = codes[order].contiguous()
        lens = (off[1:] - off[:-1])
        print(json.dumps({"tag": args.tag, "B": B, "lists": L, "list_len_min": int(lens.min()), "list_len_median": float(lens.float().median()),
                          "list_len_max": int(lens.max()), "empty_lists": int((lens == 0).sum())}), flush=True)
        norms = q.code_norms(codes)
        sample, sample_norms = codes[::16].contiguous(), norms[::16].contiguous()
        of = torch.repeat_interleave(torch.arange(L, device="cuda"), lens)
        for Q in args.queries:
            xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
            for target in args.targets:
                if target == 10:
                    radius = q.search(xq, codes, k=10, norms=norms)[0][:, 9].contiguous()
                else:
                    radius = q.search(xq, sample, k=62, norms=sample_norms)[0][:, 61].contiguous()
                full = lambda: q.range_search(xq, codes, radius, norms=norms)
                for nprobe in args.nprobe:
                    if nprobe > L:
                        continue
                    probes = probe_lists(xq, cen, nprobe)
                    lists = lambda: q.range_search_lists(xq, codes, off, probes, radius, norms=norms)
                    mq = min(Q, args.masked_queries)
                    named = torch.zeros(mq, L, dtype=torch.bool, device="cuda").scatter_(1, probes[:mq].long(), True)
                    words = [q.pack_mask(named[j][of]) for j in range(mq)]

                    def masked():
                        return [q.range_search(xq[j:j + 1], codes, radius[j:j + 1], norms=norms, mask=words[j]) for j in range(mq)]
                    fs = {"lists": lists, "full": full, "masked": masked}
                    for f in fs.values():                    # warm every variant
                        f()
                        f()
                    ts, outs = {name: [] for name in fs}, {}
                    for _ in range(args.runs):               # alternate
                        for name, f in fs.items():
                            ms, outs[name] = timed(f, args.reps)
                            ts[name].append(round(ms / (mq if name == "masked" else 1), 4))
                    med = {name: float(np.median(v)) for name, v in ts.items()}
                    lims, val, idx = outs["lists"]
                    same = True
                    for j, (ml, mv, mi) in enumerate(outs["masked"]):
                        lo, hi = int(lims[j]), int(lims[j + 1])
                        same &= hi - lo == int(ml[1]) and torch.equal(idx[lo:hi], mi) and torch.equal(val[lo:hi].view(torch.int32), mv.view(torch.int32))
                    per = (lims[1:] - lims[:-1]).float()
                    share = float(lens[probes.long()].sum(dim=1).float().mean()) / B
                    print(json.dumps({"tag": args.tag, "Q": Q, "nprobe": nprobe, "target": target, "B": B, "lists": L,
                                      "probed_share": round(share, 5), "ms": ts, "median_ms": med,
                                      "masked_is_per_query_of": mq,
                                      "listed": {"lists_total": int(lims[-1]), "full_total": int(outs["full"][0][-1]),
                                                 "lists_per_query_median": float(per.median())},
                                      "lists_over_full": round(med["lists"] / med["full"], 3),
                                      "masked_per_query_over_lists_call": round(med["masked"] / med["lists"], 2),
                                      "same_bits_as_masked": bool(same)}), flush=True)


if __name__ == "__main__":
    main()
