"""Search list by list (Quantizer.search_lists) against what a user had before it: the scan of the whole store, and the scan
under the union mask of a query's lists, one query at a time.

Shape: 1,048,576 stored codes of the bench state (dim 512, 8 x 256, synthetic_state(103, ...)), k = 10, kept in the order of
1,024 lists (--store / --lists change them).  The coarse centroids are toy ones: a random sample of decoded vectors and a few
Lloyd steps in torch; the recall they give is reported, not gated.  Per (Q, nprobe) of --queries x --nprobe under L2, and at
Q = 64 under the other metrics, timed in ONE process, alternated, --runs runs of --reps calls each (warmed, wall clock round
a device synchronise):
  lists  : search_lists with the probes of probe_lists (formed outside the timed region; their own time is reported)
  full   : search over the whole store -- what a user does today
  masked : for Q <= 64, search(mask=the union of the query's lists) one query at a time (the masks packed outside)
Prints one JSON line per (metric, Q, nprobe): the times, the share of the store a query probes, lists against full, recall@k
of lists against full, and whether lists and masked returned the same bits.
--only full times the scan alone, one line per (metric, Q): run it once per build under comparison
(MCQ_ALLOW_LIB_PATH=1 MCQ_LIB_PATH=<an older libmcq_hip.so> for the other one), alternating the processes."""
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


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, out


def same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def toy_centroids(q, codes, L, steps, rs):
    """a random sample of decoded vectors and a few Lloyd steps"""
    B = codes.shape[0]
    sample = q.decode(codes[torch.from_numpy(rs.choice(B, min(B, 32 * L), replace=False)).cuda()])
    cen = sample[:L].clone()
    for _ in range(steps):
        a = torch.cdist(sample, cen).argmin(dim=1)
        tot = torch.zeros_like(cen).index_add_(0, a, sample)
        cnt = torch.bincount(a, minlength=L).to(cen.dtype)[:, None]
        cen = torch.where(cnt > 0, tot / cnt.clamp(min=1), cen)
    return cen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--nprobe", type=int, nargs="*", default=[1, 8, 32, 128, 1024])
    ap.add_argument("--metrics", nargs="*", default=["l2", "ip", "cosine"])
    ap.add_argument("--lloyd", type=int, default=5)
    ap.add_argument("--only", choices=["full"], default=None)
    ap.add_argument("--random-codes", action="store_true", help="uniform random codes instead of encoded frames")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tag", default="", help="copied into every line (which build this process timed)")
    args = ap.parse_args()
    D, K, N, B, L, k = 512, 256, 8, args.store, args.lists, 10
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
        if args.only != "full":
            cen = toy_centroids(q, codes, L, args.lloyd, rs)
            assign = torch.cat([torch.cdist(q.decode(codes[a:a + 65536]), cen).argmin(dim=1) for a in range(0, B, 65536)])
            order, off = build_lists(assign, L)
            codes = codes[order].contiguous()
            lens = (off[1:] - off[:-1]).cpu().numpy()
            print(json.dumps({"tag": args.tag, "B": B, "lists": L, "list_len_min": int(lens.min()), "list_len_median": float(np.median(lens)),
                              "list_len_max": int(lens.max()), "empty_lists": int((lens == 0).sum())}), flush=True)
        norms = q.code_norms(codes)
        rnorms = q.rnorms_from_norms(norms)
        for metric in args.metrics:
            kw = dict(norms=norms, rnorms=rnorms, metric=metric)
            for Q in args.queries:
                if metric != "l2" and Q != 64:
                    continue
                xq = torch.from_numpy(gen.make_gaussian(900 + Q, Q, D)).cuda()
                full = lambda: q.search(xq, codes, k=k, **kw)
                for _ in range(3):
                    full()
                if args.only == "full":
                    ts = [round(timed(full, args.reps)[0], 4) for _ in range(args.runs)]
                    print(json.dumps({"tag": args.tag, "metric": metric, "call": "full", "Q": Q, "B": B, "ms": ts,
                                      "median_ms": float(np.median(ts))}), flush=True)
                    continue
                for nprobe in args.nprobe:
                    if nprobe > L:
                        continue
                    probe = lambda: probe_lists(xq, cen, nprobe, metric=metric)
                    probes = probe()
                    lists = lambda: q.search_lists(xq, codes, off, probes, k=k, **kw)
                    fs = {"lists": lists, "full": full, "probe_lists": probe}
                    if Q <= 64:
                        named = torch.zeros(Q, L, dtype=torch.bool, device="cuda").scatter_(1, probes.long(), True)
                        of = torch.repeat_interleave(torch.arange(L, device="cuda"), off[1:] - off[:-1])
                        words = [q.pack_mask(named[j][of]) for j in range(Q)]

                        def masked():
                            outs = [q.search(xq[j:j + 1], codes, k=k, mask=words[j], **kw) for j in range(Q)]
                            return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs])
                        fs["masked"] = masked
                    for f in fs.values():
                        f()
                        f()
                    ts, outs = {name: [] for name in fs}, {}
                    for _ in range(args.runs):
                        for name, f in fs.items():
                            ms, outs[name] = timed(f, args.reps if name != "masked" else max(1, args.reps // 5))
                            ts[name].append(round(ms, 4))
                    med = {name: float(np.median(v)) for name, v in ts.items()}
                    share = float((off[1:] - off[:-1])[probes.long()].sum(dim=1).float().mean()) / B
                    hit = (outs["lists"][1][:, :, None] == outs["full"][1][:, None, :]).any(dim=2).float().mean()
                    line = {"tag": args.tag, "metric": metric, "Q": Q, "nprobe": nprobe, "B": B, "lists": L, "probed_share": round(share, 4),
                            "ms": ts, "median_ms": med, "lists_over_full": round(med["lists"] / med["full"], 3),
                            f"recall@{k}": round(float(hit), 4)}
                    if "masked" in fs:
                        line["masked_over_lists"] = round(med["masked"] / med["lists"], 2)
                        line["same_bits_as_masked"] = same(outs["lists"], outs["masked"])
                    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
