"""The coarse probes in HIP (quantization_amd.coarse_probe / coarse_assign, mcq_coarse_probe) against the torch lines they stand
beside.  Writes one JSON line per cell to profiles/coarse.jsonl (--out).

Inputs: standard normal fp32 queries, vectors and centroids of dim 512 (the cost of neither path depends on the values).
Per cell, timed in ONE process, alternated, --runs runs of --reps calls each after two warm-up calls (wall clock round a device
synchronise); each contender's line holds every run, their median, and min .. max.
  probes   Q in --queries x L in --lists x nprobe in --nprobes:
    call   : coarse_probe(queries, centroids, nprobe, terms=terms, with_bias=True): the public call, allocations included
    abi    : mcq_coarse_probe alone through ctypes on buffers allocated once and cached terms: what a C caller gets
    torch  : probe_lists(queries, centroids, nprobe) + probe_bias(queries, centroids, probes): the parent's path
  assign   --store vectors x L in --assign-lists:
    call   : coarse_assign(vectors, centroids, terms=terms)
    torch  : matmul + argmin over chunks of --chunk vectors (the (chunk, L) score matrix is what a caller has to bound by hand)
    each with the peak extra device memory of one call, and the share of vectors on which the two agree"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--lists", type=int, nargs="*", default=[1024, 16384, 65536])
    ap.add_argument("--nprobes", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--assign-lists", type=int, nargs="*", default=[1024, 16384])
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse.jsonl"))
    args = ap.parse_args()
    from exp_rerank import peak_extra
    from exp_search_lists import timed
    from quantization_amd import _lib, coarse_assign, coarse_probe, coarse_terms, probe_bias, probe_lists
    assert torch.cuda.is_available(), "exp_coarse.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    lib, D = _lib.lib(), args.dim
    out = open(args.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    def contest(cell, contenders, reps):
        """alternated: run r of every contender before run r + 1 of any"""
        for f in contenders.values():
            f(), f()
        runs = {name: [] for name in contenders}
        for _ in range(args.runs):
            for name, f in contenders.items():
                runs[name].append(round(timed(f, reps)[0], 4))
        for name, ms in runs.items():
            emit({**cell, "contender": name, "ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)})

    emit({"dim": D, "runs": args.runs, "reps": args.reps})
    g = torch.Generator(device="cuda").manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        for L in args.lists:
            cen = torch.randn(L, D, device="cuda", generator=g)
            terms = coarse_terms(cen)
            for Q in args.queries:
                q = torch.randn(Q, D, device="cuda", generator=g)
                for P in args.nprobes:
                    parts = lib.mcq_coarse_parts(Q, L, D, P)
                    lists, scores, bias = (torch.empty(Q, P, dtype=t, device="cuda") for t in (torch.int32, torch.float32, torch.float32))
                    ps = torch.empty(Q, parts, P, dtype=torch.float32, device="cuda")
                    pl = torch.empty(Q, parts, P, dtype=torch.int32, device="cuda")

                    def abi():
                        rc = lib.mcq_coarse_probe(q.data_ptr(), Q, cen.data_ptr(), L, D, terms.data_ptr(), P, 0, parts, lists.data_ptr(),
                                                  scores.data_ptr(), bias.data_ptr(), ps.data_ptr(), pl.data_ptr(), st)
                        assert rc == 0

                    def torch_path():
                        probes = probe_lists(q, cen, P)
                        return probes, probe_bias(q, cen, probes)

                    mine, theirs = coarse_probe(q, cen, P, terms=terms, with_bias=True), torch_path()
                    cell = {"what": "probes", "Q": Q, "L": L, "nprobe": P, "parts": parts,
                            "same_probes": round(float((mine[0] == theirs[0]).float().mean()), 6)}
                    contest(cell, {"call": lambda: coarse_probe(q, cen, P, terms=terms, with_bias=True), "abi": abi,
                                   "torch": torch_path}, args.reps)
        x = torch.randn(args.store, D, device="cuda", generator=g)
        for L in args.assign_lists:
            cen = torch.randn(L, D, device="cuda", generator=g)
            terms = coarse_terms(cen)

            def torch_assign():
                h = 0.5 * (cen * cen).sum(dim=1)
                return torch.cat([(x[at:at + args.chunk] @ cen.t() - h[None, :]).argmax(dim=1) for at in range(0, x.shape[0], args.chunk)])

            mine, theirs = coarse_assign(x, cen, terms=terms), torch_assign()
            cell = {"what": "assign", "B": args.store, "L": L, "chunk": args.chunk,
                    "same_assign": round(float((mine.long() == theirs).float().mean()), 6),
                    "peak_extra_bytes": {"call": peak_extra(lambda: coarse_assign(x, cen, terms=terms)), "torch": peak_extra(torch_assign)}}
            contest(cell, {"call": lambda: coarse_assign(x, cen, terms=terms), "torch": torch_assign}, max(1, args.reps // 5))


if __name__ == "__main__":
    main()
