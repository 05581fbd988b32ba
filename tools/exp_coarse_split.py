"""The coarse probes for fp32 queries on the bf16 matrix cores (quantization_amd.coarse_probe_split, mcq_coarse_probe_split)
against the two paths a caller with fp32 queries had before.  Writes one JSON line per cell and contender to
profiles/coarse_split.jsonl (--out), then one line per cell of the bar.

Inputs: standard normal fp32 queries and centroids of dim 512 (the cost of no path depends on the values).  Per cell, timed in
ONE process, alternated, --runs runs of --reps calls each after two warm-up calls (wall clock round a device synchronise); each
contender's line holds every run, their median, and min .. max.  Q in --queries x L in --lists x nprobe in --nprobes, l2:
    call  : coarse_probe_split(q, centroids, nprobe, terms=terms, planes=planes, with_bias=True): allocations included
    abi   : mcq_coarse_probe_split alone through ctypes on buffers allocated once, cached terms and planes
    fp32  : coarse_probe(q, centroids, nprobe, terms=terms, with_bias=True): the only HIP path there was
    torch : probe_lists(q, centroids, nprobe) + probe_bias: the matmul path
each cell with coarse_planes_split once per centroid set (ms, median of --runs), the peak extra device memory of one `call`,
and the share of FIRST probes on which `call` and `fp32` differ (near-ties: the two scores are not the same bits).
The bar, per cell with Q >= 64 and L >= 16,384: median(fp32) - median(call) > (max - min)(call) + (max - min)(fp32)."""
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
    ap.add_argument("--nprobes", type=int, nargs="*", default=[1, 8, 64, 128])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_split.jsonl"))
    args = ap.parse_args()
    from exp_rerank import peak_extra
    from exp_search_lists import timed
    from quantization_amd import _lib, coarse_planes_split, coarse_probe, coarse_probe_split, coarse_terms, probe_bias, probe_lists
    assert torch.cuda.is_available(), "exp_coarse_split.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    lib, D = _lib.lib(), args.dim
    out = open(args.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    def contest(cell, contenders, reps):
        """alternated: run r of every contender before run r + 1 of any -> {contender: (median, max - min)}"""
        for f in contenders.values():
            f(), f()
        runs = {name: [] for name in contenders}
        for _ in range(args.runs):
            for name, f in contenders.items():
                runs[name].append(round(timed(f, reps)[0], 4))
        for name, ms in runs.items():
            emit({**cell, "contender": name, "ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms)})
        return {name: (float(np.median(ms)), max(ms) - min(ms)) for name, ms in runs.items()}

    emit({"dim": D, "runs": args.runs, "reps": args.reps})
    g = torch.Generator(device="cuda").manual_seed(11)
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        for L in args.lists:
            cen = torch.randn(L, D, device="cuda", generator=g)
            terms, planes = coarse_terms(cen), coarse_planes_split(cen)
            coarse_planes_split(cen)
            split_ms = float(np.median([timed(lambda: coarse_planes_split(cen), args.reps)[0] for _ in range(args.runs)]))
            for Q in args.queries:
                q = torch.randn(Q, D, device="cuda", generator=g)
                for P in args.nprobes:
                    parts = lib.mcq_coarse_split_parts(Q, L, D, P)
                    lists, scores, bias, ps, pl, qp = [torch.empty(shape, dtype=t, device="cuda") for shape, t in (
                        ((Q, P), torch.int32), ((Q, P), torch.float32), ((Q, P), torch.float32), ((Q, parts, P), torch.float32),
                        ((Q, parts, P), torch.int32), ((lib.mcq_kmeans_split_planes(Q, D),), torch.int16))]

                    def abi():
                        rc = lib.mcq_coarse_probe_split(q.data_ptr(), Q, cen.data_ptr(), planes.data_ptr(), L, D, terms.data_ptr(), P, 0,
                                                        parts, lists.data_ptr(), scores.data_ptr(), bias.data_ptr(), ps.data_ptr(),
                                                        pl.data_ptr(), qp.data_ptr(), st)
                        assert rc == 0

                    def call():
                        return coarse_probe_split(q, cen, P, terms=terms, planes=planes, with_bias=True)

                    def fp32():
                        return coarse_probe(q, cen, P, terms=terms, with_bias=True)

                    def torch_path():
                        probes = probe_lists(q, cen, P)
                        return probes, probe_bias(q, cen, probes)

                    cell = {"what": "probes", "Q": Q, "L": L, "nprobe": P, "parts": parts, "planes_ms": round(split_ms, 4),
                            "first_probe_differs": round(float((call()[0][:, 0] != fp32()[0][:, 0]).float().mean()), 6),
                            "peak_extra_bytes": peak_extra(call)}
                    got = contest(cell, {"call": call, "abi": abi, "fp32": fp32, "torch": torch_path}, args.reps)
                    if Q >= 64 and L >= 16384:
                        (new, new_spread), (old, old_spread) = got["call"], got["fp32"]
                        emit({"what": "bar", "Q": Q, "L": L, "nprobe": P, "margin_ms": round(old - new, 4),
                              "spreads_ms": round(new_spread + old_spread, 4), "met": old - new > new_spread + old_spread})


if __name__ == "__main__":
    main()
