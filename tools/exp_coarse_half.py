"""The coarse probes for fp16 queries in HIP (quantization_amd.coarse_probe_half, mcq_coarse_probe_half) against the three paths
a caller with fp16 queries had before.  Writes one JSON line per cell to profiles/coarse_half.jsonl (--out).

Inputs: standard normal fp16 queries and fp32 centroids of dim 512 (the cost of no path depends on the values).  Per cell, timed
in ONE process, alternated, --runs runs of --reps calls each after two warm-up calls (wall clock round a device synchronise);
each contender's line holds every run, their median, and min .. max.  Q in --queries x L in --lists x nprobe in --nprobes, l2:
    call   : coarse_probe_half(q16, centroids, nprobe, terms=terms, planes=planes, with_bias=True): allocations included
    abi    : mcq_coarse_probe_half alone through ctypes on buffers allocated once, cached terms and planes
    fp32   : coarse_probe(q16.float(), centroids, nprobe, terms=terms, with_bias=True): the only HIP path there was
    torch  : probe_lists(q16.float(), centroids, nprobe) + probe_bias: the matmul path
    torch16: (q16 @ c16.t()) and topk in fp16 on a cached fp16 copy of the centroids: plain torch (ip order, no bias)
each cell with coarse_planes once per centroid set (ms, median of --runs), the peak extra device memory of one `call`, and the
share of probe entries on which `call` and `fp32` agree.
Then the scan: at the largest Q x the largest L, `abi` alone at every nprobe of --scan (both sides of the list classes) with
half, once and twice the recommended `parts`: what the selection costs on top of the product, and whether the plan holds."""
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
    ap.add_argument("--scan", type=int, nargs="*", default=[1, 8, 16, 17, 32, 64, 65, 96, 128])
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coarse_half.jsonl"))
    args = ap.parse_args()
    from exp_rerank import peak_extra
    from exp_search_lists import timed
    from quantization_amd import _lib, coarse_planes, coarse_probe, coarse_probe_half, coarse_terms, probe_bias, probe_lists
    assert torch.cuda.is_available(), "exp_coarse_half.py times the MI355X: there is no CPU path"
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

    def buffers(Q, P, parts):
        return [torch.empty(shape, dtype=t, device="cuda") for shape, t in (((Q, P), torch.int32), ((Q, P), torch.float32),
                ((Q, P), torch.float32), ((Q, parts, P), torch.float32), ((Q, parts, P), torch.int32))]

    with torch.no_grad():
        for L in args.lists:
            cen = torch.randn(L, D, device="cuda", generator=g)
            terms, planes, c16 = coarse_terms(cen), coarse_planes(cen), cen.half()
            coarse_planes(cen)
            split_ms = float(np.median([timed(lambda: coarse_planes(cen), args.reps)[0] for _ in range(args.runs)]))
            for Q in args.queries:
                q16 = torch.randn(Q, D, device="cuda", generator=g).half()
                q32 = q16.float()
                for P in args.nprobes:
                    parts = lib.mcq_coarse_half_parts(Q, L, D, P)
                    lists, scores, bias, ps, pl = buffers(Q, P, parts)

                    def abi():
                        rc = lib.mcq_coarse_probe_half(q16.data_ptr(), Q, cen.data_ptr(), planes.data_ptr(), L, D, terms.data_ptr(), P, 0,
                                                       parts, lists.data_ptr(), scores.data_ptr(), bias.data_ptr(), ps.data_ptr(),
                                                       pl.data_ptr(), st)
                        assert rc == 0

                    def call():
                        return coarse_probe_half(q16, cen, P, terms=terms, planes=planes, with_bias=True)

                    def fp32():
                        return coarse_probe(q32, cen, P, terms=terms, with_bias=True)

                    def torch_path():
                        probes = probe_lists(q32, cen, P)
                        return probes, probe_bias(q32, cen, probes)

                    def torch16():
                        return (q16 @ c16.t()).topk(P, dim=1)

                    cell = {"what": "probes", "Q": Q, "L": L, "nprobe": P, "parts": parts, "planes_ms": round(split_ms, 4),
                            "same_probes": round(float((call()[0] == fp32()[0]).float().mean()), 6),
                            "peak_extra_bytes": peak_extra(call)}
                    contest(cell, {"call": call, "abi": abi, "fp32": fp32, "torch": torch_path, "torch16": torch16}, args.reps)

        if args.scan:
            Q, L = max(args.queries), max(args.lists)
            cen = torch.randn(L, D, device="cuda", generator=g)
            terms, planes = coarse_terms(cen), coarse_planes(cen)
            q16 = torch.randn(Q, D, device="cuda", generator=g).half()
            for P in args.scan:
                rec = lib.mcq_coarse_half_parts(Q, L, D, P)
                for parts in sorted({max(1, rec // 2), rec, min(2 * rec, -(-L // 64))}):
                    lists, scores, bias, ps, pl = buffers(Q, P, parts)

                    def abi():
                        rc = lib.mcq_coarse_probe_half(q16.data_ptr(), Q, cen.data_ptr(), planes.data_ptr(), L, D, terms.data_ptr(), P, 0,
                                                       parts, lists.data_ptr(), scores.data_ptr(), bias.data_ptr(), ps.data_ptr(),
                                                       pl.data_ptr(), st)
                        assert rc == 0

                    contest({"what": "scan", "Q": Q, "L": L, "nprobe": P, "parts": parts, "recommended": rec}, {"abi": abi}, args.reps)


if __name__ == "__main__":
    main()
