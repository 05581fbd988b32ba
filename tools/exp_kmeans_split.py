"""One Lloyd step for fp32 rows on the bf16 matrix cores (quantization_amd.kmeans_step_split: mcq_kmeans_assign_split, a torch
sort, mcq_kmeans_update) against the shipped fp32 path (kmeans_step: mcq_kmeans_assign on the fp32 matrix cores) and against
plain torch in fp32.  Writes one JSON line per contender and cell to profiles/kmeans_split.jsonl (--out).

Inputs: standard normal fp32 vectors and centroids of dim 512 (no path's cost depends on the values).  Per cell, timed in ONE
process, alternated, --runs runs of --reps calls each after two warm-up calls (wall clock round a device synchronise); each
contender's line holds every run, their median, and min .. max, and the peak extra device memory of one call.
  step         : kmeans_step_split(x, centroids, terms=terms): the public call, allocations and the sort included
  assign       : mcq_kmeans_assign_split alone through ctypes on buffers allocated once (the split of the centroids included)
  float_step   : kmeans_step(x, centroids, terms=terms) as shipped
  float_assign : mcq_kmeans_assign alone, as shipped: the bar of `assign`
  torch        : x @ centroids.t() in fp32, argmax over chunks of --chunk vectors, index_add_ of the chunks, a division
  rocblas      : the matmul + argmax of `torch` alone: what `assign` stands against in plain torch
Each cell's lines also hold the share of rows that kmeans_step_split and kmeans_step put into different lists (near-ties)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

CELLS = ((65536, 256), (262144, 1024), (1048576, 1024), (1048576, 16384))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=512)
    ap.add_argument("--cells", type=int, nargs="*", default=[v for cell in CELLS for v in cell], help="B L B L ...")
    ap.add_argument("--chunk", type=int, default=16384)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_split.jsonl"))
    ap.add_argument("--tag", default=None, help="a label put into every line, such as the library the process loaded")
    ap.add_argument("--only", nargs="*", default=None, help="the contenders to time (all by default)")
    args = ap.parse_args()
    from exp_rerank import peak_extra
    from exp_search_lists import timed
    from quantization_amd import _lib, coarse_terms, kmeans_step, kmeans_step_split
    assert torch.cuda.is_available(), "exp_kmeans_split.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    lib, D = _lib.lib(), args.dim
    out = open(args.out, "w")

    def emit(line):
        if args.tag is not None:
            line = {"tag": args.tag, **line}
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    emit({"dim": D, "runs": args.runs, "reps": args.reps, "chunk": args.chunk})
    g = torch.Generator(device="cuda").manual_seed(13)
    st = torch.cuda.current_stream().cuda_stream
    with torch.no_grad():
        for B, L in zip(args.cells[::2], args.cells[1::2]):
            x = torch.randn(B, D, device="cuda", generator=g)
            cen = torch.randn(L, D, device="cuda", generator=g)
            terms = coarse_terms(cen)
            parts, fparts = lib.mcq_kmeans_split_parts(B, L, D), lib.mcq_kmeans_parts(B, L, D)
            assign, score = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.float32, device="cuda")
            width = max(parts, fparts)
            ps, pl = torch.empty(B, width, dtype=torch.float32, device="cuda"), torch.empty(B, width, dtype=torch.int32, device="cuda")
            planes = torch.empty(lib.mcq_kmeans_split_planes(L, D), dtype=torch.int16, device="cuda")

            def abi_assign():
                assert lib.mcq_kmeans_assign_split(x.data_ptr(), B, cen.data_ptr(), L, D, terms.data_ptr(), parts, None, assign.data_ptr(),
                                                   score.data_ptr(), None, ps.data_ptr(), pl.data_ptr(), planes.data_ptr(), st) == 0

            def float_assign():
                assert lib.mcq_kmeans_assign(x.data_ptr(), B, cen.data_ptr(), L, D, terms.data_ptr(), fparts, None, assign.data_ptr(),
                                             score.data_ptr(), None, ps.data_ptr(), pl.data_ptr(), st) == 0

            def rocblas():
                h = 0.5 * (cen * cen).sum(dim=1)
                return torch.cat([(x[at:at + args.chunk] @ cen.t() - h[None, :]).argmax(dim=1) for at in range(0, B, args.chunk)])

            def plain_torch():                               # the torch update: float atomics, another sum on every run
                a = rocblas()
                n = torch.bincount(a, minlength=L).to(torch.float32)
                total = torch.zeros_like(cen)
                for at in range(0, B, args.chunk):
                    total.index_add_(0, a[at:at + args.chunk], x[at:at + args.chunk])
                return torch.where(n[:, None] > 0, total / n.clamp(min=1)[:, None], cen)

            contenders = {"step": lambda: kmeans_step_split(x, cen, terms=terms), "assign": abi_assign,
                          "float_step": lambda: kmeans_step(x, cen, terms=terms), "float_assign": float_assign,
                          "torch": plain_torch, "rocblas": rocblas}
            mine, theirs, wide = kmeans_step_split(x, cen, terms=terms), rocblas(), kmeans_step(x, cen, terms=terms)
            cell = {"B": B, "L": L, "parts": parts, "float_parts": fparts,
                    "rows_in_another_list_than_float_step": int((mine[1] != wide[1]).sum()),
                    "rows_in_another_list_than_torch": int((mine[1].long() != theirs).sum()),
                    "float_step_rows_in_another_list_than_torch": int((wide[1].long() != theirs).sum()),
                    "max_abs_diff_to_float_step_mean": float((mine[0] - wide[0]).abs().max())}
            del mine, theirs, wide
            if args.only is not None:
                contenders = {name: contenders[name] for name in args.only}
            for f in contenders.values():
                f(), f()
            runs = {name: [] for name in contenders}
            for _ in range(args.runs):                       # alternated: run r of every contender before run r + 1 of any
                for name, f in contenders.items():
                    runs[name].append(round(timed(f, args.reps)[0], 4))
            for name, ms in runs.items():
                emit({**cell, "contender": name, "ms": ms, "median_ms": float(np.median(ms)), "min_ms": min(ms), "max_ms": max(ms),
                      "peak_extra_bytes": peak_extra(contenders[name])})


if __name__ == "__main__":
    main()
