"""One Lloyd step in HIP (quantization_amd.kmeans_step: mcq_kmeans_assign, a torch sort, mcq_kmeans_update) against the same
step composed from what the library had before it and against plain torch.  Writes one JSON line per contender and cell to
profiles/kmeans.jsonl (--out).

Inputs: standard normal fp32 vectors and centroids of dim 512 (no path's cost depends on the values).  Per cell, timed in ONE
process, alternated, --runs runs of --reps calls each after two warm-up calls (wall clock round a device synchronise); each
contender's line holds every run, their median, and min .. max, and the peak extra device memory of one call.
  step    : kmeans_step(x, centroids, terms=terms): the public call, allocations and the sort included
  assign  : mcq_kmeans_assign alone through ctypes on buffers allocated once   } the shares of `step`; what is left is the
  update  : mcq_kmeans_update alone, on the sorted order of that assignment    } sort, the offsets and the allocations
  parent  : coarse_assign + a stable torch sort + index_add_ of the rows + a division: the step as the parent commit composes it
  torch   : matmul + argmin over chunks of --chunk vectors + index_add_ + a division
  rocblas : the matmul + argmin of `torch` alone: what `assign` stands against"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans.jsonl"))
    ap.add_argument("--tag", default=None, help="a label put into every line, such as the library the process loaded")
    ap.add_argument("--only", nargs="*", default=None, help="the contenders to time (all by default)")
    args = ap.parse_args()
    from exp_rerank import peak_extra
    from exp_search_lists import timed
    from quantization_amd import _lib, coarse_assign, coarse_terms, kmeans_step
    assert torch.cuda.is_available(), "exp_kmeans.py times the MI355X: there is no CPU path"
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
            x, cen = torch.randn(B, D, device="cuda", generator=g), torch.randn(L, D, device="cuda", generator=g)
            terms = coarse_terms(cen)
            parts = lib.mcq_kmeans_parts(B, L, D)
            assign, score = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.float32, device="cuda")
            ps, pl = torch.empty(B, parts, dtype=torch.float32, device="cuda"), torch.empty(B, parts, dtype=torch.int32, device="cuda")
            new, counts = torch.empty_like(cen), torch.empty(L, dtype=torch.int32, device="cuda")
            first = torch.empty(L + 1, dtype=torch.int64, device="cuda")
            sums = torch.empty(lib.mcq_kmeans_blocks(B, L, D), dtype=torch.float64, device="cuda")

            def abi_assign():
                assert lib.mcq_kmeans_assign(x.data_ptr(), B, cen.data_ptr(), L, D, terms.data_ptr(), parts, None, assign.data_ptr(),
                                             score.data_ptr(), None, ps.data_ptr(), pl.data_ptr(), st) == 0

            abi_assign()
            keys, order = torch.sort(assign.to(torch.int64), stable=True)
            offsets = torch.searchsorted(keys, torch.arange(L + 1, dtype=torch.int64, device="cuda"))

            def abi_update():
                assert lib.mcq_kmeans_update(x.data_ptr(), B, D, order.data_ptr(), offsets.data_ptr(), L, cen.data_ptr(), new.data_ptr(),
                                             counts.data_ptr(), first.data_ptr(), sums.data_ptr(), st) == 0

            def mean_of(a):                                  # the torch update: float atomics, another sum on every run
                n = torch.bincount(a, minlength=L).to(torch.float32)
                total = torch.zeros_like(cen).index_add_(0, a, x)
                return torch.where(n[:, None] > 0, total / n.clamp(min=1)[:, None], cen)

            def parent():
                a = coarse_assign(x, cen, terms=terms).to(torch.int64)
                torch.sort(a, stable=True)                   # (what build_lists does next; the mean itself needs no order)
                return mean_of(a)

            def rocblas():
                h = 0.5 * (cen * cen).sum(dim=1)
                return torch.cat([(x[at:at + args.chunk] @ cen.t() - h[None, :]).argmax(dim=1) for at in range(0, B, args.chunk)])

            contenders = {"step": lambda: kmeans_step(x, cen, terms=terms), "assign": abi_assign, "update": abi_update,
                          "parent": parent, "torch": lambda: mean_of(rocblas()), "rocblas": rocblas}
            mine, theirs = kmeans_step(x, cen, terms=terms), rocblas()
            cell = {"B": B, "L": L, "parts": parts, "same_assign": round(float((mine[1].long() == theirs).float().mean()), 6),
                    "max_abs_diff_to_torch_mean": float((mine[0] - mean_of(theirs)).abs().max())}
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
