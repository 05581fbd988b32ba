"""The exact re-ranking of a shortlist (quantization_amd.rerank, mcq_rerank) against the torch recipe it replaces.  Writes one
JSON line per cell to profiles/rerank.jsonl (--out).

Shape: 1,048,576 raw vectors of dim 512 (seeded normal draws), fp32 and fp16, their 8 x 256 codes of the bench state
(synthetic_state(103, ...)) kept in the order of the 1,024 toy lists of tools/exp_search_lists.py, L2.  The shortlists are the
indexes of search_wide (the whole store) and of search_lists_wide (8 probes) at k = S, positions of the store IN LIST ORDER, so
row_of = order is present throughout and the raw vectors stay in their original order.
Cells: dtype x source x S in --shortlists x Q in --queries x k in --ks.  Per cell, timed in ONE process, alternated, --runs
runs of --reps calls each after two warm-up calls (wall clock round a device synchronise); each contender's line holds every
run, their median, and min .. max:
  call        : quantization_amd.rerank(queries, vectors, short, k, row_of=order), the public call with its allocations
  abi         : mcq_rerank alone through ctypes on buffers allocated once: what a C caller gets
  recipe      : the line of the parent's ivf.py docstring,
                ((vectors[order][short.clamp(min=0)] - queries[:, None]) ** 2).sum(2).masked_fill(short < 0, inf).topk(k, largest=False)
  recipe_kept : the same with vectors[order] made once outside the timed region (a second copy of the store kept for good)
Each line also holds the peak extra device memory of one call of each contender (torch's allocator; recipe_kept's does not
count the kept copy, given as `kept_copy_bytes`), the bytes a re-rank has to gather, Q S D sizeof, the achieved gather rate
of `call` and `abi` over those bytes (the microarchitecture guide measures 5.5-5.8 TB/s for whole random rows gathered into
registers), and whether the call and the recipe list the same positions."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

from exp_search_lists import timed, toy_centroids
from quantization_amd import Quantizer, _lib, build_lists, probe_lists, rerank
from quantization_amd import synthetic as gen


def peak_extra(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = f()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--lists", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=8)
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--shortlists", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--ks", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--lloyd", type=int, default=5)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank.jsonl"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "exp_rerank.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    D, K, N, B, L = 512, 256, 8, args.store, args.lists
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for name, v in gen.synthetic_state(103, D, K, N).items():
        sd[name] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    q = q.cuda().requires_grad_(False)
    rs = np.random.RandomState(5)
    lib = _lib.lib()
    out = open(args.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(11)
        vectors32 = torch.randn((B, D), generator=g, device="cuda", dtype=torch.float32)
        codes = torch.cat([q.encode(vectors32[a:a + 65536]) for a in range(0, B, 65536)])
        cen = toy_centroids(q, codes, L, args.lloyd, rs)
        assign = torch.cat([torch.cdist(q.decode(codes[a:a + 65536]), cen).argmin(dim=1) for a in range(0, B, 65536)])
        order, off = build_lists(assign, L)
        codes = codes[order].contiguous()
        norms = q.code_norms(codes)
        emit({"B": B, "lists": L, "dim": D, "codebooks": N, "codebook_size": K, "nprobe": args.nprobe, "runs": args.runs,
              "reps": args.reps, "guide_gather_TBps": [5.5, 5.8]})
        for dtype in (torch.float32, torch.float16):
            vectors = vectors32 if dtype == torch.float32 else vectors32.to(dtype)
            kept = vectors[order]                             # recipe_kept's second copy of the store
            el = vectors.element_size()
            for Q in args.queries:
                xq32 = vectors32[torch.from_numpy(rs.choice(B, Q, replace=False)).cuda()] + 0.3 * torch.randn((Q, D), generator=g, device="cuda")
                xq = xq32.to(dtype)
                for source in ("search_wide", "search_lists_wide"):
                    for S in args.shortlists:
                        if source == "search_wide":
                            _, short = q.search_wide(xq32, codes, S, norms=norms)
                        else:
                            _, short = q.search_lists_wide(xq32, codes, off, probe_lists(xq32, cen, args.nprobe), S, norms=norms)
                        short = short.contiguous()
                        for k in args.ks:
                            ws = torch.empty((lib.mcq_rerank_workspace_bytes(Q, S, D, k),), dtype=torch.uint8, device="cuda")
                            o_s = torch.empty((Q, k), dtype=torch.float32, device="cuda")
                            o_i = torch.empty((Q, k), dtype=torch.int64, device="cuda")
                            st = torch.cuda.current_stream().cuda_stream
                            half = int(dtype == torch.float16)

                            def abi():
                                rc = lib.mcq_rerank(xq.data_ptr(), half, Q, vectors.data_ptr(), half, B, D, short.data_ptr(), S,
                                                    order.data_ptr(), B, k, 0, o_s.data_ptr(), o_i.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), st)
                                assert rc == 0, rc
                                return o_s, o_i

                            def recipe_on(store):
                                return ((store[short.clamp(min=0)] - xq[:, None]) ** 2).sum(2).masked_fill(
                                    short < 0, float("inf")).topk(k, largest=False)

                            fs = {"call": lambda: rerank(xq, vectors, short, k, row_of=order), "abi": abi,
                                  "recipe": lambda: recipe_on(vectors[order]), "recipe_kept": lambda: recipe_on(kept)}
                            for f in fs.values():
                                f()
                                f()
                            ts, outs = {name: [] for name in fs}, {}
                            for _ in range(args.runs):
                                for name, f in fs.items():
                                    ms, outs[name] = timed(f, args.reps)
                                    ts[name].append(round(ms, 4))
                            med = {name: float(np.median(v)) for name, v in ts.items()}
                            nbytes = Q * S * D * el
                            a, b = outs["call"][1], outs["recipe_kept"][1]
                            b = short.gather(1, b)                # the recipe lists slots of the shortlist: their positions
                            b = torch.where(torch.isinf(outs["recipe_kept"][0]), torch.full_like(b, -1), b)
                            emit({"dtype": str(dtype).split(".")[1], "source": source, "Q": Q, "S": S, "k": k, "ms": ts, "median_ms": med,
                                  "min_max_ms": {name: [min(v), max(v)] for name, v in ts.items()},
                                  "peak_extra_bytes": {name: peak_extra(f) for name, f in fs.items()},
                                  "kept_copy_bytes": kept.numel() * el, "gather_bytes": nbytes,
                                  "gather_TBps": {name: round(nbytes / (med[name] * 1e-3) / 1e12, 3) for name in ("call", "abi")},
                                  "recipe_over_call": round(med["recipe_kept"] / med["call"], 2),
                                  "same_bits_call_abi": bool(torch.equal(outs["call"][1], outs["abi"][1])),
                                  "rows_with_the_recipes_positions": int((a.sort(1).values == b.sort(1).values).all(1).sum())})
            del kept
    out.close()


if __name__ == "__main__":
    main()
