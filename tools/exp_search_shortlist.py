"""The search over a shortlist (Quantizer.search_shortlist, mcq_search_shortlist) against what a user could write before it
existed.  Writes one JSON line per cell to profiles/search_shortlist.jsonl (--out).

Shape: 1,048,576 stored codes of dim 512 at 8 x 256 and at 64 x 256 (uniform random digits: the scorer's cost does not depend
on what the digits say), the quantizer in the bench state (synthetic_state(103, ...)), L2.  Queries are decodes of stored codes
plus noise; the shortlists are the indexes of search_wide over the whole store at k = S.
Cells: shape x Q in --queries x S in --shortlists x k in --ks.  Per cell, timed in ONE process, alternated, --runs runs of
--reps calls each after two warm-up calls (wall clock round a device synchronise); each contender's line holds every run, their
median, and min .. max:
  call        : quantizer.search_shortlist(queries, codes, short, k, norms=norms): the public call, tables and allocations included
  abi         : mcq_search_shortlist alone through ctypes on buffers allocated once and tables made once: what a C caller gets
  abi_row_of  : the same through row_of, a random permutation of the store (the three-deep chain entry -> row_of -> digits)
  instep      : abi and abi_row_of from a second build of the library whose kernel resolves the next step's entries in the step
  instep_row_of itself (-DMCQ_SHORT_AHEAD=0; --build-variant compiles it beside the product's library, which never loads it);
                absent when that library is not there
  torch       : the torch line: decode(codes[short.clamp(min=0)]) as (Q, S, D) fp32, a batched matmul, |x|^2 - 2 <q, x>,
                masked_fill for the padding, topk -- with the peak extra device memory of one call
  masked      : one search_wide(mask=...) per query, the masks packed outside the timed region (Q <= --masked-max only: it is
                one scan of the whole store per query)
  whole       : search_wide over the whole store at the same k, for orientation"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch

VARIANT = os.path.join(ROOT, "quantization_amd", "lib", "libmcq_short_instep.so")


def build_variant():
    import __graft_entry__ as g
    os.makedirs(g.LIBDIR, exist_ok=True)
    subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + g.HIPCC_FLAGS +
                          ["-DMCQ_SHORT_AHEAD=0", os.path.join(g.CSRC, "mcq_api.hip"), "-o", VARIANT], cwd=g.CSRC)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", type=int, default=1 << 20)
    ap.add_argument("--shapes", type=int, nargs="*", default=[8, 64], help="codebooks (of 256 entries)")
    ap.add_argument("--queries", type=int, nargs="*", default=[1, 64, 1024])
    ap.add_argument("--shortlists", type=int, nargs="*", default=[100, 1000])
    ap.add_argument("--ks", type=int, nargs="*", default=[10, 100])
    ap.add_argument("--masked-max", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--build-variant", action="store_true", help="compile the in-step variant of the library and exit (no GPU)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_shortlist.jsonl"))
    args = ap.parse_args()
    if args.build_variant:
        build_variant()
        return
    from exp_rerank import peak_extra
    from exp_search_lists import timed
    from quantization_amd import Quantizer, _lib
    from quantization_amd import synthetic as gen
    assert torch.cuda.is_available(), "exp_search_shortlist.py times the MI355X: there is no CPU path"
    assert args.runs >= 7, "medians of at least 7 runs"
    D, K, B = 512, 256, args.store
    lib = _lib.lib()
    alt = None
    if os.path.exists(VARIANT):
        alt = ctypes.CDLL(VARIANT)
        alt.mcq_search_shortlist.restype = _lib.SHORTLIST_SIGNATURES["mcq_search_shortlist"][0]
        alt.mcq_search_shortlist.argtypes = list(_lib.SHORTLIST_SIGNATURES["mcq_search_shortlist"][1])
    rs = np.random.RandomState(5)
    out = open(args.out, "w")

    def emit(line):
        out.write(json.dumps(line) + "\n")
        out.flush()
        print(json.dumps(line), flush=True)

    emit({"B": B, "dim": D, "codebook_size": K, "runs": args.runs, "reps": args.reps, "variant": alt is not None})
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(11)
        for N in args.shapes:
            q = Quantizer(D, K, N)
            sd = q.state_dict()
            for name, v in gen.synthetic_state(103, D, K, N).items():
                sd[name] = torch.from_numpy(np.asarray(v))
            q.load_state_dict(sd)
            q = q.cuda().requires_grad_(False)
            codes = torch.randint(0, K, (B, N), generator=g, device="cuda", dtype=torch.uint8)
            norms = q.code_norms(codes)
            order = torch.randperm(B, generator=g, device="cuda")                  # position p of the shortlist is row order[p]
            inverse = torch.empty_like(order)
            inverse[order] = torch.arange(B, device="cuda")
            for Q in args.queries:
                rows = torch.from_numpy(rs.choice(B, Q, replace=False)).cuda()
                xq = q.decode(codes[rows]) + 0.3 * torch.randn((Q, D), generator=g, device="cuda")
                tables = q.search_tables(xq)
                qq = (xq * xq).sum(1, keepdim=True)
                for S in args.shortlists:
                    _, short = q.search_wide(xq, codes, S, norms=norms)
                    short = short.contiguous()
                    moved = torch.where(short >= 0, inverse[short.clamp(min=0)], short).contiguous()
                    words = None
                    if Q <= args.masked_max:
                        keep = torch.zeros((Q, B), dtype=torch.bool, device="cuda")
                        keep.scatter_(1, short.clamp(min=0), True)
                        words = [q.pack_mask(keep[j]) for j in range(Q)]
                        del keep
                    for k in args.ks:
                        ws = torch.empty((lib.mcq_search_shortlist_workspace_bytes(Q, S, N, K, k),), dtype=torch.uint8, device="cuda")
                        o_s = torch.empty((Q, k), dtype=torch.float32, device="cuda")
                        o_i = torch.empty((Q, k), dtype=torch.int64, device="cuda")
                        st = torch.cuda.current_stream().cuda_stream

                        def abi(L=lib, sh=short, ro=None):
                            rc = L.mcq_search_shortlist(tables.data_ptr(), Q, codes.data_ptr(), norms.data_ptr(), B, N, K, k, 0,
                                                        sh.data_ptr(), S, None if ro is None else ro.data_ptr(), B, None,
                                                        o_s.data_ptr(), o_i.data_ptr(), ws.data_ptr(), ws.numel(), st)
                            assert rc == 0, rc
                            return o_s, o_i

                        def torch_line():
                            rec = q.decode(codes[short.clamp(min=0)].reshape(-1, N)).reshape(Q, S, D)
                            d = (rec * rec).sum(2) - 2.0 * torch.bmm(rec, xq[:, :, None])[:, :, 0] + qq
                            return d.masked_fill(short < 0, float("inf")).topk(k, largest=False)

                        def masked():
                            return [q.search_wide(xq[j:j + 1], codes, k, norms=norms, mask=words[j]) for j in range(Q)]

                        fs = {"call": lambda: q.search_shortlist(xq, codes, short, k, norms=norms), "abi": abi,
                              "abi_row_of": lambda: abi(lib, moved, order), "torch": torch_line,
                              "whole": lambda: q.search_wide(xq, codes, k, norms=norms)}
                        if alt is not None:
                            fs["instep"] = lambda: abi(alt)
                            fs["instep_row_of"] = lambda: abi(alt, moved, order)
                        if words is not None:
                            fs["masked"] = masked
                        reps = {name: (2 if name == "masked" else args.reps) for name in fs}
                        for f in fs.values():
                            f()
                            f()
                        ts, outs = {name: [] for name in fs}, {}
                        for _ in range(args.runs):
                            for name, f in fs.items():
                                ms, res = timed(f, reps[name])
                                outs[name] = res if name == "masked" else tuple(t.clone() for t in res)
                                ts[name].append(round(ms, 4))
                        med = {name: float(np.median(v)) for name, v in ts.items()}
                        a = outs["call"][1]
                        b = short.gather(1, outs["torch"][1])         # the torch line lists slots of the shortlist: their positions
                        b = torch.where(torch.isinf(outs["torch"][0]), torch.full_like(b, -1), b)
                        line = {"codebooks": N, "Q": Q, "S": S, "k": k, "ms": ts, "median_ms": med,
                                "min_max_ms": {name: [min(v), max(v)] for name, v in ts.items()},
                                "peak_extra_bytes": {name: peak_extra(fs[name]) for name in ("call", "torch")},
                                "torch_over_call": round(med["torch"] / med["call"], 2),
                                "same_bits_call_abi": bool(torch.equal(outs["call"][1], outs["abi"][1])),
                                "same_positions_through_row_of": bool(torch.equal(
                                    torch.where(outs["abi_row_of"][1] >= 0, order[outs["abi_row_of"][1].clamp(min=0)],
                                                outs["abi_row_of"][1]), outs["abi"][1])),
                                "rows_with_the_torch_lines_positions": int((a.sort(1).values == b.sort(1).values).all(1).sum())}
                        if alt is not None:
                            line["same_bits_instep"] = bool(torch.equal(outs["instep"][1], outs["abi"][1]) and
                                                            torch.equal(outs["instep"][0].view(torch.int32), outs["abi"][0].view(torch.int32)))
                        if words is not None:
                            line["masked_over_call"] = round(med["masked"] / med["call"], 2)
                            line["same_bits_masked"] = bool(torch.equal(torch.cat([m[1] for m in outs["masked"]]), a))
                        emit(line)
            del codes, norms, order, inverse
    out.close()


if __name__ == "__main__":
    main()
