"""Fixed-point skipping (the default encode path) against MCQ_ENCODE_ALL_PASSES, on a trained state and on the bench state.

  * trained_d512_b8_p2 (a state the reference trained; tests/golden): 65,536 frames from the fixture's own generator
    (make_kind(x_kind, ...)), pinned scale factors;
  * the bench workload: synthetic_state(103), N(0,1) frames, 65,536 rows;
  * per pass, the fraction of vectors that start it (the oracle's rule: a vector has converged from the first pass whose
    result equals its input), from the GPU path itself -- encode(x, p) for p = 0 .. 5;
  * the small-batch crossover of the compaction path (MCQ_SKIP_MIN_BATCH=0 against the all-passes path);
  * the trainer's fused search (mcq_logits_refine_codes, all passes) at its 4,096-vector batch, against the same search with
    skipping (mcq_encode_ex, int64 output): what the trainer step would gain.

Prints one JSON object; run from the repository root on the GPU box."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from golden import fixtures, gen  # noqa: E402
from quantization_amd import Quantizer, _lib  # noqa: E402


def load_quantizer(state, D, K, N):
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for k, v in state.items():
        sd[k] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    if getattr(state, "scales_exp", None) is not None:
        q.pin_scale_factors(*state.scales_exp)
    return q.cuda()


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def active_fractions(q, x, iters=5):
    codes = [q.encode(x, p, as_bytes=False) for p in range(iters + 1)]
    B = x.shape[0]
    done = torch.zeros(B, dtype=torch.bool, device=x.device)
    out = []
    for p in range(1, iters + 1):
        out.append(round(1.0 - float(done.float().mean()), 4))          # active when pass p starts
        done |= (codes[p] == codes[p - 1]).all(dim=1)
    return out


def skip_vs_all(q, x, iters=5, reps=20):
    q.skip_fixed_points = True
    a = q.encode(x, iters)
    t_skip = timed(lambda: q.encode(x, iters), reps)
    q.skip_fixed_points = False
    b = q.encode(x, iters)
    t_all = timed(lambda: q.encode(x, iters), reps)
    q.skip_fixed_points = True
    return {"default_ms": round(t_skip, 4), "all_passes_ms": round(t_all, 4), "gain": round(1 - t_skip / t_all, 4),
            "codes_identical": bool(torch.equal(a, b))}


def trainer_search(q, x, iters):
    """the trainer's fused search (mcq_logits_refine_codes: all passes) against the default path's int64 search"""
    L = _lib.lib()
    N, K, D = q.num_codebooks, q.codebook_size, q.dim
    B = x.shape[0]
    logits = torch.empty((B, N * K), dtype=torch.float32, device=x.device)
    idx = torch.empty((B, N), dtype=torch.int64, device=x.device)
    codes = torch.empty((B, N), dtype=torch.uint8, device=x.device)
    ws = torch.empty(L.mcq_encode_workspace_bytes(B, N, K, D), dtype=torch.uint8, device=x.device)
    blob = q._prepared()

    def fused():
        _lib.check(L.mcq_logits_refine_codes(x.data_ptr(), B, blob.data_ptr(), q._lscale_exp, N, K, D, iters, logits.data_ptr(),
                                             idx.data_ptr(), codes.data_ptr(), ws.data_ptr(), ws.numel(),
                                             torch.cuda.current_stream().cuda_stream, q._scale_flags), "refine_codes")
    return {"logits_refine_codes_all_passes_ms": round(timed(fused, 50), 4),
            "encode_int64_default_ms": round(timed(lambda: q.encode(x, iters, as_bytes=False), 50), 4)}


def main():
    res = {}
    with torch.no_grad():
        fx = fixtures.load("trained_d512_b8_p2")
        D, K, N = fx["D"], fx["K"], fx["N"]
        q = load_quantizer(fx["state"], D, K, N)
        x = torch.from_numpy(gen.make_kind(str(fx["x_kind"]), int(fx["x_seed"]) + 1000, 65536, D)).cuda()
        res["trained_d512_b8_p2"] = dict(skip_vs_all(q, x), active_at_pass_start=active_fractions(q, x),
                                         frames=f"make_kind({fx['x_kind']!r}, seed {int(fx['x_seed']) + 1000}, 65536)")
        res["trained_d512_b8_p2"]["trainer_batch_4096"] = trainer_search(q, x[:4096].contiguous(), 5)

        sd = gen.synthetic_state(103, 512, 256, 8)
        qb = load_quantizer(sd, 512, 256, 8)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(0)
        xb = torch.randn(65536, 512, generator=g, device="cuda:0")
        res["bench_state"] = dict(skip_vs_all(qb, xb), active_at_pass_start=active_fractions(qb, xb))
        res["bench_state"]["iters2_nothing_converges"] = skip_vs_all(qb, xb, iters=2)

        cross = {}
        for bs in (64, 1024, 4096, 8192, 16384, 32768):
            xs = xb[:bs].contiguous()
            row = {}
            os.environ["MCQ_SKIP_MIN_BATCH"] = "0"
            row["compaction_ms"] = round(timed(lambda: qb.encode(xs, 5), 50), 4)
            os.environ.pop("MCQ_SKIP_MIN_BATCH")
            qb.skip_fixed_points = False
            row["all_passes_ms"] = round(timed(lambda: qb.encode(xs, 5), 50), 4)
            qb.skip_fixed_points = True
            cross[str(bs)] = row
        res["bench_state"]["small_batch_crossover"] = cross
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
