"""The coarse centroids of an inverted file over an fp16 raw store (include/mcq_half.h rules 48-51): coarse_assign, kmeans_step
and coarse_train of quantization_amd/coarse.py and kmeans.py for torch.float16 vectors, with no fp32 copy of the store and
nothing of size (B, L).  The centroids stay fp32 -- they are means -- and are split once per call into two fp16 planes (hi, and
the rest times 2^11) that the vectors meet on the f16 matrix cores (v_mfma_f32_32x32x16_f16, two fp32 accumulators a pair); the
update widens every fp16 element exactly into the float64 tree of rule 47, so kmeans_step_half(x, c)'s new centroids and counts
are kmeans_step(x.float(), c)'s bit for bit wherever the two assignments agree.

    centroids = coarse_train_half(store16, 1024, iters=10, seed=0)    # (1024, D) fp32
    terms = coarse_terms(centroids)
    assign = coarse_assign_half(store16, centroids, terms=terms)      # and on to build_lists

The serving side (include/mcq_coarse_half.h rules 52-55): coarse_probe for torch.float16 queries on the same matrix cores, the
nprobe best lists per query under all three metrics and the bias a store of residual codes takes.  The planes of a centroid
set are made once:

    planes = coarse_planes(centroids)                                 # once per centroid set, like the terms
    probes, bias = coarse_probe_half(q16, centroids, 16, terms=terms, planes=planes, with_bias=True)
    dist, idx = quantizer.search_lists(q16.float(), codes, list_offsets, probes, k=10, norms=norms, probe_bias=bias)

The training side is "l2" only; there is no CPU path, and nothing is read back to the host."""
import torch
from torch import Tensor

from .coarse import MAX_NPROBE, _checked, coarse_terms
from .kmeans import _assign, _checked_step, _public_step, _train
from .search import METRICS, _call, _entry, _on_device

__all__ = ["coarse_assign_half", "kmeans_step_half", "coarse_train_half", "coarse_planes", "coarse_probe_half"]


def coarse_assign_half(vectors: Tensor, centroids: Tensor, terms: Tensor = None) -> Tensor:
    """vectors (B, D) fp16, centroids (L, D) fp32, L >= 1, on the device -> int32 (B,): the nearest centroid of each vector
    under "l2" by the score of include/mcq_half.h rule 49, the lower list among equals, -1 for a row whose every score is NaN.
    It allocates its output, the part buffers (8 bytes per vector and part) and the two fp16 planes of the centroids; no fp32
    copy of the vectors and nothing of size (B, L).  terms: what coarse_terms(centroids) returned (computed here if None).
    fp32 vectors are a ValueError that names coarse_assign; no CPU fallback (McqError)."""
    B, L, D = _checked_step(vectors, centroids, terms, None, torch.float16, "coarse_assign")
    _on_device(vectors, centroids, terms)
    with torch.no_grad(), torch.cuda.device(vectors.device):
        c = centroids.detach().contiguous()
        return _assign(vectors.detach().contiguous(), c, coarse_terms(c) if terms is None else terms, None, B, L, D)[0]


def kmeans_step_half(vectors: Tensor, centroids: Tensor, terms: Tensor = None, prev_assign: Tensor = None):
    """vectors (B, D) fp16, centroids (L, D) fp32, L >= 1, on the device -> (new_centroids (L, D) fp32, assign int32 (B,),
    counts int32 (L,), changed): kmeans_step for an fp16 store.  assign is coarse_assign_half(vectors, centroids);
    new_centroids[l] is the mean of list l's rows, each fp16 element widened exactly, over the fixed float64 tree of
    include/mcq_kmeans.h rule 47, rounded once; a list without rows keeps its centroid and counts 0.  changed is a device tensor
    of one int32, the number of rows whose assignment differs from prev_assign, or None without one.
    Not differentiable; fp32 vectors are a ValueError that names kmeans_step; no CPU fallback (McqError); shape and dtype errors
    are ValueErrors raised before any device work; nothing is read back to the host."""
    return _public_step(vectors, centroids, terms, prev_assign, torch.float16, "kmeans_step")


def coarse_train_half(vectors: Tensor, num_lists: int, iters: int = 10, seed: int = 0, init: Tensor = None) -> Tensor:
    """vectors (B, D) fp16 on the device -> centroids (num_lists, D) fp32: coarse_train for an fp16 store: `iters` steps
    (kmeans_step_half) from `init` -- (num_lists, D) fp32 rows -- or, without one, from num_lists distinct rows of `vectors`,
    widened to fp32, drawn by a torch.Generator seeded with `seed`.  After each step an empty list is reseeded from the largest
    as in coarse_train.  The same vectors, seed or init, and iters give the same bits on every run.  fp32 vectors are a
    ValueError that names coarse_train; argument errors are ValueErrors raised before any device work; no CPU fallback."""
    return _train(vectors, num_lists, iters, seed, init, torch.float16, "coarse_train")


def _planes_shape(L, D):
    return (2 * L * 32 * -(-D // 32),)


def coarse_planes(centroids: Tensor) -> Tensor:
    """centroids (L, D) fp32 on the device -> int16 (2 L 32 ceil(D / 32),): the two fp16 planes of include/mcq_half.h rule 49,
    the hi rows and then the lo rows, each padded with zeros to a multiple of 32 halves: what coarse_probe_half takes as
    `planes`.  Once per centroid set, like coarse_terms."""
    L, D = _checked(None, centroids, "l2", None, "")
    _on_device(centroids)
    with torch.no_grad(), torch.cuda.device(centroids.device):
        c = centroids.detach().contiguous()
        planes = torch.empty(_planes_shape(L, D), dtype=torch.int16, device=c.device)
        _call("mcq_coarse_half_split", c.data_ptr(), L, D, planes.data_ptr(), torch.cuda.current_stream(c.device).cuda_stream)
    return planes


def coarse_probe_half(queries: Tensor, centroids: Tensor, nprobe: int, metric: str = "l2", terms: Tensor = None,
                      planes: Tensor = None, with_bias: bool = False):
    """queries (*, D) fp16, centroids (L, D) fp32, on the device -> int32 (*, nprobe): coarse_probe for fp16 queries: per query
    the nprobe best lists, best first, by the score of include/mcq_coarse_half.h rule 53 (the f16 matrix cores against the two
    fp16 planes of the centroids); among equal scores the lower list first; -1 where there are fewer than nprobe lists (or the
    score is NaN).  with_bias=True: -> (probes, fp32 (*, nprobe)): -2 <q, c> per probe from the fp32 centroid row, 0 for a -1:
    the bits coarse_probe(queries.float(), ...) reports for the same pair.
    terms: what coarse_terms(centroids, metric) returned; planes: what coarse_planes(centroids) returned (each computed here if
    None: a serving process passes both).  1 <= nprobe <= 128.  It allocates its outputs and the part buffers, nothing of size
    (Q, L) and no fp32 copy of the queries.
    Not differentiable; fp32 queries are a ValueError that names coarse_probe; no CPU fallback (McqError); shape, dtype and
    metric errors are ValueErrors raised before any device work; nothing is read back to the host."""
    L, D = _checked(None, centroids, metric, terms, "")
    if isinstance(queries, Tensor) and queries.dtype == torch.float32:
        raise ValueError("queries: fp32 rows go to coarse_probe; coarse_probe_half takes torch.float16")
    if not isinstance(queries, Tensor) or queries.ndim < 1 or queries.dtype != torch.float16 or queries.shape[-1] != D:
        raise ValueError(f"queries: an fp16 (*, {D}) tensor, not {getattr(queries, 'dtype', type(queries))} "
                         f"{tuple(getattr(queries, 'shape', ()))}")
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 1 <= nprobe <= MAX_NPROBE:
        raise ValueError(f"nprobe = {nprobe!r}: an integer, 1 <= nprobe <= {MAX_NPROBE}; use probe_lists (and probe_bias) beyond that")
    if planes is not None and (not isinstance(planes, Tensor) or planes.dtype != torch.int16 or
                               tuple(planes.shape) != _planes_shape(L, D) or not planes.is_contiguous()):
        raise ValueError(f"planes: what coarse_planes returned, a contiguous int16 {_planes_shape(L, D)} tensor, not "
                         f"{getattr(planes, 'dtype', type(planes))} {tuple(getattr(planes, 'shape', ()))}")
    _on_device(queries, centroids, terms, planes)
    lead, P, dev = tuple(queries.shape[:-1]), nprobe, centroids.device
    with torch.no_grad(), torch.cuda.device(dev):
        c, q = centroids.detach().contiguous(), queries.detach().reshape(-1, D).contiguous()
        if terms is None and metric != "ip":
            terms = coarse_terms(c, metric)
        if planes is None:
            planes = coarse_planes(c)
        Q = q.shape[0]
        parts = int(_entry("mcq_coarse_half_parts")(Q, L, D, P))
        lists = torch.empty((Q, P), dtype=torch.int32, device=dev)
        scores = torch.empty((Q, P), dtype=torch.float32, device=dev)
        bias = torch.empty((Q, P), dtype=torch.float32, device=dev) if with_bias else None
        part_score = torch.empty((Q, parts, P), dtype=torch.float32, device=dev)
        part_list = torch.empty((Q, parts, P), dtype=torch.int32, device=dev)
        _call("mcq_coarse_probe_half", q.data_ptr(), Q, c.data_ptr(), planes.data_ptr(), L, D,
              None if terms is None or metric == "ip" else terms.data_ptr(), P, METRICS[metric], parts, lists.data_ptr(),
              scores.data_ptr(), None if bias is None else bias.data_ptr(), part_score.data_ptr(), part_list.data_ptr(),
              torch.cuda.current_stream(dev).cuda_stream)
    lists = lists.reshape(*lead, P)
    return (lists, bias.reshape(*lead, P)) if with_bias else lists
