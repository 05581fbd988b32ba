"""The coarse centroids of an inverted file for fp32 rows on the bf16 matrix cores (include/mcq_split.h rules 60-63):
coarse_assign, kmeans_step and coarse_train of quantization_amd/coarse.py and kmeans.py with the assignment made from six
products of bf16 planes (v_mfma_f32_32x32x16_bf16, one fp32 accumulator a pair).  Both rows are split exactly into three bf16
planes -- the centroids once per call, the vectors in the kernel while a chunk is staged -- so the score is fp32-grade, within a
few roundings of the float64 value, but not the bits of coarse_assign: a row on a near-tie may land in the other list.  The
update is kmeans.py's as it stands, so kmeans_step_split's new centroids and counts are kmeans_step's bit for bit wherever the
two assignments agree.  No plane copy of the store and nothing of size (B, L).

    centroids = coarse_train_split(sample, 1024, iters=10, seed=0)     # (1024, D) fp32
    terms = coarse_terms(centroids)
    assign = coarse_assign_split(x, centroids, terms=terms)            # and on to build_lists

The training calls are "l2" only; there is no CPU path, and nothing is read back to the host.

The retrieval side (include/mcq_coarse_split.h rules 64-67): coarse_probe for fp32 queries on the same six products, under
the three metrics, the nprobe best of a query kept in a bounded heap:

    planes = coarse_planes_split(centroids)                            # once per centroid set, like coarse_terms
    probes, bias = coarse_probe_split(q, centroids, 32, terms=terms, planes=planes, with_bias=True)

Its scores are fp32-grade but not coarse_probe's bits, so on a near-tie the two may list another centroid; the biases of a
listed pair are coarse_probe's bit for bit.  Probes for bf16 queries are not built."""
import torch
from torch import Tensor

from .coarse import MAX_NPROBE, _checked, coarse_terms
from .kmeans import PLANES6, _assign, _checked_step, _public_step, _train
from .search import METRICS, _call, _entry, _on_device

__all__ = ["coarse_assign_split", "kmeans_step_split", "coarse_train_split", "coarse_planes_split", "coarse_probe_split"]


def coarse_assign_split(vectors: Tensor, centroids: Tensor, terms: Tensor = None) -> Tensor:
    """vectors (B, D) fp32, centroids (L, D) fp32, L >= 1, on the device -> int32 (B,): the nearest centroid of each vector
    under "l2" by the score of include/mcq_split.h rules 61 and 62, the lower list among equals, -1 for a row whose every score
    is NaN (a row with an infinite element is one).  It allocates its output, the part buffers (8 bytes per vector and part)
    and the three bf16 planes of the centroids; nothing of size (B, L).  terms: what coarse_terms(centroids) returned (computed
    here if None).  fp16 vectors are a ValueError that names coarse_assign_half, bf16 vectors one that names
    coarse_assign_bf16; no CPU fallback (McqError)."""
    B, L, D = _checked_step(vectors, centroids, terms, None, PLANES6, "coarse_assign")
    _on_device(vectors, centroids, terms)
    with torch.no_grad(), torch.cuda.device(vectors.device):
        c = centroids.detach().contiguous()
        return _assign(vectors.detach().contiguous(), c, coarse_terms(c) if terms is None else terms, None, B, L, D, PLANES6)[0]


def kmeans_step_split(vectors: Tensor, centroids: Tensor, terms: Tensor = None, prev_assign: Tensor = None):
    """vectors (B, D) fp32, centroids (L, D) fp32, L >= 1, on the device -> (new_centroids (L, D) fp32, assign int32 (B,),
    counts int32 (L,), changed): kmeans_step with assign = coarse_assign_split(vectors, centroids); new_centroids, counts and
    changed are kmeans_step's functions of that assignment (include/mcq_kmeans.h rules 45-47).
    Not differentiable; fp16 vectors are a ValueError that names kmeans_step_half, bf16 vectors one that names
    kmeans_step_bf16; no CPU fallback (McqError); shape and dtype errors are ValueErrors raised before any device work;
    nothing is read back to the host."""
    return _public_step(vectors, centroids, terms, prev_assign, PLANES6, "kmeans_step")


def coarse_train_split(vectors: Tensor, num_lists: int, iters: int = 10, seed: int = 0, init: Tensor = None) -> Tensor:
    """vectors (B, D) fp32 on the device -> centroids (num_lists, D) fp32: coarse_train with kmeans_step_split as its step:
    the same start (`init`, or num_lists distinct rows drawn by a torch.Generator seeded with `seed`), the same reseeding of
    empty lists.  The same vectors, seed or init, and iters give the same bits on every run.  fp16 vectors are a ValueError
    that names coarse_train_half, bf16 vectors one that names coarse_train_bf16; argument errors are ValueErrors raised before
    any device work; no CPU fallback."""
    return _train(vectors, num_lists, iters, seed, init, PLANES6, "coarse_train")


def _planes_shape(R, D):
    return (3 * R * 32 * -(-D // 32),)


def coarse_planes_split(centroids: Tensor) -> Tensor:
    """centroids (L, D) fp32 on the device -> int16 (3 L 32 ceil(D / 32),): the three bf16 planes of include/mcq_bf16.h rule 57,
    the hi rows, the mid rows and then the lo rows, each padded with zeros to a multiple of 32 elements: what coarse_probe_split
    takes as `planes`.  Once per centroid set, like coarse_terms."""
    L, D = _checked(None, centroids, "l2", None, "")
    _on_device(centroids)
    with torch.no_grad(), torch.cuda.device(centroids.device):
        c = centroids.detach().contiguous()
        planes = torch.empty(_planes_shape(L, D), dtype=torch.int16, device=c.device)
        _call("mcq_coarse_split_planes", c.data_ptr(), L, D, planes.data_ptr(), torch.cuda.current_stream(c.device).cuda_stream)
    return planes


def coarse_probe_split(queries: Tensor, centroids: Tensor, nprobe: int, metric: str = "l2", terms: Tensor = None,
                       planes: Tensor = None, with_bias: bool = False):
    """queries (*, D) fp32, centroids (L, D) fp32, on the device -> int32 (*, nprobe): coarse_probe on the bf16 matrix cores:
    per query the nprobe best lists, best first, by the score of include/mcq_coarse_split.h rule 65 (six products of the three
    bf16 planes of both rows, one fp32 accumulator a pair); among equal scores the lower list first; -1 where there are fewer
    than nprobe lists (or the score is NaN).  with_bias=True: -> (probes, fp32 (*, nprobe)): -2 <q, c> per probe from the fp32
    rows, 0 for a -1: the bits coarse_probe reports for the same pair.
    terms: what coarse_terms(centroids, metric) returned; planes: what coarse_planes_split(centroids) returned (each computed
    here if None: a serving process passes both).  1 <= nprobe <= 128.  It allocates its outputs, the part buffers and the
    three bf16 planes of the queries (6 bytes per padded element), nothing of size (Q, L).
    Not differentiable; fp16 queries are a ValueError that names coarse_probe_half, and no probe takes bf16 queries (a
    ValueError that says so); no CPU fallback (McqError); shape, dtype and metric errors are ValueErrors raised before any
    device work; nothing is read back to the host."""
    L, D = _checked(None, centroids, metric, terms, "")
    if isinstance(queries, Tensor) and queries.dtype == torch.float16:
        raise ValueError("queries: fp16 rows go to coarse_probe_half; coarse_probe_split takes torch.float32")
    if isinstance(queries, Tensor) and queries.dtype == torch.bfloat16:
        raise ValueError("queries: no probe takes bf16 rows; coarse_probe_split takes torch.float32")
    if not isinstance(queries, Tensor) or queries.ndim < 1 or queries.dtype != torch.float32 or queries.shape[-1] != D:
        raise ValueError(f"queries: an fp32 (*, {D}) tensor, not {getattr(queries, 'dtype', type(queries))} "
                         f"{tuple(getattr(queries, 'shape', ()))}")
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or not 1 <= nprobe <= MAX_NPROBE:
        raise ValueError(f"nprobe = {nprobe!r}: an integer, 1 <= nprobe <= {MAX_NPROBE}; use probe_lists (and probe_bias) beyond that")
    if planes is not None and (not isinstance(planes, Tensor) or planes.dtype != torch.int16 or
                               tuple(planes.shape) != _planes_shape(L, D) or not planes.is_contiguous()):
        raise ValueError(f"planes: what coarse_planes_split returned, a contiguous int16 {_planes_shape(L, D)} tensor, not "
                         f"{getattr(planes, 'dtype', type(planes))} {tuple(getattr(planes, 'shape', ()))}")
    _on_device(queries, centroids, terms, planes)
    lead, P, dev = tuple(queries.shape[:-1]), nprobe, centroids.device
    with torch.no_grad(), torch.cuda.device(dev):
        c, q = centroids.detach().contiguous(), queries.detach().reshape(-1, D).contiguous()
        if terms is None and metric != "ip":
            terms = coarse_terms(c, metric)
        if planes is None:
            planes = coarse_planes_split(c)
        Q = q.shape[0]
        parts = int(_entry("mcq_coarse_split_parts")(Q, L, D, P))
        lists = torch.empty((Q, P), dtype=torch.int32, device=dev)
        scores = torch.empty((Q, P), dtype=torch.float32, device=dev)
        bias = torch.empty((Q, P), dtype=torch.float32, device=dev) if with_bias else None
        part_score = torch.empty((Q, parts, P), dtype=torch.float32, device=dev)
        part_list = torch.empty((Q, parts, P), dtype=torch.int32, device=dev)
        query_planes = torch.empty(_planes_shape(Q, D), dtype=torch.int16, device=dev)
        _call("mcq_coarse_probe_split", q.data_ptr(), Q, c.data_ptr(), planes.data_ptr(), L, D,
              None if terms is None or metric == "ip" else terms.data_ptr(), P, METRICS[metric], parts, lists.data_ptr(),
              scores.data_ptr(), None if bias is None else bias.data_ptr(), part_score.data_ptr(), part_list.data_ptr(),
              query_planes.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    lists = lists.reshape(*lead, P)
    return (lists, bias.reshape(*lead, P)) if with_bias else lists
