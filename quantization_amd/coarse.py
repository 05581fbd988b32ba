"""The coarse quantizer of an inverted file in HIP (mcq_coarse_probe, include/mcq_coarse.h rules 40-43): what probe_lists and
probe_bias of quantization_amd/ivf.py do with two matmuls, a topk and a gather, and the assignment of a store to its cells,
which is the same kernel at nprobe = 1.  One kernel scores a tile of 32 queries against the centroids on the fp32 matrix cores
and keeps the nprobe best per query in LDS; a second merges the parts and recomputes <q, c> for the winners alone.  Nothing of
size (Q, L) is materialised, ties go to the lower list, and every value is a stated function of its two rows.

    terms = coarse_terms(centroids)                                    # once per centroid set
    assign = coarse_assign(x, centroids, terms=terms)                  # build_lists' `assign`
    probes, bias = coarse_probe(queries, centroids, 16, terms=terms, with_bias=True)
    dist, idx = quantizer.search_lists(queries, codes, list_offsets, probes, k=10, norms=norms, probe_bias=bias)

There is no CPU path; probe_lists and probe_bias stay as they are for CPU tensors and for nprobe past 128."""
import torch
from torch import Tensor

from . import _lib
from .search import METRICS, _call, _entry, _on_device, check_metric

__all__ = ["coarse_terms", "coarse_probe", "coarse_assign"]
MAX_DIM = 16384             # kCoarseMaxD of mcq_coarse_kernels.h
MAX_NPROBE = 128            # kCoarseMaxP


def _checked(rows, centroids, metric, terms, what):
    """shape, dtype and metric errors: looks at no data, so it runs before any device work, on CPU tensors too"""
    check_metric(metric)
    if not isinstance(centroids, Tensor) or centroids.ndim != 2 or centroids.dtype != torch.float32:
        raise ValueError(f"centroids: an fp32 (L, D) tensor, not {getattr(centroids, 'dtype', type(centroids))} "
                         f"{tuple(getattr(centroids, 'shape', ()))}")
    L, D = centroids.shape
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"centroids of dim {D}: 1 <= D <= {MAX_DIM}")
    if L >= (1 << 31) - 1:
        raise ValueError("centroids: fewer than 2^31 - 1 rows")
    if rows is not None and (not isinstance(rows, Tensor) or rows.ndim < 1 or rows.dtype != torch.float32 or rows.shape[-1] != D):
        raise ValueError(f"{what}: an fp32 (*, {D}) tensor, not {getattr(rows, 'dtype', type(rows))} "
                         f"{tuple(getattr(rows, 'shape', ()))}")
    if terms is not None and (not isinstance(terms, Tensor) or terms.dtype != torch.float32 or tuple(terms.shape) != (L,)):
        raise ValueError(f"terms: what coarse_terms returned, an fp32 ({L},) tensor, not {getattr(terms, 'dtype', type(terms))} "
                         f"{tuple(getattr(terms, 'shape', ()))}")
    return int(L), int(D)


def coarse_terms(centroids: Tensor, metric: str = "l2"):
    """centroids (L, D) fp32 -> fp32 (L,): the per-centroid term of the score, computed once per centroid set: 0.5 |c|^2 under
    "l2", 1 / |c| (0 for a zero row) under "cosine"; None under "ip"."""
    L, D = _checked(None, centroids, metric, None, "")
    _on_device(centroids)
    if metric == "ip":
        return None
    with torch.no_grad(), torch.cuda.device(centroids.device):
        c = centroids.detach().contiguous()
        terms = torch.empty((L,), dtype=torch.float32, device=c.device)
        _call("mcq_coarse_terms", c.data_ptr(), L, D, METRICS[metric], terms.data_ptr(),
              torch.cuda.current_stream(c.device).cuda_stream)
    return terms


def _probe(q2d, centroids, L, D, P, metric, terms, with_bias):
    """the entry on (Q, D) rows: allocates the outputs and the part buffers, nothing else"""
    dev = centroids.device
    with torch.no_grad(), torch.cuda.device(dev):
        c = centroids.detach().contiguous()
        if terms is None and metric != "ip":
            terms = coarse_terms(c, metric)
        Q = q2d.shape[0]
        parts = int(_entry("mcq_coarse_parts")(Q, L, D, P))
        lists = torch.empty((Q, P), dtype=torch.int32, device=dev)
        scores = torch.empty((Q, P), dtype=torch.float32, device=dev)
        bias = torch.empty((Q, P), dtype=torch.float32, device=dev) if with_bias else None
        part_score = torch.empty((Q, parts, P), dtype=torch.float32, device=dev)
        part_list = torch.empty((Q, parts, P), dtype=torch.int32, device=dev)
        _call("mcq_coarse_probe", q2d.data_ptr(), Q, c.data_ptr(), L, D, None if terms is None else terms.data_ptr(), P,
              METRICS[metric], parts, lists.data_ptr(), scores.data_ptr(), None if bias is None else bias.data_ptr(),
              part_score.data_ptr(), part_list.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return lists, bias


def coarse_probe(queries: Tensor, centroids: Tensor, nprobe: int, metric: str = "l2", terms: Tensor = None,
                 with_bias: bool = False):
    """queries (*, D) fp32, centroids (L, D) fp32, on the device -> int32 (*, nprobe): per query the nprobe best lists, best
    first -- the nearest centroids under "l2", the largest inner products under "ip", the largest cosines under "cosine";
    among equal scores the lower list first; -1 where there are fewer than nprobe lists (or the score is NaN).
    with_bias=True: -> (probes, fp32 (*, nprobe)): -2 <q, c> per probe, 0 for a -1: what search_lists(probe_bias=) and
    range_search_lists(probe_bias=) take for a store of residual codes.
    terms: what coarse_terms(centroids, metric) returned (computed here if None).  1 <= nprobe <= 128; past that, probe_lists.
    Not differentiable; no CPU fallback (McqError); shape, dtype and metric errors are ValueErrors raised before any device
    work; nothing is read back to the host."""
    L, D = _checked(queries, centroids, metric, terms, "queries")
    if isinstance(nprobe, bool) or not isinstance(nprobe, int) or nprobe < 1:
        raise ValueError(f"nprobe = {nprobe!r}: an integer, 1 <= nprobe <= {MAX_NPROBE}")
    if nprobe > MAX_NPROBE:
        raise ValueError(f"nprobe = {nprobe}: coarse_probe keeps at most {MAX_NPROBE} lists per query; use probe_lists "
                         "(and probe_bias) beyond that")
    _on_device(queries, centroids, terms)
    lead = tuple(queries.shape[:-1])
    lists, bias = _probe(queries.detach().reshape(-1, D).contiguous(), centroids, L, D, nprobe, metric, terms, bool(with_bias))
    lists = lists.reshape(*lead, nprobe)
    return (lists, bias.reshape(*lead, nprobe)) if with_bias else lists


def coarse_assign(vectors: Tensor, centroids: Tensor, metric: str = "l2", terms: Tensor = None) -> Tensor:
    """vectors (B, D) fp32, centroids (L, D) fp32, L >= 1, on the device -> int32 (B,): the best list of each vector, the lower
    one among equals: the `assign` build_lists takes and a k-means iteration needs.  coarse_probe at nprobe = 1 without a
    bias; it allocates its output and the part buffers (8 bytes per vector and part) and nothing of size (B, L)."""
    L, D = _checked(vectors, centroids, metric, terms, "vectors")
    if vectors.ndim != 2:
        raise ValueError(f"vectors: an fp32 (B, {D}) tensor, not {tuple(vectors.shape)}")
    if L < 1:
        raise ValueError("centroids: at least one list to assign to")
    _on_device(vectors, centroids, terms)
    lists, _ = _probe(vectors.detach().contiguous(), centroids, L, D, 1, metric, terms, False)
    return lists.reshape(-1)
