"""An inverted file over a store of codes: the torch plumbing round Quantizer.search_lists and Quantizer.range_search_lists
(no hot path; the scoring is mcq_search_scan_lists and mcq_search_range_lists_count / _fill).

    order, list_offsets = build_lists(assign, num_lists)       # once per store: assign[b] = the coarse cell of vector b
    codes, norms = codes[order], norms[order]                  # the store in list order
    probes = probe_lists(queries, centroids, nprobe)           # per call: the nprobe nearest cells of each query
    dist, idx = quantizer.search_lists(queries, codes, list_offsets, probes, k=10, norms=norms)
    original = torch.where(idx >= 0, order[idx.clamp(min=0)], idx)
    lims, dist, idx = quantizer.range_search_lists(queries, codes, list_offsets, probes, radius, norms=norms)
    original = order[idx]                                      # every hit within the radius in the probed lists, as CSR

A store of RESIDUAL codes (IVFADC): list l keeps the codes of x - centroids[l], so the bytes spend their precision inside the
cell.  The centroid's share of a score comes back as one value per (query, probe), and the norms are those of centroid + decode:

    codes = quantizer.encode(x - centroids[assign], as_bytes=True)              # the residuals' codes
    order, list_offsets = build_lists(assign, num_lists)
    codes = codes[order]                                                          # in list order
    norms = quantizer.code_norms(codes, base=centroids, assign=list_assign(list_offsets, B))
    probes = probe_lists(queries, centroids, nprobe)
    dist, idx = quantizer.search_lists(queries, codes, list_offsets, probes, k=10, norms=norms,
                                       probe_bias=probe_bias(queries, centroids, probes))
    lims, dist, idx = quantizer.range_search_lists(queries, codes, list_offsets, probes, radius, norms=norms,
                                                   probe_bias=probe_bias(queries, centroids, probes))

A shortlist for an exact re-ranker (recall@100, recall@1000): search_lists stops at k = 64, search_lists_wide goes to 1,024.

    _, short = quantizer.search_lists_wide(queries, codes, list_offsets, probes, 1000, norms=norms)     # (Q, 1000), -1 = none
    dist, idx = quantization_amd.rerank(queries, vectors, short, 10, row_of=order)      # exact |q - x|^2 of the raw vectors
    original = torch.where(idx >= 0, order[idx.clamp(min=0)], idx)

rerank (quantization_amd/rerank.py, mcq_rerank) reads every candidate's raw row once; `vectors` stays in its original order,
row_of = order maps a position of the store in list order to its row, and the -1 padding is skipped, not clamped.

Two-stage quantisation (faiss's IndexRefine / IVFPQR): cheap codes in the inverted file find the candidates, a second, finer
Quantizer over the SAME vectors -- 32 to 64 bytes a vector where the raw row takes 2 KB -- rescores them, and only then, if at
all, is raw data touched.  The fine codes stay in the original order, as the raw vectors do:

    fine_codes = fine.encode(x, as_bytes=True); fine_norms = fine.code_norms(fine_codes)      # once, original order
    _, short = coarse.search_lists_wide(queries, codes, list_offsets, probes, 1000, norms=norms)        # positions in list order
    dist, idx = fine.search_shortlist(queries, fine_codes, short, 100, norms=fine_norms, row_of=order)  # the fine codes' ADC
    dist, idx = quantization_amd.rerank(queries, vectors, idx, 10, row_of=order)                        # optional: exact
    original = torch.where(idx >= 0, order[idx.clamp(min=0)], idx)

search_shortlist (quantization_amd/search.py, mcq_search_shortlist) reads the fine codes of the named rows and nothing else;
its values are the bits fine.search reports for the same (query, vector), and its indexes stay positions in list order.

Where the coarse centroids come from (k-means over a sample, a trained layer) is the caller's business."""
import torch
from torch import Tensor

from .search import check_metric

__all__ = ["build_lists", "probe_lists", "probe_bias", "list_assign"]


def build_lists(assign: Tensor, num_lists: int):
    """assign (B,) integer, assign[b] in [0, num_lists) -> (order int64 (B,), list_offsets int64 (num_lists + 1,)).
    order is the STABLE sort of the assignments: list l is order[list_offsets[l]:list_offsets[l + 1]], in ascending original
    position.  The caller stores codes[order] (and norms[order], and a packed mask of keep[order]) and maps a result back
    through order."""
    if not isinstance(assign, Tensor) or assign.ndim != 1 or assign.dtype.is_floating_point or assign.dtype == torch.bool:
        raise ValueError(f"assign: an integer (B,) tensor, not {getattr(assign, 'dtype', type(assign))} "
                         f"{tuple(getattr(assign, 'shape', ()))}")
    num_lists = int(num_lists)
    if num_lists < 0 or (assign.numel() and num_lists == 0):
        raise ValueError(f"{num_lists} lists for {assign.numel()} vectors")
    a = assign.detach().to(torch.int64)
    if a.numel() and (int(a.min()) < 0 or int(a.max()) >= num_lists):
        raise ValueError(f"assign holds values outside [0, {num_lists})")
    order = torch.sort(a, stable=True).indices
    counts = torch.bincount(a, minlength=num_lists)
    offsets = torch.zeros(num_lists + 1, dtype=torch.int64, device=a.device)
    offsets[1:] = torch.cumsum(counts, dim=0)
    return order, offsets


def probe_lists(queries: Tensor, centroids: Tensor, nprobe: int, metric: str = "l2") -> Tensor:
    """queries (*, dim), centroids (L, dim) -> int32 (*, nprobe): per query the nprobe best lists, best first -- the nearest
    centroids under "l2", the largest inner products under "ip", the largest cosines under "cosine".  One matmul and one
    topk; the rows hold distinct lists by construction."""
    check_metric(metric)
    if not isinstance(centroids, Tensor) or centroids.ndim != 2 or queries.shape[-1] != centroids.shape[1]:
        raise ValueError(f"centroids: an (L, {queries.shape[-1]}) tensor, not {tuple(getattr(centroids, 'shape', ()))}")
    nprobe = int(nprobe)
    if not 1 <= nprobe <= centroids.shape[0]:
        raise ValueError(f"nprobe {nprobe} for {centroids.shape[0]} lists")
    with torch.no_grad():
        q = queries.detach().reshape(-1, queries.shape[-1]).to(torch.float32)
        c = centroids.detach().to(torch.float32)
        sim = q @ c.t()
        if metric == "l2":                                  # |q - c|^2 = |q|^2 - 2 <q, c> + |c|^2: |q|^2 does not order the lists
            sim = sim - 0.5 * (c * c).sum(dim=1)[None, :]
        elif metric == "cosine":
            cn = (c * c).sum(dim=1).sqrt()
            sim = sim / cn.masked_fill(cn == 0, 1.0)[None, :]
        top = torch.topk(sim, nprobe, dim=1).indices.to(torch.int32)
    return top.reshape(*queries.shape[:-1], nprobe)


def probe_bias(queries: Tensor, centroids: Tensor, probes: Tensor) -> Tensor:
    """queries (*, dim), centroids (L, dim), probes (*, P) integer as search_lists takes them -> fp32 (*, P):
    -2 <queries[q], centroids[probes[q][p]]>, and 0 where an entry names no list.  What search_lists(probe_bias=...) adds to
    the table sums of a store of residual codes.  One matmul and one gather."""
    if not isinstance(centroids, Tensor) or centroids.ndim != 2 or queries.shape[-1] != centroids.shape[1]:
        raise ValueError(f"centroids: an (L, {queries.shape[-1]}) tensor, not {tuple(getattr(centroids, 'shape', ()))}")
    if not isinstance(probes, Tensor) or probes.dtype.is_floating_point or probes.dtype == torch.bool or probes.ndim < 1 or \
            tuple(probes.shape[:-1]) != tuple(queries.shape[:-1]):
        raise ValueError(f"probes: an integer {tuple(queries.shape[:-1])} + (P,) tensor, not "
                         f"{getattr(probes, 'dtype', type(probes))} {tuple(getattr(probes, 'shape', ()))}")
    with torch.no_grad():
        q = queries.detach().reshape(-1, queries.shape[-1]).to(torch.float32)
        c = centroids.detach().to(torch.float32)
        p = probes.detach().reshape(q.shape[0], probes.shape[-1]).to(torch.int64)
        named = (p >= 0) & (p < c.shape[0])
        if c.shape[0] == 0:
            return torch.zeros(probes.shape, dtype=torch.float32, device=q.device)
        dots = torch.gather(q @ c.t(), 1, p.clamp(0, c.shape[0] - 1))
        out = torch.where(named, -2.0 * dots, torch.zeros_like(dots))
    return out.reshape(probes.shape)


def list_assign(list_offsets: Tensor, B: int) -> Tensor:
    """list_offsets int64 (L + 1,) as build_lists returned them, B the length of the store -> int32 (B,): the list of each
    position of the store in list order, -1 for a position outside every list.  What code_norms(base=centroids, assign=...)
    takes for a store of residual codes."""
    if not isinstance(list_offsets, Tensor) or list_offsets.dtype != torch.int64 or list_offsets.ndim != 1 or list_offsets.numel() < 1:
        raise ValueError(f"list_offsets: an int64 (L + 1,) tensor, not {getattr(list_offsets, 'dtype', type(list_offsets))} "
                         f"{tuple(getattr(list_offsets, 'shape', ()))}")
    B = int(B)
    if B < 0:
        raise ValueError(f"a store of {B} vectors")
    off = list_offsets.detach()
    pos = torch.arange(B, dtype=torch.int64, device=off.device)
    l = torch.searchsorted(off, pos, right=True) - 1                # the last l with off[l] <= b: an empty list is passed
    inside = (l >= 0) & (l < off.numel() - 1)
    return torch.where(inside, l, torch.full_like(l, -1)).to(torch.int32)
