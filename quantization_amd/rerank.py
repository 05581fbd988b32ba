"""The exact re-ranking of a shortlist (mcq_rerank, include/mcq_rerank.h rules 28-31): the step after search_wide and
search_lists_wide.  One HIP kernel gathers the raw rows a shortlist names, scores each against its query in fp32 and keeps the
k best; a second merges the parts of a row.  Every candidate row is read once, nothing of size (Q, S, D) is materialised, the
raw store is neither permuted nor copied, and padding needs no clamp: an entry that names no candidate issues no load.

    _, short = quantizer.search_lists_wide(queries, codes, list_offsets, probes, 1000, norms=norms)     # positions in list order
    dist, idx = rerank(queries, vectors, short, 10, row_of=order)          # vectors stay in their original order
    original = torch.where(idx >= 0, order[idx.clamp(min=0)], idx)

It needs no quantizer, so it is a function."""
import torch
from torch import Tensor

from . import _lib
from .search import METRICS, WIDE_MAX_K, _call, _on_device, check_metric

__all__ = ["rerank"]
MAX_DIM = 16384             # kRerankMaxD of mcq_rerank_kernels.h
_FLOATS = (torch.float32, torch.float16)


def _checked(queries, vectors, shortlist, k, metric, row_of):
    """shape, dtype and metric errors of rerank(): looks at no data, so it runs before any device work, on CPU tensors too"""
    check_metric(metric)
    if not isinstance(vectors, Tensor) or vectors.ndim != 2 or vectors.dtype not in _FLOATS:
        raise ValueError(f"vectors: an fp32 or fp16 (B, D) tensor, not {getattr(vectors, 'dtype', type(vectors))} "
                         f"{tuple(getattr(vectors, 'shape', ()))}")
    B, D = vectors.shape
    if not 1 <= D <= MAX_DIM:
        raise ValueError(f"vectors of dim {D}: 1 <= D <= {MAX_DIM}")
    if not vectors.is_contiguous():
        raise ValueError("vectors: contiguous rows (the raw store is never copied)")
    if not isinstance(queries, Tensor) or queries.ndim < 1 or queries.dtype not in _FLOATS or queries.shape[-1] != D:
        raise ValueError(f"queries: an fp32 or fp16 (*, {D}) tensor, not {getattr(queries, 'dtype', type(queries))} "
                         f"{tuple(getattr(queries, 'shape', ()))}")
    lead = tuple(queries.shape[:-1])
    if not isinstance(shortlist, Tensor) or shortlist.dtype not in (torch.int64, torch.int32) or shortlist.ndim < 1 or \
            tuple(shortlist.shape[:-1]) != lead:
        raise ValueError(f"shortlist: an int64 or int32 {lead} + (S,) tensor, not {getattr(shortlist, 'dtype', type(shortlist))} "
                         f"{tuple(getattr(shortlist, 'shape', ()))}")
    if row_of is not None and (not isinstance(row_of, Tensor) or row_of.dtype != torch.int64 or row_of.ndim != 1):
        raise ValueError(f"row_of: an int64 (Bs,) tensor, not {getattr(row_of, 'dtype', type(row_of))} "
                         f"{tuple(getattr(row_of, 'shape', ()))}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= WIDE_MAX_K:
        raise ValueError(f"k = {k!r}: an integer, 1 <= k <= {WIDE_MAX_K}")
    limit = (1 << 31) - 1
    if B >= limit or shortlist.shape[-1] >= limit or (row_of is not None and row_of.numel() >= limit):
        raise ValueError("vectors, shortlist and row_of: fewer than 2^31 - 1 rows and entries")
    return lead, int(B), int(D)


def rerank(queries: Tensor, vectors: Tensor, shortlist: Tensor, k: int, metric: str = "l2", row_of: Tensor = None):
    """Score the candidates a shortlist names against the raw vectors, exactly, and keep the k best of each query.

    queries (*, D) fp32 or fp16; vectors (B, D) fp32 or fp16 with contiguous rows, on the device (the two dtypes may differ);
    shortlist (*, S) int64 or int32 with the leading dimensions of queries -- what search_wide / search_lists_wide return as
    indexes.  An entry p with 0 <= p < Bs names a candidate, every other value none (-1 is the padding; B, 2**40 and -7
    likewise); Bs is row_of.numel() with row_of, else B; a position named twice in a row is a candidate twice.
    row_of: optional int64 (Bs,): candidate p is scored against vectors[row_of[p]], and an entry outside [0, B) makes p no
    candidate.  This is build_lists' `order`: the raw store stays in its original order and is never permuted or copied.
    Reported indexes stay the shortlist's positions p, like those of every other call of the search.
    1 <= k <= 1,024; k may exceed S.

    -> (values fp32 (*, k), indexes int64 (*, k)): "l2" |q - x|^2, nearest first; "ip" <q, x>, largest first; "cosine"
    cos(q, x), largest first, 0 for a zero query or a zero row.  Among equal values the lower position comes first.  The tail
    of a row with fewer than k candidates is (+inf, -1) under "l2" and (-inf, -1) under the other two.
    All arithmetic is fp32 in a fixed order (rule 29): a value depends on its two rows alone, not on the other arguments.
    Not differentiable; no CPU fallback (McqError); shape, dtype and metric errors are ValueErrors raised before any device
    work; nothing is read back to the host."""
    lead, B, D = _checked(queries, vectors, shortlist, k, metric, row_of)
    _on_device(queries, vectors, shortlist, row_of)
    S = int(shortlist.shape[-1])
    with torch.no_grad(), torch.cuda.device(vectors.device):
        dev = vectors.device
        q2d = queries.detach().reshape(-1, D).contiguous()
        short = shortlist.detach().reshape(-1, S).to(torch.int64).contiguous()
        x = vectors.detach()
        rows = None if row_of is None else row_of.detach().contiguous()
        Q = q2d.shape[0]
        Bs = B if rows is None else int(rows.numel())
        L = _lib.lib()
        ws = torch.empty((L.mcq_rerank_workspace_bytes(Q, S, D, k),), dtype=torch.uint8, device=dev)
        scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
        indexes = torch.empty((Q, k), dtype=torch.int64, device=dev)
        _call("mcq_rerank", q2d.data_ptr(), int(q2d.dtype == torch.float16), Q, x.data_ptr(), int(x.dtype == torch.float16), B, D,
              short.data_ptr(), S, None if rows is None else rows.data_ptr(), Bs, k, METRICS[metric], scores.data_ptr(),
              indexes.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(dev).cuda_stream)
        values = scores if metric == "l2" else -scores       # rule 29: the scores ascend; the tail +inf becomes -inf
        if metric == "cosine":                               # the score is -|q| cos: divide by |q| (1 for a zero query)
            qn = (q2d.to(torch.float32) ** 2).sum(dim=1, keepdim=True).sqrt()
            values = values / qn.masked_fill_(qn == 0, 1.0)
    return values.reshape(*lead, k), indexes.reshape(*lead, k)
