"""The coarse centroids of an inverted file over an fp16 raw store (include/mcq_half.h rules 48-51): coarse_assign, kmeans_step
and coarse_train of quantization_amd/coarse.py and kmeans.py for torch.float16 vectors, with no fp32 copy of the store and
nothing of size (B, L).  The centroids stay fp32 -- they are means -- and are split once per call into two fp16 planes (hi, and
the rest times 2^11) that the vectors meet on the f16 matrix cores (v_mfma_f32_32x32x16_f16, two fp32 accumulators a pair); the
update widens every fp16 element exactly into the float64 tree of rule 47, so kmeans_step_half(x, c)'s new centroids and counts
are kmeans_step(x.float(), c)'s bit for bit wherever the two assignments agree.

    centroids = coarse_train_half(store16, 1024, iters=10, seed=0)    # (1024, D) fp32
    terms = coarse_terms(centroids)
    assign = coarse_assign_half(store16, centroids, terms=terms)      # and on to build_lists

"l2" only; there is no CPU path, and nothing is read back to the host."""
import torch
from torch import Tensor

from .coarse import MAX_DIM, _checked, coarse_terms
from .kmeans import _reseed
from .search import _call, _entry, _on_device

__all__ = ["coarse_assign_half", "kmeans_step_half", "coarse_train_half"]


def _checked_half(vectors, centroids, terms, prev_assign, fp32_name):
    """shape and dtype errors: looks at no data, so it runs before any device work, on CPU tensors too"""
    L, D = _checked(None, centroids, "l2", terms, "")
    if isinstance(vectors, Tensor) and vectors.dtype == torch.float32:
        raise ValueError(f"vectors: fp32 rows go to {fp32_name}; this call takes torch.float16")
    if not isinstance(vectors, Tensor) or vectors.dtype != torch.float16 or vectors.ndim != 2 or vectors.shape[1] != D:
        raise ValueError(f"vectors: an fp16 (B, {D}) tensor, not {getattr(vectors, 'dtype', type(vectors))} "
                         f"{tuple(getattr(vectors, 'shape', ()))}")
    if L < 1:
        raise ValueError("centroids: at least one list to assign to")
    B = int(vectors.shape[0])
    if B >= (1 << 31) - 1:
        raise ValueError("vectors: fewer than 2^31 - 1 rows")
    if prev_assign is not None and (not isinstance(prev_assign, Tensor) or prev_assign.dtype != torch.int32 or
                                    tuple(prev_assign.shape) != (B,)):
        raise ValueError(f"prev_assign: the int32 ({B},) tensor an earlier step returned, not "
                         f"{getattr(prev_assign, 'dtype', type(prev_assign))} {tuple(getattr(prev_assign, 'shape', ()))}")
    return B, L, D


def _assign(x, c, terms, prev, B, L, D):
    """x (B, D) fp16 and c (L, D) fp32 contiguous on one device: the entry, its outputs and its scratch"""
    dev = x.device
    parts = int(_entry("mcq_kmeans_half_parts")(B, L, D))
    assign = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    changed = None if prev is None else torch.empty((1,), dtype=torch.int32, device=dev)
    part_score = torch.empty((B, parts), dtype=torch.float32, device=dev)
    part_list = torch.empty((B, parts), dtype=torch.int32, device=dev)
    planes = torch.empty((int(_entry("mcq_kmeans_half_planes")(L, D)),), dtype=torch.int16, device=dev)
    _call("mcq_kmeans_assign_half", x.data_ptr(), B, c.data_ptr(), L, D, terms.data_ptr(), parts,
          None if prev is None else prev.data_ptr(), assign.data_ptr(), score.data_ptr(),
          None if changed is None else changed.data_ptr(), part_score.data_ptr(), part_list.data_ptr(), planes.data_ptr(),
          torch.cuda.current_stream(dev).cuda_stream)
    return assign, changed


def _step(x, c, terms, prev, B, L, D):
    """the two entries and the sort between them, as kmeans._step"""
    dev = x.device
    if terms is None:
        terms = coarse_terms(c)
    assign, changed = _assign(x, c, terms, prev, B, L, D)
    # the stable sort by list: ascending original position inside a list; a row assigned -1 sorts behind list L - 1
    key = torch.where(assign < 0, torch.full_like(assign, L), assign).to(torch.int64)
    keys, order = torch.sort(key, stable=True)
    offsets = torch.searchsorted(keys, torch.arange(L + 1, dtype=torch.int64, device=dev))
    new = torch.empty_like(c)
    counts = torch.empty((L,), dtype=torch.int32, device=dev)
    block_first = torch.empty((L + 1,), dtype=torch.int64, device=dev)
    block_sums = torch.empty((int(_entry("mcq_kmeans_blocks")(B, L, D)),), dtype=torch.float64, device=dev)
    _call("mcq_kmeans_update_half", x.data_ptr(), B, D, order.data_ptr(), offsets.data_ptr(), L, c.data_ptr(), new.data_ptr(),
          counts.data_ptr(), block_first.data_ptr(), block_sums.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return new, assign, counts, changed


def coarse_assign_half(vectors: Tensor, centroids: Tensor, terms: Tensor = None) -> Tensor:
    """vectors (B, D) fp16, centroids (L, D) fp32, L >= 1, on the device -> int32 (B,): the nearest centroid of each vector
    under "l2" by the score of include/mcq_half.h rule 49, the lower list among equals, -1 for a row whose every score is NaN.
    It allocates its output, the part buffers (8 bytes per vector and part) and the two fp16 planes of the centroids; no fp32
    copy of the vectors and nothing of size (B, L).  terms: what coarse_terms(centroids) returned (computed here if None).
    fp32 vectors are a ValueError that names coarse_assign; no CPU fallback (McqError)."""
    B, L, D = _checked_half(vectors, centroids, terms, None, "coarse_assign")
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
    B, L, D = _checked_half(vectors, centroids, terms, prev_assign, "kmeans_step")
    _on_device(vectors, centroids, terms, prev_assign)
    with torch.no_grad(), torch.cuda.device(vectors.device):
        return _step(vectors.detach().contiguous(), centroids.detach().contiguous(), terms,
                     None if prev_assign is None else prev_assign.detach().contiguous(), B, L, D)


def coarse_train_half(vectors: Tensor, num_lists: int, iters: int = 10, seed: int = 0, init: Tensor = None) -> Tensor:
    """vectors (B, D) fp16 on the device -> centroids (num_lists, D) fp32: coarse_train for an fp16 store: `iters` steps
    (kmeans_step_half) from `init` -- (num_lists, D) fp32 rows -- or, without one, from num_lists distinct rows of `vectors`,
    widened to fp32, drawn by a torch.Generator seeded with `seed`.  After each step an empty list is reseeded from the largest
    as in coarse_train.  The same vectors, seed or init, and iters give the same bits on every run.  fp32 vectors are a
    ValueError that names coarse_train; argument errors are ValueErrors raised before any device work; no CPU fallback."""
    if isinstance(num_lists, bool) or not isinstance(num_lists, int) or num_lists < 1:
        raise ValueError(f"num_lists = {num_lists!r}: a positive integer")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"iters = {iters!r}: a non-negative integer")
    if isinstance(vectors, Tensor) and vectors.dtype == torch.float32:
        raise ValueError("vectors: fp32 rows go to coarse_train; this call takes torch.float16")
    if not isinstance(vectors, Tensor) or vectors.ndim != 2 or vectors.dtype != torch.float16 or \
            not 1 <= vectors.shape[1] <= MAX_DIM:
        raise ValueError(f"vectors: an fp16 (B, D) tensor, 1 <= D <= {MAX_DIM}, not {getattr(vectors, 'dtype', type(vectors))} "
                         f"{tuple(getattr(vectors, 'shape', ()))}")
    B, D = int(vectors.shape[0]), int(vectors.shape[1])
    if init is None:
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed = {seed!r}: an integer")
        if num_lists > B:
            raise ValueError(f"num_lists = {num_lists}: {B} vectors have no {num_lists} distinct rows to start from; pass init")
    elif not isinstance(init, Tensor) or init.dtype != torch.float32 or tuple(init.shape) != (num_lists, D):
        raise ValueError(f"init: an fp32 ({num_lists}, {D}) tensor, not {getattr(init, 'dtype', type(init))} "
                         f"{tuple(getattr(init, 'shape', ()))}")
    if B >= (1 << 31) - 1:
        raise ValueError("vectors: fewer than 2^31 - 1 rows")
    _on_device(vectors, init)
    with torch.no_grad(), torch.cuda.device(vectors.device):
        x = vectors.detach().contiguous()
        if init is None:
            rows = torch.randperm(B, generator=torch.Generator().manual_seed(seed))[:num_lists]
            centroids = x[rows.to(x.device)].float()
        else:
            centroids = init.detach().contiguous().clone()
        for _ in range(iters):
            centroids, _, counts, _ = _step(x, centroids, None, None, B, num_lists, D)
            centroids = _reseed(centroids, counts)
    return centroids
