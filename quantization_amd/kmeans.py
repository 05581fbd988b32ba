"""The coarse centroids of an inverted file, trained in HIP (include/mcq_kmeans.h rules 44-47): one Lloyd step is
mcq_kmeans_assign -- the nearest centroid of every training vector on the fp32 matrix cores, the bits of coarse_assign, with
nothing of size (B, L) -- then a stable sort by list in torch, then mcq_kmeans_update -- the members' mean per list as a float64
sum over a fixed tree, gathered through `order` from the vectors where they lie.  No floating-point atomics: the centroids are a
stated function of the vectors, the start and the number of steps, the same bits on every run.

    centroids = coarse_train(sample, 1024, iters=10, seed=0)          # (1024, D) fp32
    terms = coarse_terms(centroids)
    assign = coarse_assign(x, centroids, terms=terms)                 # and on to build_lists, coarse_probe, search_lists

    new, assign, counts, changed = kmeans_step(sample, centroids)     # a single step, for a loop of one's own

"l2" only; there is no CPU path, and nothing is read back to the host."""
import torch
from torch import Tensor

from .coarse import MAX_DIM, _checked, coarse_terms
from .search import _call, _entry, _on_device

__all__ = ["kmeans_step", "coarse_train"]
SPLIT = 1e-4                # faiss's split of the largest list when another is empty


# the dtype of the vector rows picks the entries (the parts query, the assignment, the update, and the size query of the planes
# the centroids are split into, where they are); PLANES6 picks those of include/mcq_split.h, which take fp32 rows too
PLANES6 = "split"
_ENTRIES = {torch.float32: ("mcq_kmeans_parts", "mcq_kmeans_assign", "mcq_kmeans_update", None),
            torch.float16: ("mcq_kmeans_half_parts", "mcq_kmeans_assign_half", "mcq_kmeans_update_half", "mcq_kmeans_half_planes"),
            torch.bfloat16: ("mcq_kmeans_bf16_parts", "mcq_kmeans_assign_bf16", "mcq_kmeans_update_bf16", "mcq_kmeans_bf16_planes"),
            PLANES6: ("mcq_kmeans_split_parts", "mcq_kmeans_assign_split", "mcq_kmeans_update", "mcq_kmeans_split_planes")}
_NAME = {torch.float32: "fp32", torch.float16: "fp16", torch.bfloat16: "bf16"}
# the rows a call sends on by name, and the suffix of the public call that takes them
_SENT_ON = {torch.float16: {torch.float32: ""}, torch.bfloat16: {torch.float32: "", torch.float16: "_half"},
            PLANES6: {torch.float16: "_half", torch.bfloat16: "_bf16"}}


def _elsewhere(vectors, dtype, name):
    """rows of a type that another call serves: a ValueError that names that call.  name: the fp32 call's name"""
    if isinstance(vectors, Tensor) and vectors.dtype in _SENT_ON[dtype]:
        raise ValueError(f"vectors: {_NAME[vectors.dtype]} rows go to {name}{_SENT_ON[dtype][vectors.dtype]}; this call takes "
                         f"{torch.float32 if dtype == PLANES6 else dtype}")


def _checked_step(vectors, centroids, terms, prev_assign, dtype=torch.float32, fp32_name=None):
    """shape and dtype errors of a step over rows of `dtype` (PLANES6: fp32 rows for the entries of include/mcq_split.h): looks
    at no data, so it runs before any device work, on CPU tensors too.  fp32_name: the call that fp32 rows are sent to by a
    call that takes 16-bit rows, or the one whose suffixed forms take the 16-bit rows that PLANES6 sends on"""
    if dtype == PLANES6:
        _elsewhere(vectors, dtype, fp32_name)
    if dtype in (torch.float32, PLANES6):
        L, D = _checked(vectors, centroids, "l2", terms, "vectors")
        if vectors.ndim != 2:
            raise ValueError(f"vectors: an fp32 (B, {D}) tensor, not {tuple(vectors.shape)}")
    else:
        L, D = _checked(None, centroids, "l2", terms, "")
        _elsewhere(vectors, dtype, fp32_name)
        if not isinstance(vectors, Tensor) or vectors.dtype != dtype or vectors.ndim != 2 or vectors.shape[1] != D:
            raise ValueError(f"vectors: an {_NAME[dtype]} (B, {D}) tensor, not {getattr(vectors, 'dtype', type(vectors))} "
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


def _assign(x, c, terms, prev, B, L, D, key=None):
    """x (B, D) fp32, fp16 or bf16 and c (L, D) fp32 contiguous on one device: the assignment entry of x.dtype, or of `key`
    (PLANES6, fp32 rows) where one is given, its outputs and its scratch -> (assign, changed)"""
    dev = x.device
    parts_query, entry, _, planes_query = _ENTRIES[key or x.dtype]
    parts = int(_entry(parts_query)(B, L, D))
    assign = torch.empty((B,), dtype=torch.int32, device=dev)
    score = torch.empty((B,), dtype=torch.float32, device=dev)
    changed = None if prev is None else torch.empty((1,), dtype=torch.int32, device=dev)
    part_score = torch.empty((B, parts), dtype=torch.float32, device=dev)
    part_list = torch.empty((B, parts), dtype=torch.int32, device=dev)
    scratch = [part_score.data_ptr(), part_list.data_ptr()]
    if planes_query is not None:                             # the 16-bit planes of the centroids: two of fp16, three of bf16
                                                             # (for bf16 rows and for PLANES6)
        planes = torch.empty((int(_entry(planes_query)(L, D)),), dtype=torch.int16, device=dev)
        scratch.append(planes.data_ptr())
    _call(entry, x.data_ptr(), B, c.data_ptr(), L, D, terms.data_ptr(), parts, None if prev is None else prev.data_ptr(),
          assign.data_ptr(), score.data_ptr(), None if changed is None else changed.data_ptr(), *scratch,
          torch.cuda.current_stream(dev).cuda_stream)
    return assign, changed


def _step(x, c, terms, prev, B, L, D, entries=None):
    """x (B, D) fp32, fp16 or bf16 and c (L, D) fp32 contiguous on one device: the two entries of x.dtype, or of `entries`
    (_assign's `key`), and the sort between them"""
    dev = x.device
    if terms is None:
        terms = coarse_terms(c)
    assign, changed = _assign(x, c, terms, prev, B, L, D, entries)
    # the stable sort by list: ascending original position inside a list; a row assigned -1 sorts behind list L - 1
    key = torch.where(assign < 0, torch.full_like(assign, L), assign).to(torch.int64)
    keys, order = torch.sort(key, stable=True)
    offsets = torch.searchsorted(keys, torch.arange(L + 1, dtype=torch.int64, device=dev))
    new = torch.empty_like(c)
    counts = torch.empty((L,), dtype=torch.int32, device=dev)
    block_first = torch.empty((L + 1,), dtype=torch.int64, device=dev)
    block_sums = torch.empty((int(_entry("mcq_kmeans_blocks")(B, L, D)),), dtype=torch.float64, device=dev)
    _call(_ENTRIES[entries or x.dtype][2], x.data_ptr(), B, D, order.data_ptr(), offsets.data_ptr(), L, c.data_ptr(), new.data_ptr(),
          counts.data_ptr(), block_first.data_ptr(), block_sums.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    return new, assign, counts, changed


def _public_step(vectors, centroids, terms, prev_assign, dtype, fp32_name):
    """kmeans_step, kmeans_step_half, kmeans_step_bf16 and kmeans_step_split (dtype PLANES6): the checks, then _step on
    contiguous tensors"""
    B, L, D = _checked_step(vectors, centroids, terms, prev_assign, dtype, fp32_name)
    _on_device(vectors, centroids, terms, prev_assign)
    with torch.no_grad(), torch.cuda.device(vectors.device):
        return _step(vectors.detach().contiguous(), centroids.detach().contiguous(), terms,
                     None if prev_assign is None else prev_assign.detach().contiguous(), B, L, D,
                     PLANES6 if dtype == PLANES6 else None)


def kmeans_step(vectors: Tensor, centroids: Tensor, terms: Tensor = None, prev_assign: Tensor = None):
    """vectors (B, D) fp32, centroids (L, D) fp32, L >= 1, on the device -> (new_centroids (L, D) fp32, assign int32 (B,),
    counts int32 (L,), changed): one Lloyd step under "l2".  assign is coarse_assign(vectors, centroids), ties to the lower
    list, -1 for a row whose every score is NaN (it belongs to no list); new_centroids[l] is the mean of list l's rows, a
    float64 sum in ascending row order over the fixed tree of include/mcq_kmeans.h rule 47, rounded once; a list without rows
    keeps its centroid and counts 0.  changed is a device tensor of one int32, the number of rows whose assignment differs from
    prev_assign (what an earlier step returned), or None without prev_assign.
    terms: what coarse_terms(centroids) returned (computed here if None).  Not differentiable; no CPU fallback (McqError);
    shape and dtype errors are ValueErrors raised before any device work; nothing is read back to the host."""
    return _public_step(vectors, centroids, terms, prev_assign, torch.float32, None)


def _reseed(centroids, counts):
    """empty lists take a share of the largest ones: the j-th empty list, by index, becomes the centroid of the j-th largest
    list (stable descending counts) times 1 + SPLIT, and that donor's own centroid is scaled by 1 - SPLIT.  Over L rows, on
    the device, without a host read; no list empty: every row keeps its bits"""
    L = counts.shape[0]
    empty = counts == 0
    donors = torch.sort(counts, descending=True, stable=True).indices
    rank = torch.cumsum(empty, 0) - 1                        # j of an empty list
    source = torch.where(empty, donors[rank.clamp(min=0)], torch.arange(L, device=counts.device))
    gives = torch.empty_like(empty)
    gives[donors] = torch.arange(L, device=counts.device) < empty.sum()
    one = torch.ones((), dtype=torch.float32, device=counts.device)
    scale = torch.where(empty, one * (1 + SPLIT), torch.where(gives, one * (1 - SPLIT), one))
    return centroids[source] * scale[:, None]


def _train(vectors, num_lists, iters, seed, init, dtype, fp32_name):
    """coarse_train, coarse_train_half, coarse_train_bf16 and coarse_train_split (dtype PLANES6): the argument errors, the start
    and `iters` times _step and _reseed"""
    key, dtype = (PLANES6, torch.float32) if dtype == PLANES6 else (None, dtype)
    if isinstance(num_lists, bool) or not isinstance(num_lists, int) or num_lists < 1:
        raise ValueError(f"num_lists = {num_lists!r}: a positive integer")
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"iters = {iters!r}: a non-negative integer")
    if key or dtype != torch.float32:
        _elsewhere(vectors, key or dtype, fp32_name)
    if not isinstance(vectors, Tensor) or vectors.ndim != 2 or vectors.dtype != dtype or not 1 <= vectors.shape[1] <= MAX_DIM:
        raise ValueError(f"vectors: an {_NAME[dtype]} (B, D) tensor, 1 <= D <= {MAX_DIM}, not "
                         f"{getattr(vectors, 'dtype', type(vectors))} {tuple(getattr(vectors, 'shape', ()))}")
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
            centroids = x[rows.to(x.device)].float()         # (fp32 rows: the same tensor, no copy)
        else:
            centroids = init.detach().contiguous().clone()
        for _ in range(iters):
            centroids, _, counts, _ = _step(x, centroids, None, None, B, num_lists, D, key)
            centroids = _reseed(centroids, counts)
    return centroids


def coarse_train(vectors: Tensor, num_lists: int, iters: int = 10, seed: int = 0, init: Tensor = None) -> Tensor:
    """vectors (B, D) fp32 on the device -> centroids (num_lists, D) fp32: `iters` Lloyd steps (kmeans_step) under "l2" from
    `init` -- (num_lists, D) fp32 rows -- or, without one, from num_lists distinct rows of `vectors` drawn by a
    torch.Generator seeded with `seed`.  After each step an empty list is reseeded from the largest (faiss's split, _reseed).
    The same vectors, seed or init, and iters give the same bits on every run.  Argument errors are ValueErrors raised before
    any device work; no CPU fallback (McqError); nothing is read back to the host."""
    return _train(vectors, num_lists, iters, seed, init, torch.float32, None)


