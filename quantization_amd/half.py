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

from .coarse import coarse_terms
from .kmeans import _assign, _checked_step, _public_step, _train
from .search import _on_device

__all__ = ["coarse_assign_half", "kmeans_step_half", "coarse_train_half"]


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
