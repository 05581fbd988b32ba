"""The coarse centroids of an inverted file over a bf16 raw store (include/mcq_bf16.h rules 56-59): coarse_assign, kmeans_step
and coarse_train of quantization_amd/coarse.py and kmeans.py for torch.bfloat16 vectors, with no fp32 copy of the store and
nothing of size (B, L).  The centroids stay fp32 -- they are means -- and are split once per call into three bf16 planes (hi,
mid and lo, unscaled: bf16 has fp32's exponent) that the vectors meet on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, one
fp32 accumulator a pair); the update widens every bf16 element exactly into the float64 tree of rule 47, so
kmeans_step_bf16(x, c)'s new centroids and counts are kmeans_step(x.float(), c)'s bit for bit wherever the two assignments
agree.

    centroids = coarse_train_bf16(store_bf16, 1024, iters=10, seed=0)  # (1024, D) fp32
    terms = coarse_terms(centroids)
    assign = coarse_assign_bf16(store_bf16, centroids, terms=terms)    # and on to build_lists

"l2" only; there is no CPU path, and nothing is read back to the host.  The coarse probes for bf16 queries and rerank over
bf16 rows are not built."""
import torch
from torch import Tensor

from .coarse import coarse_terms
from .kmeans import _assign, _checked_step, _public_step, _train
from .search import _on_device

__all__ = ["coarse_assign_bf16", "kmeans_step_bf16", "coarse_train_bf16"]


def coarse_assign_bf16(vectors: Tensor, centroids: Tensor, terms: Tensor = None) -> Tensor:
    """vectors (B, D) bf16, centroids (L, D) fp32, L >= 1, on the device -> int32 (B,): the nearest centroid of each vector
    under "l2" by the score of include/mcq_bf16.h rule 57, the lower list among equals, -1 for a row whose every score is NaN.
    It allocates its output, the part buffers (8 bytes per vector and part) and the three bf16 planes of the centroids; no fp32
    copy of the vectors and nothing of size (B, L).  terms: what coarse_terms(centroids) returned (computed here if None).
    fp32 vectors are a ValueError that names coarse_assign, fp16 vectors one that names coarse_assign_half; no CPU fallback
    (McqError)."""
    B, L, D = _checked_step(vectors, centroids, terms, None, torch.bfloat16, "coarse_assign")
    _on_device(vectors, centroids, terms)
    with torch.no_grad(), torch.cuda.device(vectors.device):
        c = centroids.detach().contiguous()
        return _assign(vectors.detach().contiguous(), c, coarse_terms(c) if terms is None else terms, None, B, L, D)[0]


def kmeans_step_bf16(vectors: Tensor, centroids: Tensor, terms: Tensor = None, prev_assign: Tensor = None):
    """vectors (B, D) bf16, centroids (L, D) fp32, L >= 1, on the device -> (new_centroids (L, D) fp32, assign int32 (B,),
    counts int32 (L,), changed): kmeans_step for a bf16 store.  assign is coarse_assign_bf16(vectors, centroids);
    new_centroids[l] is the mean of list l's rows, each bf16 element widened exactly, over the fixed float64 tree of
    include/mcq_kmeans.h rule 47, rounded once; a list without rows keeps its centroid and counts 0.  changed is a device tensor
    of one int32, the number of rows whose assignment differs from prev_assign, or None without one.
    Not differentiable; fp32 vectors are a ValueError that names kmeans_step, fp16 vectors one that names kmeans_step_half; no
    CPU fallback (McqError); shape and dtype errors are ValueErrors raised before any device work; nothing is read back to the
    host."""
    return _public_step(vectors, centroids, terms, prev_assign, torch.bfloat16, "kmeans_step")


def coarse_train_bf16(vectors: Tensor, num_lists: int, iters: int = 10, seed: int = 0, init: Tensor = None) -> Tensor:
    """vectors (B, D) bf16 on the device -> centroids (num_lists, D) fp32: coarse_train for a bf16 store: `iters` steps
    (kmeans_step_bf16) from `init` -- (num_lists, D) fp32 rows -- or, without one, from num_lists distinct rows of `vectors`,
    widened to fp32, drawn by a torch.Generator seeded with `seed`.  After each step an empty list is reseeded from the largest
    as in coarse_train.  The same vectors, seed or init, and iters give the same bits on every run.  fp32 vectors are a
    ValueError that names coarse_train, fp16 vectors one that names coarse_train_half; argument errors are ValueErrors raised
    before any device work; no CPU fallback."""
    return _train(vectors, num_lists, iters, seed, init, torch.bfloat16, "coarse_train")
