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

"l2" only; there is no CPU path, and nothing is read back to the host.  The coarse probes for fp32 queries split into planes
are not built."""
import torch
from torch import Tensor

from .coarse import coarse_terms
from .kmeans import PLANES6, _assign, _checked_step, _public_step, _train
from .search import _on_device

__all__ = ["coarse_assign_split", "kmeans_step_split", "coarse_train_split"]


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
