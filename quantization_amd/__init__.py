"""quantization_amd -- MI355X-native multi-codebook vector quantizer.

Drop-in for the hot path of danpovey/quantization (`Quantizer.encode/decode`,
`QuantizerTrainer.step`): same class names, arguments and state-dict layout as
/root/reference/quantization/__init__.py:1-2 exports for this path.
"""
from .quantizer import Quantizer  # noqa: F401
from .trainer import QuantizerTrainer  # noqa: F401
from .prediction import JointCodebookLoss  # noqa: F401   (the consumer of the codes, quantization/__init__.py:4)
from .hdf5_data import read_hdf5_data  # noqa: F401      (the data helper, quantization/__init__.py:3)
from .ivf import build_lists, probe_lists, probe_bias, list_assign  # noqa: F401   (an inverted file over a store of codes: Quantizer.search_lists, range_search_lists)
from .rerank import rerank  # noqa: F401   (the exact re-ranking of a shortlist: the step after search_wide / search_lists_wide)
from .coarse import coarse_terms, coarse_probe, coarse_assign  # noqa: F401   (the coarse quantizer in HIP: probes, biases, assignment)
from .kmeans import kmeans_step, coarse_train  # noqa: F401   (the coarse centroids themselves: a Lloyd step and the trainer, in HIP)
from .half import coarse_assign_half, kmeans_step_half, coarse_train_half  # noqa: F401   (the same over an fp16 raw store, on the f16 matrix cores)
from .half import coarse_planes, coarse_probe_half  # noqa: F401   (the coarse probes for fp16 queries, on the same matrix cores)
from .bf16 import coarse_assign_bf16, kmeans_step_bf16, coarse_train_bf16  # noqa: F401   (the Lloyd step and the trainer over a bf16 raw store, on the bf16 matrix cores)
from .split import coarse_assign_split, kmeans_step_split, coarse_train_split  # noqa: F401   (the same for fp32 rows on the bf16 matrix cores: six products of bf16 planes)
from .split import coarse_planes_split, coarse_probe_split  # noqa: F401   (the coarse probes for fp32 queries on those six products, a heap per query)

__all__ = ["Quantizer", "QuantizerTrainer", "JointCodebookLoss", "read_hdf5_data", "build_lists", "probe_lists", "probe_bias", "list_assign", "rerank",
           "coarse_terms", "coarse_probe", "coarse_assign", "kmeans_step", "coarse_train",
           "coarse_assign_half", "kmeans_step_half", "coarse_train_half", "coarse_planes", "coarse_probe_half",
           "coarse_assign_bf16", "kmeans_step_bf16", "coarse_train_bf16",
           "coarse_assign_split", "kmeans_step_split", "coarse_train_split", "coarse_planes_split", "coarse_probe_split"]
