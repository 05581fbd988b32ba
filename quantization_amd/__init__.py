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

__all__ = ["Quantizer", "QuantizerTrainer", "JointCodebookLoss", "read_hdf5_data", "build_lists", "probe_lists", "probe_bias", "list_assign", "rerank"]
