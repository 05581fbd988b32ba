"""Host-side checks of the encode flags (no GPU): fixed-point skipping is the default, MCQ_ENCODE_ALL_PASSES turns it off,
and the ABI version did not move."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "mcq.h")) as f:
        return f.read()


def test_header_defines_all_passes_flag_and_abi_7():
    hdr = _header()
    flags = dict(re.findall(r"#define\s+(MCQ_ENCODE_[A-Z0-9_]+)\s+(\d+)u", hdr))
    assert flags.get("MCQ_ENCODE_ALL_PASSES") == "8"
    assert flags.get("MCQ_ENCODE_SKIP_FIXED_POINTS") == "1"          # still accepted
    assert len(set(flags.values())) == len(flags)                      # distinct bits
    assert re.search(r"#define\s+MCQ_ABI_VERSION\s+7\b", hdr)


def test_python_binding_and_quantizer_default():
    from quantization_amd import _lib
    from quantization_amd import Quantizer
    assert _lib.MCQ_ENCODE_ALL_PASSES == 8
    assert Quantizer(16, 16, 2).skip_fixed_points is True
