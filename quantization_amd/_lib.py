"""ctypes binding of libmcq_hip.so (C ABI: include/mcq.h and its companions include/mcq_residual.h, include/mcq_probe.h, include/mcq_wide.h, include/mcq_rerank.h, include/mcq_code16.h and include/mcq_shortlist.h).

The library is built in-tree by `__graft_entry__.build()` (hipcc, gfx950).  There
is no CPU fallback: a missing library or a non-HIP tensor is an error.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# Another build of the same library for same-box A/B timing of kernel variants (tools/ab_lib.sh): honoured only when the process
# opts in with MCQ_ALLOW_LIB_PATH=1 beside MCQ_LIB_PATH, so that a deployed process never loads a library an inherited
# environment variable names.
_ALT = os.environ.get("MCQ_LIB_PATH") if os.environ.get("MCQ_ALLOW_LIB_PATH") == "1" else None
LIB_PATH = _ALT or os.path.join(_HERE, "lib", "libmcq_hip.so")

# The C ABI, one line per function of include/mcq.h in the header's order: name -> (return type, argument types), written as
# _sig("return", "arguments") with one letter per type.  tests/test_abi_signatures_host.py parses the header and compares.
_C = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "d": ctypes.c_double,
      "z": ctypes.c_size_t, "u": ctypes.c_uint, "s": ctypes.c_char_p,
      "F": ctypes.POINTER(ctypes.c_float), "I": ctypes.POINTER(ctypes.c_int)}      # (typed pointers: mcq_profile_encode's outputs)


def _sig(ret, args=""):
    return _C[ret], tuple(_C[c] for c in args)


SIGNATURES = {
    "mcq_abi_version": _sig("i"),
    "mcq_padded_dim": _sig("i", "i"),
    "mcq_prepared_bytes": _sig("z", "iii"),
    "mcq_prepared_decode_bytes": _sig("z", "iii"),
    "mcq_prepared_mean_offset": _sig("z", "iii"),
    "mcq_prepare": _sig("i", "pfppiiipp"),
    "mcq_prepare_dev": _sig("i", "ppppiiipp"),
    "mcq_prepare_params": _sig("i", "pppfppiiippp"),
    "mcq_encode_workspace_bytes": _sig("z", "liii"),
    "mcq_encode": _sig("i", "plpfiiiipppzp"),
    "mcq_encode_ex": _sig("i", "plpfiiiipppzpu"),
    "mcq_refine_indexes": _sig("i", "plpiiiipppzp"),
    "mcq_decode": _sig("i", "piilpiiipp"),
    "mcq_decode_backward": _sig("i", "ppliiipp"),
    "mcq_logits_argmax": _sig("i", "plpfiiipppzpu"),
    "mcq_logits_refine": _sig("i", "plpfiiiipppzpu"),
    "mcq_logits_refine_codes": _sig("i", "plpfiiiippppzpu"),
    "mcq_loss_workspace_bytes": _sig("z", "lii"),
    "mcq_loss_fwd": _sig("i", "ppliipppppzp"),
    "mcq_loss_bwd": _sig("i", "pppliipppp"),
    "mcq_loss_tail": _sig("i", "pppiifpppp"),
    "mcq_recon_fwd": _sig("i", "pplppiiipppp"),
    "mcq_weight_grad_workspace_bytes": _sig("z", "lii"),
    "mcq_weight_grad": _sig("i", "ppliippppzp"),
    "mcq_adam_step": _sig("i", "ppppldddddddp"),
    "mcq_loss_head": _sig("i", "pplpifpp"),
    "mcq_scales_exp": _sig("i", "ppfpp"),
    "mcq_loss_head_tail": _sig("i", "pplpifpppifpppp"),
    "mcq_decode_backward_waves": _sig("l", "iii"),
    "mcq_decode_backward_u8_ex": _sig("i", "ppliiipppfppp"),
    "mcq_loss_bwd_waves": _sig("l", "lii"),
    "mcq_loss_bwd_ex": _sig("i", "pppliipppppp"),
    "mcq_grad_tail": _sig("i", "plppfplfppp"),
    "mcq_jcl_prefix_fwd": _sig("i", "pppliiifpp"),
    "mcq_jcl_prefix_bwd": _sig("i", "ppliifppp"),
    "mcq_scatter_rows": _sig("i", "pllpiliiipp"),
    "mcq_decode_backward_u8": _sig("i", "ppliiipp"),
    "mcq_search_tables": _sig("i", "pilpiiipp"),
    "mcq_code_norms": _sig("i", "plpiiipp"),
    "mcq_search_workspace_bytes": _sig("z", "lliii"),
    "mcq_search_scan": _sig("i", "plppliiipppzp"),
    "mcq_search_scan_metric": _sig("i", "plppliiiipppzp"),
    "mcq_code_rnorms": _sig("i", "plpiiipp"),
    "mcq_rnorms_from_norms": _sig("i", "plpp"),
    "mcq_search_range_workspace_bytes": _sig("z", "llii"),
    "mcq_search_range_count": _sig("i", "plppliiipppzp"),
    "mcq_search_range_fill": _sig("i", "plppliiipppplpzp"),
    "mcq_search_pack_mask": _sig("i", "plpp"),
    "mcq_search_scan_masked": _sig("i", "plppliiiippppzp"),
    "mcq_search_range_count_masked": _sig("i", "plppliiippppzp"),
    "mcq_search_range_fill_masked": _sig("i", "plppliiippppplpzp"),
    "mcq_search_lists_workspace_bytes": _sig("z", "liiii"),
    "mcq_search_scan_lists": _sig("i", "plppliiiipplpipppzp"),
    "mcq_search_range_lists_workspace_bytes": _sig("z", "liii"),
    "mcq_search_range_lists_count": _sig("i", "plppliiipplpipppzp"),
    "mcq_search_range_lists_fill": _sig("i", "plppliiipplpipppplpzp"),
    "mcq_logits_workspace_bytes": _sig("z", "lii"),
    "mcq_logits": _sig("i", "plpfiiippzp"),
    "mcq_test_prepared_layout": _sig("i", "iiipi"),
    "mcq_test_xc": _sig("i", "plpiiippzpu"),
    "mcq_test_select": _sig("i", "piiippp"),
    "mcq_last_encode_launches": _sig("i"),
    "mcq_profile_encode": _sig("i", "plpfiiiipzpFIi"),
    "mcq_profile_category_name": _sig("s", "i"),
}
SYMBOLS = tuple(SIGNATURES)     # every symbol include/mcq.h declares

# include/mcq_residual.h, the companion header of the search over residual codes, in the same form and in its order
# (tests/test_search_bias_host.py parses that header and compares)
RESIDUAL_SIGNATURES = {
    "mcq_search_scan_lists_bias": _sig("i", "plppliiiipplpippppzp"),
    "mcq_search_range_lists_bias_count": _sig("i", "plppliiipplpippppzp"),
    "mcq_search_range_lists_bias_fill": _sig("i", "plppliiipplpippppplpzp"),
    "mcq_code_norms_based": _sig("i", "plpiiiplppp"),
    "mcq_code_rnorms_based": _sig("i", "plpiiiplppp"),
}
RESIDUAL_SYMBOLS = tuple(RESIDUAL_SIGNATURES)

# include/mcq_probe.h, the companion header of the probes the tests run single steps of the encode through, in the same form
# (tests/test_er_probe_host.py, tests/test_pass_lists_host.py and tests/test_pass16_lists_host.py parse that header and compare)
PROBE_SIGNATURES = {
    "mcq_test_er_workspace_bytes": _sig("z", "li"),
    "mcq_test_er": _sig("i", "piiippplppipppzp"),
    "mcq_test_xc_xx": _sig("i", "plpiiipppzpu"),
    "mcq_test_pass_layout": _sig("i", "liiipi"),
    "mcq_test_pass": _sig("i", "plpiiippppupzp"),
    "mcq_test_pass16_layout": _sig("i", "ipi"),
    "mcq_test_pass16": _sig("i", "plpiiipppzipzp"),
}
PROBE_SYMBOLS = tuple(PROBE_SIGNATURES)

# include/mcq_wide.h, the companion header of the top-k search past 64 neighbours, in the same form and in its order
# (tests/test_search_wide_host.py parses that header and compares)
WIDE_SIGNATURES = {
    "mcq_search_wide_workspace_bytes": _sig("z", "lliii"),
    "mcq_search_wide": _sig("i", "plppliiiippppzp"),
    "mcq_search_wide_lists_workspace_bytes": _sig("z", "liiii"),
    "mcq_search_wide_lists": _sig("i", "plppliiiipplpippppzp"),
}
WIDE_SYMBOLS = tuple(WIDE_SIGNATURES)

# include/mcq_rerank.h, the companion header of the exact re-ranking of a shortlist, in the same form and in its order
# (tests/test_rerank_host.py parses that header and compares)
RERANK_SIGNATURES = {
    "mcq_rerank_workspace_bytes": _sig("z", "llii"),
    "mcq_rerank": _sig("i", "pilpiliplpliipppzp"),
}
RERANK_SYMBOLS = tuple(RERANK_SIGNATURES)

# include/mcq_code16.h, the companion header of the search over stores of two-byte codes, in the same form and in its order
# (tests/test_search_code16_host.py parses that header and compares)
CODE16_SIGNATURES = {
    "mcq_search_tables_u16": _sig("i", "pilpiiipp"),
    "mcq_code_norms_u16": _sig("i", "plpiiiiplppp"),
    "mcq_search_topk_u16_workspace_bytes": _sig("z", "liiii"),
    "mcq_search_topk_u16": _sig("i", "plppliiiipplpippppzp"),
    "mcq_search_range_u16_workspace_bytes": _sig("z", "liii"),
    "mcq_search_range_u16_count": _sig("i", "plppliiipplpippppzp"),
    "mcq_search_range_u16_fill": _sig("i", "plppliiipplpippppplpzp"),
}
CODE16_SYMBOLS = tuple(CODE16_SIGNATURES)

# include/mcq_shortlist.h, the companion header of the search over a shortlist, in the same form and in its order
# (tests/test_search_shortlist_host.py parses that header and compares)
SHORTLIST_SIGNATURES = {
    "mcq_search_shortlist_workspace_bytes": _sig("z", "lliii"),
    "mcq_search_shortlist": _sig("i", "plppliiiiplplppppzp"),
    "mcq_search_shortlist_u16": _sig("i", "plppliiiiplplppppzp"),
}
SHORTLIST_SYMBOLS = tuple(SHORTLIST_SIGNATURES)

MCQ_EINVAL, MCQ_EUNSUPPORTED, MCQ_EWORKSPACE = -1, -2, -3
MCQ_SEARCH_L2, MCQ_SEARCH_IP, MCQ_SEARCH_COS = 0, 1, 2     # mcq_search_scan_metric
MCQ_ENCODE_ALL_PASSES = 8       # mcq_encode_ex: every pass on every vector (fixed-point skipping is the default)
MCQ_ENCODE_EXACT_LOGITS = 16    # mcq_encode_ex: the initial arg max from all ten limb products (the screened path is the default)
_lib = None


class McqError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise McqError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950); quantization_amd has no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in {**SIGNATURES, **RESIDUAL_SIGNATURES, **PROBE_SIGNATURES, **WIDE_SIGNATURES,
                                      **RERANK_SIGNATURES, **CODE16_SIGNATURES, **SHORTLIST_SIGNATURES}.items():
        # an older build loaded through the A/B hook above may lack a symbol: it stays unbound, and calling it raises.
        # Without the hook a missing symbol fails here, at load
        if _ALT and not hasattr(L, name):
            continue
        f = getattr(L, name)
        f.restype, f.argtypes = restype, list(argtypes)
    assert L.mcq_abi_version() == 7
    _lib = L
    return L


def check(rc: int, what: str):
    if rc == 0:
        return
    names = {MCQ_EINVAL: "invalid argument", MCQ_EUNSUPPORTED: "unsupported (codebook_size, num_codebooks)",
             MCQ_EWORKSPACE: "workspace too small"}
    raise McqError(f"{what}: {names.get(rc, 'HIP error %d' % rc)}")
