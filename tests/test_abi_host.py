"""Host-side checks that need no GPU: the C-ABI library loads and exports every
symbol of include/mcq.h; size queries; argument validation that precedes any launch."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    import __graft_entry__ as g
    g.build()
    from quantization_amd import _lib
    return _lib


def test_header_symbols_are_exported():
    _lib_mod = _lib()
    L = _lib_mod.lib()
    hdr = open(os.path.join(ROOT, "include", "mcq.h")).read()
    declared = set(re.findall(r"\b(mcq_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib_mod.SYMBOLS), declared ^ set(_lib_mod.SYMBOLS)
    for s in declared:
        assert hasattr(L, s), s
    assert L.mcq_abi_version() == 7


def test_size_queries():
    L = _lib().lib()
    assert L.mcq_padded_dim(512) == 512 and L.mcq_padded_dim(40) == 48 and L.mcq_padded_dim(1) == 16
    # scaled centers + sumsq + padded weight + bias
    assert L.mcq_prepared_bytes(8, 256, 512) >= 2 * 8 * 256 * 512 * 4 + 2 * 8 * 256 * 4
    a = L.mcq_encode_workspace_bytes(1000, 8, 256, 512)
    b = L.mcq_encode_workspace_bytes(65536, 8, 256, 512)
    c = L.mcq_encode_workspace_bytes(10 ** 7, 8, 256, 512)
    assert a < b and b == c          # the batch is chunked: the workspace stops growing


def test_argument_validation_without_launch():
    m = _lib()
    L = m.lib()
    # unsupported domain and bad arguments are rejected before anything touches the device
    assert L.mcq_encode(None, 4, None, 1.0, 8, 8, 64, 1, None, None, None, 0, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_encode(None, 4, None, 1.0, 8, 2048, 64, 1, None, None, None, 0, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_encode(None, 4, None, 1.0, 32, 1024, 64, 1, None, None, None, 0, None) == m.MCQ_EUNSUPPORTED    # Gram matrix past 16,384 rows
    assert L.mcq_encode(None, 4, None, 1.0, 8, 512, 64, 1, None, None, None, 0, None) == m.MCQ_EINVAL            # supported shape, no output array
    assert L.mcq_encode(None, 4, None, 1.0, 3, 256, 64, 1, None, None, None, 0, None) == m.MCQ_EINVAL
    assert L.mcq_encode(None, -1, None, 1.0, 8, 256, 64, 1, None, None, None, 0, None) == m.MCQ_EINVAL
    assert L.mcq_decode(None, 2, 8, 4, None, 8, 256, 64, None, None) == m.MCQ_EINVAL
    assert L.mcq_decode(None, 1, 3, 4, None, 8, 256, 64, None, None) == m.MCQ_EINVAL
    assert L.mcq_prepare(None, 1.0, None, None, 8, 256, 64, None, None) == m.MCQ_EINVAL
    # the trainer's entry points stay at K <= 256 (include/mcq.h): wider codebooks are UNSUPPORTED there, not "invalid"
    assert L.mcq_logits_refine(None, 4, None, 1.0, 4, 512, 64, 1, None, None, None, 0, None, 0) == m.MCQ_EUNSUPPORTED
    assert L.mcq_logits_refine_codes(None, 4, None, 1.0, 4, 512, 64, 1, None, None, None, None, 0, None, 0) == m.MCQ_EUNSUPPORTED
    assert L.mcq_decode_backward_u8(None, None, 4, 4, 512, 64, None, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_decode_backward_u8_ex(None, None, 4, 4, 512, 64, None, None, None, 1.0, None, None, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_decode_backward_u8(None, None, 4, 4, 256, 64, None, None) == m.MCQ_EINVAL
    assert L.mcq_loss_fwd(None, None, 4, 4, 512, None, None, None, None, None, 0, None) == m.MCQ_EUNSUPPORTED
    # the loss tail keeps one entropy pair per codebook in shared memory: N > 64 is refused before any pointer is read
    assert L.mcq_loss_tail(None, None, None, 65, 256, 1.0, None, None, None, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_loss_tail(None, None, None, 1 << 20, 16, 1.0, None, None, None, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_loss_tail(None, None, None, 64, 256, 1.0, None, None, None, None) == m.MCQ_EINVAL
    assert L.mcq_loss_head_tail(None, None, 1, None, 65, 1.0, None, None, None, 16, 1.0, None, None, None, None) == m.MCQ_EUNSUPPORTED
    assert L.mcq_loss_head_tail(None, None, 1, None, 64, 1.0, None, None, None, 16, 1.0, None, None, None, None) == m.MCQ_EINVAL
    assert L.mcq_profile_encode(None, 4, None, 1.0, 8, 256, 64, 1, None, 0, None, None, None, 0) == m.MCQ_EINVAL     # no output array


def test_rejections_of_the_decode_logits_trainer_and_encode_entry_points():
    """Return codes that precede any launch, as commit e388410's library gives them.  Null pointers wherever the check under
    test allows; `p` is a host buffer standing in for a pointer that must be non-null to REACH that check (the call returns
    before anything is enqueued)."""
    m = _lib()
    L = m.lib()
    EINVAL, EUNSUP = m.MCQ_EINVAL, m.MCQ_EUNSUPPORTED
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    # mcq_decode(codes, code_bytes, codes_per_row, B, prepared, N, K, D, out, stream)
    assert L.mcq_decode(None, 1, 2, 4, None, 64, 16, 64, None, None) == EINVAL            # rep = 32
    assert L.mcq_decode(None, 1, 8, 4, None, 8, 256, 64, None, None) == EINVAL            # rep = 1, null pointers
    assert L.mcq_decode(None, 2, 8, 0, None, 8, 256, 64, None, None) == EINVAL            # code_bytes 2 (before B == 0)
    assert L.mcq_decode(None, 4, 8, 0, None, 8, 256, 64, None, None) == EINVAL
    assert L.mcq_decode(None, 1, 8, -1, None, 8, 256, 64, None, None) == EINVAL
    assert L.mcq_decode(None, 1, 8, 0, None, 8, 256, 64, None, None) == 0
    assert L.mcq_decode(None, 8, 1, 0, None, 16, 256, 64, None, None) == 0                # rep = 16, int64 codes
    assert L.mcq_decode(None, 1, 8, 4, None, 8, 8, 64, None, None) == EUNSUP              # K below the domain, valid D
    assert L.mcq_decode(None, 1, 8, 4, None, 8, 2048, 64, None, None) == EUNSUP
    assert L.mcq_decode(None, 1, 8, 4, None, 8, 48, 64, None, None) == EINVAL             # K inside the range, no power of two
    assert L.mcq_decode(None, 1, 8, 4, None, 8, 256, 20000, None, None) == EINVAL         # (its domain_err never sees D)
    assert L.mcq_encode(None, 4, None, 1.0, 8, 256, 20000, 1, None, None, None, 0, None) == EUNSUP
    # mcq_logits(x, B, prepared, lscale, N, K, D, out, ws, ws_bytes, stream): UNSUPPORTED for anything outside the domain
    assert L.mcq_logits(None, 4, None, 1.0, 3, 256, 64, None, None, 0, None) == EUNSUP
    assert L.mcq_logits(None, 4, None, 1.0, 8, 8, 64, None, None, 0, None) == EUNSUP
    assert L.mcq_logits(None, 0, None, 1.0, 8, 256, 64, None, None, 0, None) == 0
    assert L.mcq_logits(None, -1, None, 1.0, 8, 256, 64, None, None, 0, None) == EINVAL
    assert L.mcq_logits(None, 4, None, 1.0, 8, 256, 64, None, None, 0, None) == EINVAL
    # mcq_test_xc(x, B, prepared, N, K, D, out, ws, ws_bytes, stream, flags): the checks of mcq_logits in its order, then the flags
    assert L.mcq_test_xc(None, 4, None, 3, 256, 64, None, None, 0, None, 0) == EUNSUP
    assert L.mcq_test_xc(None, 4, None, 8, 8, 64, None, None, 0, None, 0) == EUNSUP
    assert L.mcq_test_xc(None, 0, None, 8, 256, 64, None, None, 0, None, 0) == 0
    assert L.mcq_test_xc(None, -1, None, 8, 256, 64, None, None, 0, None, 0) == EINVAL
    assert L.mcq_test_xc(None, 4, None, 8, 256, 64, None, None, 0, None, 0) == EINVAL
    assert L.mcq_test_xc(p, 4, p, 8, 256, 64, p, None, 1 << 30, None, 0) == EINVAL                      # null workspace
    assert L.mcq_test_xc(p, 4, p, 8, 256, 64, p, p, 1 << 30, None, 2) == EINVAL                         # a flag that is not X_FP16
    assert L.mcq_test_xc(p, 4, p, 8, 256, 64, p, p, 0, None, 4) == m.MCQ_EWORKSPACE
    assert L.mcq_test_xc(p, 4, p, 8, 256, 64, p, p, L.mcq_logits_workspace_bytes(4, 8, 64) - 1, None, 0) == m.MCQ_EWORKSPACE
    # mcq_test_prepared_layout(N, K, D, offsets_out, cap): the domain first (as mcq_prepare), then the pointer
    assert L.mcq_test_prepared_layout(8, 8, 64, None, 13) == EUNSUP
    assert L.mcq_test_prepared_layout(3, 256, 64, None, 13) == EINVAL
    assert L.mcq_test_prepared_layout(8, 256, 64, None, 13) == EINVAL
    assert L.mcq_test_prepared_layout(8, 256, 64, p, -1) == EINVAL
    assert L.mcq_test_prepared_layout(8, 256, 64, p, 0) == 13
    # mcq_logits_argmax(x, B, prepared, lscale, N, K, D, logits_out, argmax_out, ws, ws_bytes, stream, flags)
    assert L.mcq_logits_argmax(None, 4, None, 1.0, 4, 512, 64, None, None, None, 0, None, 0) == EUNSUP
    assert L.mcq_logits_argmax(None, 4, None, 1.0, 3, 256, 64, None, None, None, 0, None, 0) == EUNSUP
    assert L.mcq_logits_argmax(None, -1, None, 1.0, 4, 256, 64, None, None, None, 0, None, 0) == EINVAL
    assert L.mcq_logits_argmax(None, 0, None, 1.0, 4, 256, 64, None, None, None, 0, None, 0) == 0
    assert L.mcq_logits_argmax(None, 4, None, 1.0, 4, 256, 64, None, None, None, 0, None, 0) == EINVAL
    # the loss kernels: K in 16 .. 256, B > 0 (an empty batch is INVALID, not a no-op)
    for K, want in ((8, EUNSUP), (512, EUNSUP), (48, EUNSUP), (256, EINVAL)):
        Bs = (0, -1) if want == EINVAL else (4, 0)
        for Bq in Bs:
            assert L.mcq_loss_fwd(None, None, Bq, 4, K, None, None, None, None, None, 0, None) == want, (K, Bq)
            assert L.mcq_loss_bwd(None, None, None, Bq, 4, K, None, None, None, None) == want, (K, Bq)
            assert L.mcq_loss_bwd_ex(None, None, None, Bq, 4, K, None, None, None, None, None, None) == want, (K, Bq)
            assert L.mcq_recon_fwd(None, None, Bq, None, None, 4, K, 64, None, None, None, None) == want, (K, Bq)
    assert L.mcq_loss_fwd(None, None, 4, 0, 64, None, None, None, None, None, 0, None) == EUNSUP        # N < 1
    assert L.mcq_loss_bwd(None, None, None, 4, 0, 64, None, None, None, None) == EUNSUP
    assert L.mcq_loss_bwd_ex(None, None, None, 4, 0, 64, None, None, None, None, None, None) == EUNSUP
    assert L.mcq_loss_fwd(None, None, 4, 128, 64, None, None, None, None, None, 0, None) == EINVAL      # (no cap on N here)
    assert L.mcq_loss_tail(None, None, None, 0, 64, 1.0, None, None, None, None) == EUNSUP
    assert L.mcq_loss_head_tail(None, None, 1, None, 4, 1.0, None, None, None, 8, 1.0, None, None, None, None) == EUNSUP
    assert L.mcq_loss_bwd(None, None, None, 4, 4, 64, None, None, None, None) == EINVAL                 # null pointers
    assert L.mcq_loss_bwd_ex(p, p, p, 4, 4, 64, p, p, p, None, p, None) == EINVAL                       # null bias
    assert L.mcq_loss_bwd_ex(p, p, p, 4, 4, 64, p, p, p, p, None, None) == EINVAL                       # null dot_part
    assert L.mcq_recon_fwd(None, None, 4, None, None, 3, 64, 64, None, None, None, None) == EUNSUP      # domain_ok, not the K test
    assert L.mcq_recon_fwd(None, None, 4, None, None, 4, 64, 64, None, None, None, None) == EINVAL
    # mcq_weight_grad(G, x, B, M, D, scale_dev, gW, gb, ws, ws_bytes, stream)
    assert L.mcq_weight_grad(p, p, 4, 24, 64, p, p, p, p, 1 << 30, None) == EINVAL                      # M % 16 != 0
    assert L.mcq_weight_grad(None, None, 4, 32, 64, None, None, None, None, 0, None) == EINVAL
    assert L.mcq_weight_grad(p, p, 4, 32, 64, p, p, p, p, 0, None) == m.MCQ_EWORKSPACE
    # mcq_adam_step(p, g, m, v, n, ...)
    assert L.mcq_adam_step(None, None, None, None, -1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None) == EINVAL
    assert L.mcq_adam_step(None, None, None, None, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None) == 0
    assert L.mcq_adam_step(None, None, None, None, 4, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1.0, None) == EINVAL
    # mcq_scatter_rows(grad, stride_b, stride_n, idx, idx_stride, B, N, K, D, out, stream)
    assert L.mcq_scatter_rows(None, 64, 0, None, 7, 0, 8, 256, 64, p, None) == EINVAL                   # idx_stride < N
    # mcq_decode_backward_u8_ex(grad_out, codes, B, N, K, D, gC, sa, sb, sc, dotw, dot_part, stream)
    assert L.mcq_decode_backward_u8_ex(None, None, 0, 8, 256, 64, p, None, None, 1.0, p, None, None) == EINVAL
    assert L.mcq_decode_backward_u8_ex(None, None, 0, 8, 256, 64, p, None, None, 1.0, None, p, None) == EINVAL
    assert L.mcq_decode_backward_u8_ex(None, None, 4, 8, 256, 64, p, None, None, 1.0, None, None, None) == EINVAL
    # mcq_encode(x, B, prepared, lscale, N, K, D, iters, out_u8, out_i64, ws, ws_bytes, stream)
    assert L.mcq_encode(None, 4, None, 1.0, 8, 256, 64, 1, p, p, None, 0, None) == EINVAL               # both outputs
    assert L.mcq_encode(None, 4, None, 1.0, 8, 256, 64, 61, p, None, None, 0, None) == EINVAL
    assert L.mcq_encode(None, 4, None, 1.0, 8, 256, 64, -1, p, None, None, 0, None) == EINVAL
    # an empty batch is a no-op once exactly one output is named; with NO output the output check comes first
    assert L.mcq_encode(None, 0, None, 1.0, 8, 256, 64, 1, p, None, None, 0, None) == 0
    assert L.mcq_encode(None, 0, None, 1.0, 8, 256, 64, 1, None, None, None, 0, None) == EINVAL
    assert L.mcq_last_encode_launches() == 0
    assert L.mcq_encode(None, 4, None, 1.0, 4, 512, 64, 1, p, None, None, 0, None) == EINVAL            # two-byte entries, byte output
    assert L.mcq_encode(None, 0, None, 1.0, 4, 512, 64, 1, None, p, None, 0, None) == 0
    assert L.mcq_encode(None, 4, None, 1.0, 8, 256, 64, 1, p, None, None, 0, None) == EINVAL            # null x / prepared / workspace
    assert L.mcq_encode(p, 4, p, 1.0, 8, 256, 64, 1, p, None, p, 0, None) == m.MCQ_EWORKSPACE
    assert L.mcq_encode_ex(None, 4, None, 1.0, 8, 256, 64, 61, p, None, None, 0, None, 0) == EINVAL
    # mcq_refine_indexes(x, B, prepared, N, K, D, iters, idx_in, idx_out, ws, ws_bytes, stream)
    assert L.mcq_refine_indexes(None, 4, None, 8, 256, 64, 1, None, p, None, 0, None) == EINVAL
    assert L.mcq_refine_indexes(None, 0, None, 8, 256, 64, 1, None, p, None, 0, None) == 0
    assert L.mcq_refine_indexes(None, 4, None, 8, 8, 64, 1, None, None, None, 0, None) == EINVAL        # (the pointers come first)
    # mcq_logits_refine_codes(x, B, prepared, lscale, N, K, D, iters, logits_out, idx_out, codes_out, ws, ws_bytes, stream, flags)
    assert L.mcq_logits_refine_codes(None, 4, None, 1.0, 4, 256, 64, 1, None, p, None, None, 0, None, 0) == EINVAL
    assert L.mcq_logits_refine_codes(None, 0, None, 1.0, 4, 256, 64, 1, None, p, None, None, 0, None, 0) == 0
    assert L.mcq_logits_refine_codes(None, 4, None, 1.0, 4, 8, 64, 1, p, p, None, None, 0, None, 0) == EUNSUP
    # mcq_prepare*: the domain first, then the pointers
    assert L.mcq_prepare(None, 1.0, None, None, 8, 8, 64, None, None) == EUNSUP
    assert L.mcq_prepare(p, 1.0, p, None, 8, 256, 64, p, None) == EINVAL                                # weight without bias
    assert L.mcq_prepare_dev(p, None, None, None, 8, 256, 64, p, None) == EINVAL
    assert L.mcq_prepare_params(p, None, p, 10.0, None, None, 8, 256, 64, p, None, None) == EINVAL


def test_module_api_surface_and_state_dict():
    import torch
    from quantization_amd import Quantizer, QuantizerTrainer
    q = Quantizer(dim=64, codebook_size=256, num_codebooks=4)
    sd = q.state_dict()
    shapes = {k: (tuple(v.shape), v.dtype) for k, v in sd.items()}
    assert shapes == {
        "centers": ((4, 256, 64), torch.float32), "logits_scale": ((), torch.float32),
        "centers_scale": ((), torch.float32), "id_buf": ((8,), torch.uint8),
        "to_logits.weight": ((1024, 64), torch.float32), "to_logits.bias": ((1024,), torch.float32)}
    assert torch.equal(q.centers.reshape(1024, 64), q.to_logits.weight)      # quantization.py:41-42
    q2 = Quantizer(64, 256, 4)
    assert q2.get_id() != q.get_id() and len(q.get_id()) == 8
    q2.load_state_dict(sd)
    assert q2.get_id() == q.get_id()                                         # test_train_hdf5.py:54
    assert "codebook_size=256" in q.show_init_invocation()
    for bad in (dict(dim=8, codebook_size=12, num_codebooks=2), dict(dim=8, codebook_size=16, num_codebooks=3)):
        with pytest.raises(AssertionError):
            Quantizer(**bad)
    with pytest.raises(AssertionError):
        QuantizerTrainer(dim=8, bytes_per_frame=3, device=torch.device("cpu"))
    # no CPU fallback: a CPU tensor is an error, not a slow path
    with pytest.raises(Exception):
        q.encode(torch.zeros(2, 64))


def test_product_quantizer_matches_definition():
    import torch
    from quantization_amd import Quantizer
    torch.manual_seed(0)
    q = Quantizer(8, 16, 4)
    with torch.no_grad():
        q.logits_scale.fill_(0.3)
        q.centers_scale.fill_(-0.2)
        q.centers.normal_()
    p = q.get_product_quantizer()
    assert (p.codebook_size, p.num_codebooks) == (256, 2)
    assert float(p.logits_scale) == float(q.logits_scale) and float(p.centers_scale) == float(q.centers_scale)
    for c in range(2):
        for k1 in (0, 5, 15):
            for k2 in (0, 7, 15):
                ko = k1 * 16 + k2                                            # quantization.py:107
                assert torch.equal(p.centers[c, ko], q.centers[2 * c, k1] + q.centers[2 * c + 1, k2])
                assert torch.equal(p.to_logits.weight[256 * c + ko],
                                   q.to_logits.weight[16 * 2 * c + k1] + q.to_logits.weight[16 * (2 * c + 1) + k2])
                assert p.to_logits.bias[256 * c + ko] == q.to_logits.bias[16 * 2 * c + k1] + q.to_logits.bias[16 * (2 * c + 1) + k2]


def test_workspace_and_prepared_sizes_over_the_domain():
    """mcq_encode_workspace_bytes / mcq_prepared_bytes for every (K, N) of the domain: positive, monotone in B up to the
    default chunk, below 4 GB at the largest shapes, and 'slack only' outside the domain."""
    from quantization_amd import _lib as m
    L = m.lib()
    for K in (16, 32, 64, 128, 256):
        for N in (1, 2, 4, 8, 16, 32, 64, 128):
            ok = N <= 64
            big = L.mcq_encode_workspace_bytes(10 ** 7, N, K, 512)
            small = L.mcq_encode_workspace_bytes(100, N, K, 512)
            if not ok:
                assert big == small
                continue
            assert 0 < small < big <= 4 * 2 ** 30, (K, N, small, big)
            nk = N * K
            assert L.mcq_prepared_bytes(N, K, 512) >= 4 * (2 * nk * 512 + nk * nk)
