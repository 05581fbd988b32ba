"""Host-side checks of tests/train_grid.py (no GPU): the constants it reads from the kernel sources are where the GPU cases of
tests/test_gpu_train_kernels.py expect them, every case reaches the path it names, and the mirror agrees with the sizes the
library itself reports."""
import pytest

import test_gpu_train_kernels as T
import train_grid as tg


def test_constants_read_from_the_driver():
    assert tg.constants() == dict(
        loss_waves=4, reduce_unroll=16, loss_chunks_max=1024, loss_rows_min=64, loss_rows_round=16, wg_m=128, wg_n=64,
        wb_m=128, wb_n=128, bf3_min_m=1024, bf3_min_b=2048, bf3_target=256, bf3_rows_min=512, f32_target=2048,
        f32_rows_min=128, f32_splits_max=64, split_round=32, db_k_wide=64, db_d4=1024, db_d2=512, adam_blocks_max=2048)


def test_loss_cases_reach_their_paths():
    U = tg.constants()["reduce_unroll"]
    Bs = {B for _, _, B, _ in T.LOSS_CASES}
    assert {1, 3, 63, 65, 333} <= Bs
    assert {K for K, _, _, _ in T.LOSS_CASES} == {16, 32, 64, 128, 256}
    assert {1, 64} <= {N for _, N, _, _ in T.LOSS_CASES}
    assert {"trained", "spread200", "offset1000"} == {s for _, _, _, s in T.LOSS_CASES}
    # more than 64 rows per chunk, at 65,537 and near 2^20 rows
    big = [B for B in Bs if tg.loss_rows_per_chunk(B) > 64]
    assert 65537 in big and any(B >= 1_000_000 for B in big)
    assert tg.loss_rows_per_chunk(65537) == 80 and tg.loss_rows_per_chunk(1_048_575) == 1024
    # chunk counts that leave a trailing group of fewer than 16 chunks in k_loss_reduce, and one that does not
    assert tg.loss_chunks(333) == 6 and tg.loss_chunks(65537) % U == 4
    assert any(tg.loss_chunks(B) % U == 0 and tg.loss_chunks(B) >= U for B in Bs)
    # K < 64 packs 64 / K rows into a wave
    assert [tg.rows_per_wave(K) for K in (16, 32, 64, 128, 256)] == [4, 2, 1, 1, 1]


def test_recon_cases_reach_both_branches():
    scalar = [D for D, _, _, aligned in T.RECON_CASES if not tg.recon_vector_branch(D, aligned)]
    vector = [D for D, _, _, aligned in T.RECON_CASES if tg.recon_vector_branch(D, aligned)]
    assert {1, 3, 30, 130, 514, 777} <= set(scalar) and {64, 512, 768} <= set(vector)
    assert any(D % 4 == 0 and not aligned for D, _, _, aligned in T.RECON_CASES)     # the offset view
    assert any(D > 64 for D in scalar)


def test_decode_backward_cases_reach_every_width_and_mapping():
    seen = {(tg.db_cw_of(D, K), tg.db_xcd_mapping(D, K)) for D, K, _, _ in T.DB_CASES}
    assert {1, 2, 4} == {cw for cw, _ in seen} and {True, False} == {m for _, m in seen}
    by = {(D, K): (tg.db_cw_of(D, K), tg.db_chunks(D, tg.db_cw_of(D, K)), tg.db_xcd_mapping(D, K)) for D, K, _, _ in T.DB_CASES}
    assert by[(768, 256)] == (4, 3, False)
    assert by[(320, 16)] == (1, 5, False)
    assert by[(512, 16)] == (2, 4, True)
    assert by[(600, 16)] == (2, 5, False)
    assert by[(4096, 16)] == (4, 16, False)
    assert by[(30, 16)] == (1, 1, True)
    assert {0, 1, 4097} <= {B for _, _, B, _ in T.DB_CASES}


def test_weight_grad_cases_reach_empty_and_short_splits():
    plans = {(B, M, D): tg.wgrad_plan(B, M, D) for B, M, D in T.WGRAD_CASES}
    bf3, s, rps, rows = plans[(8200, 128, 64)]
    assert not bf3 and s == 64 and rps == 160 and rows[51] == 40 and rows[52:] == [0] * 12
    bf3, s, rps, rows = plans[(16385, 1024, 128)]
    assert bf3 and s == 32 and rps == 544 and rows[30] == 65 and rows[31] == 0
    assert not plans[(2047, 1024, 128)][0] and plans[(2048, 1024, 128)][0]
    assert {1, 3, 130} <= {D for _, M, D in T.WGRAD_CASES if M == 16}


def test_adam_cases_reach_the_second_trip():
    trips = {n: tg.adam_trips(n) for n in T.ADAM_SIZES}
    assert trips[2097152] == 1 and trips[2097155] == 2 and trips[2099208] == 2
    assert 2099208 - tg.adam_blocks(2099208) * 256 * 4 == 2056


def test_grad_tail_sizes_straddle_the_strides():
    assert {0, 1, 1023, 1024, 8192, 8193, 100000} == set(T.TAIL_SIZES)


@pytest.mark.parametrize("B,N,K", [(1, 1, 16), (3, 64, 256), (333, 8, 32), (65537, 1, 16), (1_048_575, 1, 16), (4096, 8, 256)])
def test_loss_mirror_matches_the_library(B, N, K):
    from quantization_amd import _lib
    L = _lib.lib()
    assert L.mcq_loss_workspace_bytes(B, N, K) == tg.loss_workspace_bytes(B, N, K)
    assert L.mcq_loss_bwd_waves(B, N, K) == tg.loss_bwd_waves(B, N, K)


@pytest.mark.parametrize("N,K,D", [(8, 256, 768), (16, 16, 320), (16, 16, 512), (16, 16, 600), (4, 16, 4096), (2, 16, 30),
                                   (8, 256, 512), (64, 16, 130)])
def test_decode_backward_mirror_matches_the_library(N, K, D):
    from quantization_amd import _lib
    assert _lib.lib().mcq_decode_backward_waves(N, K, D) == tg.decode_backward_waves(N, K, D)


@pytest.mark.parametrize("B,M,D", [(8200, 128, 64), (16385, 1024, 128), (2047, 1024, 128), (2048, 1024, 128), (4096, 2048, 512),
                                   (5, 16, 3), (1, 16, 1)])
def test_weight_grad_mirror_matches_the_library(B, M, D):
    from quantization_amd import _lib
    assert _lib.lib().mcq_weight_grad_workspace_bytes(B, M, D) == tg.weight_grad_workspace_bytes(B, M, D)
