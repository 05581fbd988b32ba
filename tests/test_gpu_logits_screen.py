"""The screened initial arg max (k_fgemm<FG_SCREEN> + k_fscreen_recheck: six limb products, the pairs they cannot decide
recomputed exactly) against the ten-product kernel (Quantizer.exact_logits = True, MCQ_ENCODE_EXACT_LOGITS): byte-equal codes
without refinement and after five passes.  Run on the MI355X: pytest -m gpu."""
import numpy as np
import pytest
import torch

from golden import fixtures, gen

pytestmark = pytest.mark.gpu

ALL = fixtures.names()


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def load_quantizer(state, D, K, N, device="cuda:0"):
    from quantization_amd import Quantizer
    q = Quantizer(D, K, N)
    sd = q.state_dict()
    for k, v in state.items():
        sd[k] = torch.from_numpy(np.asarray(v))
    q.load_state_dict(sd)
    if getattr(state, "scales_exp", None) is not None:
        q.pin_scale_factors(*state.scales_exp)
    return q.to(device)


def both(q, x, it):
    """codes of the screened path and of the ten-product kernel, int64 [B][N]"""
    q.exact_logits = False
    a = q.encode(x, it, as_bytes=False).cpu().numpy()
    q.exact_logits = True
    b = q.encode(x, it, as_bytes=False).cpu().numpy()
    q.exact_logits = False
    return a, b


def check(q, x, what):
    for it in (0, 5):
        a, b = both(q, x, it)
        nbad = int((a != b).any(axis=1).sum())
        assert nbad == 0, f"{what} iters={it}: {nbad} of {len(a)} vectors differ between the screened and the exact arg max"


@pytest.mark.parametrize("name", ALL)
def test_screened_codes_equal_exact_codes_on_every_fixture_shape(name):
    fx = fixtures.load(name)
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    check(q, torch.from_numpy(fx["x"]).cuda(), name)


def test_bench_shape_65536_frames():
    D, K, N = 512, 256, 8
    q = load_quantizer(gen.synthetic_state(103, D, K, N), D, K, N)
    x = torch.from_numpy(gen.make_gaussian(5, 65536, D)).cuda()
    check(q, x, "bench shape")
    # bytes as well (what bench.py encodes)
    q.exact_logits = False
    a = q.encode(x, 5)
    q.exact_logits = True
    b = q.encode(x, 5)
    q.exact_logits = False
    assert torch.equal(a, b)


@pytest.mark.parametrize("B", [1, 127, 1000, 8192 + 77])
def test_batch_that_is_not_a_multiple_of_the_tile(B):
    fx = fixtures.load("config_b_d512_n8")
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    x = gen.make_gaussian(11, B, fx["D"])
    check(q, torch.from_numpy(x).cuda(), f"config_b B={B}")


@pytest.mark.parametrize("name", ["config_b_d512_n8", "synth_d40_k64_n8", "synth_d64_k16_n32", "k512_d32_n4", "k1024_d24_n2"])
def test_zero_frames_every_pair_undecided(name):
    """all-zero frames (one input, 300 times: whatever one pair decides, all do) and frames equal to the data mean, which centre
    to zero rows so that the limb products vanish and a logit is fl(fl(wmu * ls) + bias)"""
    fx = fixtures.load(name)
    q = load_quantizer(fx["state"], fx["D"], fx["K"], fx["N"])
    check(q, torch.zeros(300, fx["D"]).cuda(), f"{name} zero frames")
    mean = q.get_data_mean().detach().reshape(1, -1).float()
    check(q, mean.expand(300, -1).contiguous().cuda(), f"{name} frames at the data mean")


@pytest.mark.parametrize("name", ["config_b_d512_n8", "synth_d40_k64_n8", "synth_d64_k16_n32", "k512_d32_n4"])
def test_duplicated_classifier_rows_lower_row_wins(name):
    """rows 2i and 2i + 1 of the classifier are made equal: every pair has two equal best values, so every pair goes through the
    recheck, and the first arg max is the even row"""
    fx = fixtures.load(name)
    st = fixtures.PinnedState(fx["state"])
    st.scales_exp = fx["state"].scales_exp
    w = np.array(st["to_logits.weight"], copy=True)
    b = np.array(st["to_logits.bias"], copy=True)
    w[1::2] = w[0::2]
    b[1::2] = b[0::2]
    st["to_logits.weight"], st["to_logits.bias"] = w, b
    q = load_quantizer(st, fx["D"], fx["K"], fx["N"])
    x = torch.from_numpy(fx["x"][:515]).cuda()
    check(q, x, f"{name} duplicated rows")
    a, _ = both(q, x, 0)
    assert (a % 2 == 0).all()
