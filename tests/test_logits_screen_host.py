"""The margin of the screened logits arg max (k_fgemm<FG_SCREEN>, mcq_fix_kernels.h) restated on the host and checked
against exact integer limb sums (tests/logits_screen.py): on every fixture state with its own frames, on four kinds of
frames against the benchmark's state, and on constructed worst cases.  No GPU needed."""
import numpy as np
import pytest

import logits_screen as ls
from golden import fixtures, gen

ALL = fixtures.names()


@pytest.mark.parametrize("name", ALL)
def test_margin_is_sound_on_every_fixture_state_with_its_own_frames(name):
    fx = fixtures.load(name)
    ops = ls.state_operands(fx["state"], fx["x"][:256])
    share = ls.assert_sound(ls.screen(*ops, fx["N"], fx["K"]), name)
    print(f"{name}: undecided {100 * share:.3f} %")


@pytest.mark.parametrize("kind", ["gaussian", "mean10", "student2", "outlier300"])
def test_margin_is_sound_and_not_vacuous_on_the_bench_state(kind):
    D, K, N, B = 512, 256, 8, 2048
    state = gen.synthetic_state(103, D, K, N)
    ops = ls.state_operands(state, gen.make_kind(kind, 0, B, D))
    share = ls.assert_sound(ls.screen(*ops, N, K), kind)
    print(f"bench state, {kind}: undecided {100 * share:.3f} % of {B * N} pairs")
    if kind == "gaussian":
        # neither everything (a margin that decides nothing saves nothing) nor nothing (a margin of zero would pass the soundness
        # checks only by luck): at least one pair and at most 5 % of them
        assert 1.0 / (B * N) <= share <= 0.05, share


def _limbs_const(rows, cols, vals):
    return [np.full((rows, cols), v, np.int64) for v in vals]


@pytest.mark.parametrize("Dq", [128, 512, 1024, 16384])
@pytest.mark.parametrize("sign", [(-128, -128), (127, 127), (-128, 127)])
def test_dropped_class_at_its_integer_extreme(Dq, sign):
    """every limb of both operands at -128 / 127 with equal signs per operand: |T_3| = 4 * Dq * 128 * 128 (or as close as 127
    allows), the largest the integers permit; rows whose limbs 0-2 are zero (t' = 0, t = T_3) beside them; exponents at the
    maximum of a codebook and far below it; biases and mean products of both signs and sizes"""
    K, N, B = 16, 4, 6
    rng = np.random.default_rng(Dq * 1000 + 300 + sign[0] + 2 * sign[1])
    sx, sw = sign
    lx = _limbs_const(B, Dq, (sx, sx, sx, sx))
    lw = _limbs_const(N * K, Dq, (sw, sw, sw, sw))
    for l in range(3):                       # every fourth row: only limb 3 is set
        lw[l][::4] = 0
    for l in range(4):                       # a few random rows among them
        lw[l][1::8] = rng.integers(-128, 128, size=lw[l][1::8].shape)
    lx[3][1] = -sx - (1 if sx < 0 else 0)    # a frame whose limb 3 has the other sign
    ex = np.array([0, 3, -20, 7, 1, -125])[:B]
    ew = rng.integers(-6, 2, size=N * K)
    ew[::K] = 2                              # the maximum of each codebook sits on one row
    for scale in (0.0, 1.0, 1e4):
        wmu = (rng.standard_normal(N * K) * scale).astype(np.float32)
        bias = (rng.standard_normal(N * K) * scale).astype(np.float32)
        for lsc in (0.37, 1.0, 54.6):
            r = ls.screen(lx, ex, lw, ew, wmu, bias, lsc, N, K)
            ls.assert_sound(r, f"Dq={Dq} sign={sign} scale={scale} ls={lsc}")
    T3 = ls.limb_sums(lx, lw)[3]
    assert np.abs(T3).max() >= 4 * Dq * 127 * 127


def test_row_maximum_of_exactly_a_power_of_two_and_zero_frames():
    D, K, N, B = 96, 32, 4, 64
    state = gen.synthetic_state(3, D, K, N)
    x = gen.make_gaussian(1, B, D)
    x[::2] /= np.abs(x[::2]).max(axis=1, keepdims=True)      # row maximum exactly 1.0
    x[1::4] = 0.0
    ops = list(ls.state_operands(state, x))
    # (state_operands centres the frames; these are meant as they are)
    ops[0], ops[1] = ls.limbs_of(x)
    assert (ops[1][::2] == 1).all()                           # max |v| = 2^0 < 2^e: e = 1
    w = np.array(state["to_logits.weight"], copy=True)
    w[::3] *= (2.0 / np.abs(w[::3]).max(axis=1, keepdims=True)).astype(np.float32)
    ops[2], ops[3] = ls.limbs_of(w)
    r = ls.screen(*ops, N, K)
    ls.assert_sound(r, "power-of-two maxima / zero frames")
    # a zero frame's logits are exact from six products: whatever the decision, both winners agree
    assert (r["winner"][1::4] == r["exact"][1::4]).all()


def test_duplicated_rows_are_always_undecided():
    D, K, N, B = 64, 16, 4, 32
    state = gen.synthetic_state(5, D, K, N)
    w = np.array(state["to_logits.weight"], copy=True)
    b = np.array(state["to_logits.bias"], copy=True)
    w[1::2], b[1::2] = w[0::2], b[0::2]
    st = dict(state)
    st["to_logits.weight"], st["to_logits.bias"] = w, b
    r = ls.screen(*ls.state_operands(st, gen.make_gaussian(2, B, D)), N, K)
    assert r["undecided"].all()
    ls.assert_sound(r, "duplicated rows")


def test_rn24_is_the_float_conversion():
    rng = np.random.default_rng(0)
    n = np.concatenate([rng.integers(-2 ** 40, 2 ** 40, 20000), rng.integers(-2 ** 26, 2 ** 26, 20000),
                        np.array([0, 1, -1, 2 ** 24, 2 ** 24 + 1, 2 ** 24 + 3, 2 ** 25 + 2, 2 ** 25 + 6, -(2 ** 24 + 1)])])
    assert np.array_equal(ls.rn24(n), n.astype(np.float32).astype(np.int64))
