"""CPU-only checks of tests/_fma_chain_np.py, the exact statement of the 2-D convolutions' accumulation order that
tests/test_gpu_conv2d.py holds the kernels to bit for bit: fmaf_np against the definition of correct rounding in exact rational
arithmetic, and the gathered chains against the float64 oracle tests/_specunet_np.py."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
from _fma_chain_np import chain, conv_weights, fmaf_np, gather_conv, gather_transpose, transpose_weights  # noqa: E402

U = 2.0 ** -24
F32 = np.float32
# a b = 2^-24 (1 - 2^-36), so a b + c lies 2^-60 below the tie between 1 + 2^-23 and 1 + 2^-22: the answer is 1 + 2^-23; float64
# cannot hold the 2^-60, lands on the tie, and the second rounding goes to the even neighbour 1 + 2^-22
DOUBLE_ROUNDING_TRAP = (F32(2.0 ** -12 * (1 + 2.0 ** -18)), F32(2.0 ** -12 * (1 - 2.0 ** -18)), F32(1 + 2.0 ** -23))


def _naive(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _traps():
    a, b, c = DOUBLE_ROUNDING_TRAP
    t = [(a, b, c), (-a, b, -c), (a, -b, -c),
         (a, b, F32(1 + 2.0 ** -22)),                        # just below the other kind of tie (the even neighbour below)
         (F32(2.0 ** -12 * (1 + 2.0 ** -18)), F32(2.0 ** -12 * (1 + 2.0 ** -17)), c),       # just above a tie
         (F32(2.0 ** -24), F32(1.0), F32(1.0)),              # exact ties: to even, down
         (F32(2.0 ** -24), F32(1.0), c),                     # and up
         (F32(-2.0 ** -24), F32(1.0), F32(1.0)),             # 1 - 2^-24 is a float32: exact
         (F32(-2.0 ** -25), F32(1.0), F32(1.0)),             # a tie below a power of two (the spacing halves there)
         (F32(3.0), F32(1.0 / 3.0), F32(-1.0)),              # cancellation: the product's low bits are the answer
         (F32(1 + 2.0 ** -23), F32(1 - 2.0 ** -23), F32(-1.0)),
         (F32(1.5), F32(2.0), F32(-3.0)), (F32(0.0), F32(5.0), F32(0.0)), (F32(0.0), F32(-5.0), F32(7.0)),
         (F32(2.0 ** -70), F32(2.0 ** -70), F32(1.0)),       # a product far below the addend's last bit
         (F32(-2.0 ** -70), F32(2.0 ** -70), F32(1.0)),
         (F32(2.0 ** 60), F32(2.0 ** 60), F32(-1.0))]
    return t


def _random_triples(n):
    rng = np.random.RandomState(20)
    a, b = rng.randn(n).astype(np.float32), rng.randn(n).astype(np.float32)
    c = rng.randn(n).astype(np.float32)
    k = n // 4
    # a quarter each: any addend; an addend that cancels the product to its last bits; addends 2^+-24 and 2^+-48 away, where the
    # smaller operand only decides the rounding
    c[k:2 * k] = -(a[k:2 * k] * b[k:2 * k]) * (1 + rng.randint(-3, 4, k) * np.float32(2.0 ** -23))
    c[2 * k:3 * k] *= np.float32(2.0) ** rng.choice([-24, -23, 23, 24, 25], k).astype(np.float32)
    c[3 * k:] *= np.float32(2.0) ** rng.choice([-48, -47, 47, 48], n - 3 * k).astype(np.float32)
    return a, b, c.astype(np.float32)


def _assert_correctly_rounded(a, b, c, got):
    """got is the float32 nearest the exact a b + c, ties to even -- by the definition, in exact rationals."""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    g = np.float32(got)
    assert np.isfinite(g)
    d = abs(exact - Fraction(float(g)))
    even = (int(g.view(np.uint32)) & 1) == 0
    for other in (np.nextafter(g, F32(-np.inf)), np.nextafter(g, F32(np.inf))):
        do = abs(exact - Fraction(float(other)))
        assert d <= do, (a, b, c, g, other)
        if d == do:
            assert even, (a, b, c, g, other)
    if exact == 0:
        assert g == 0


def test_fmaf_np_is_correctly_rounded():
    a, b, c = _random_triples(4000)
    ta, tb, tc = (np.array(v, dtype=np.float32) for v in zip(*_traps()))
    a, b, c = np.concatenate([ta, a]), np.concatenate([tb, b]), np.concatenate([tc, c])
    got = fmaf_np(a, b, c)
    assert got.dtype == np.float32 and got.shape == a.shape
    for i in range(a.size):
        _assert_correctly_rounded(a[i], b[i], c[i], got[i])
    # broadcasting, as chain uses it
    assert np.array_equal(fmaf_np(a[:8, None], b[None, :8], c[:8, None]), np.stack([fmaf_np(a[:8], b[j], c[:8]) for j in range(8)], 1))


def test_the_traps_catch_the_double_rounding_route():
    a, b, c = DOUBLE_ROUNDING_TRAP
    assert fmaf_np(a, b, c) == F32(1 + 2.0 ** -23)
    assert _naive(a, b, c) == F32(1 + 2.0 ** -22)            # the route fmaf_np must not take
    with pytest.raises(AssertionError):
        _assert_correctly_rounded(a, b, c, _naive(a, b, c))
    wrong = sum(bool(_naive(*t) != fmaf_np(*t)) for t in _traps())
    assert wrong >= 1


def test_non_finite_operands_pass_through():
    inf, nan = F32(np.inf), F32(np.nan)
    got = fmaf_np(np.array([nan, 1, inf, inf, 0], F32), np.array([1, nan, 2, 1, 3], F32), np.array([1, 1, 1, -inf, nan], F32))
    assert np.isnan(got[[0, 1, 3, 4]]).all() and got[2] == inf


@pytest.mark.parametrize("case", [(2, 4, 6, 1, 5), (1, 8, 6, 3, 4), (1, 2, 2, 4, 3)], ids=lambda c: "x".join(map(str, c)))
def test_conv_chain_against_the_float64_oracle(case):
    B, H, W, ci, co = case
    rng = np.random.RandomState(sum(case))
    x, w = (0.5 * rng.randn(B, H, W, ci)).astype(np.float32), (0.3 * rng.randn(5, 5, ci, co)).astype(np.float32)
    A = gather_conv(x)
    assert A.shape == (B * (H // 2) * (W // 2), 25 * ci)
    got = chain(A, conv_weights(w)).reshape(B, H // 2, W // 2, co)
    want = ora.conv2d_s2(torch.tensor(x, dtype=torch.float64), torch.tensor(w, dtype=torch.float64)).numpy()
    bound = (25 * ci + 4) * U * ora.abs_conv(x, w)
    assert (np.abs(got - want) <= bound).all() and np.abs(want).max() > 0
    # every input appears in A as often as outputs read it: the corner pixel (0, 0) once (the tap (1, 1) of output (0, 0))
    assert np.count_nonzero(A == x[0, 0, 0, 0]) == 1


@pytest.mark.parametrize("case", [(2, 3, 5, 3, 4), (1, 1, 5, 4, 3), (1, 5, 1, 4, 3), (1, 1, 1, 1, 1)], ids=lambda c: "x".join(map(str, c)))
def test_transpose_chain_against_the_float64_oracle(case):
    B, H, W, ci, co = case
    rng = np.random.RandomState(sum(case) + 1)
    x, w = (0.5 * rng.randn(B, H, W, ci)).astype(np.float32), (0.3 * rng.randn(5, 5, co, ci)).astype(np.float32)
    A = gather_transpose(x)
    assert A.shape == (B * 4 * H * W, 25 * ci)
    got = chain(A, transpose_weights(w)).reshape(B, 2 * H, 2 * W, co)
    want = ora.conv2d_transpose_s2(torch.tensor(x, dtype=torch.float64), torch.tensor(w, dtype=torch.float64)).numpy()
    bound = (25 * ci + 4) * U * ora.abs_transpose(x, w)
    assert (np.abs(got - want) <= bound).all() and np.abs(want).max() > 0
    # an output of class (py, px) has at most 2 or 3 live taps per axis
    live = (A.reshape(B, 2 * H, 2 * W, 25, ci) != 0).any(-1).sum(-1)
    assert live[:, 0::2, 0::2].max() <= 4 and live[:, 1::2, 1::2].max() <= 9 and live[:, 0::2, 1::2].max() <= 6
