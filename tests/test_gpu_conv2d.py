"""GPU tests of the spectrogram U-Net's layers as single operators (include/wun.h: wun_op_conv2d_s2,
wun_op_conv2d_transpose_s2) against the float64 oracle tests/_specunet_np.py.

Bound per output, derived and not measured: the kernels accumulate n <= 25 Cin products in fp32, one rounding each, and add the
bias, so |got - want| <= (25 Cin + 4) 2^-24 (sum |x| |w| + |bias|) -- the standard bound of recursive summation, the sum formed
by the oracle on the absolute values.  The transposed conv sums at most 9 Cin products per output; it is held to the same figure.
Epilogue cases: with e the bound above on the pre-activation z and u = 2^-24,
  batch norm   out = (z - mean) s + beta, s = 1 / sqrt(var + 1e-3) with at most 3 roundings, the difference, the product and the
               sum one each: |err| <= s e + 8 u (s (|z| + |mean|) + |beta|)
  LeakyReLU, ReLU are 1-Lipschitz (0.2 z adds one rounding: + u |out|); sigmoid is 1/4-Lipschitz and expf, the sum and the
               quotient cost a few roundings of a value below 1: |err| <= e / 4 + 8 u.
Shapes are the smallest at which each path can go wrong (see the tables): padding-only taps, the VALU kernels of Cin == 1 and
Cout == 1, sizes off the 64 x 32 tile and the 32-index reduction chunk, two excerpts in one row tile, a row tile crossing rows."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

from wave_u_net_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ACTS = {None: 0, "lrelu": 1, "relu": 2, "sigmoid": 3}
# (B, H, W, Cin, Cout)
CONV_CASES = [
    (1, 2, 2, 1, 1),        # padding taps only
    (2, 4, 6, 1, 5),        # first-layer shape (VALU); two excerpts in one tile
    (1, 8, 16, 3, 17),      # both off the 16 tile
    (3, 6, 10, 16, 32),
    (1, 2, 34, 33, 16),     # reduction off any chunk; a row tile crossing image rows
]
# (B, H, W, c0, c1, Cout): the input is [c0 + c1] channels, given as two ranges when c1 > 0
TRANSPOSE_CASES = [
    (1, 1, 1, 1, 0, 1),
    (2, 3, 5, 5, 0, 3),
    (1, 4, 8, 17, 0, 1),    # the mask-layer shape (VALU)
    (2, 3, 5, 3, 5, 7),     # two ranges
    (1, 4, 6, 16, 16, 16),
    (1, 4, 8, 3, 5, 1),     # two ranges into the mask layer
]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def run_conv(lib, x, w, bias=None, bn=None, act=None, xdev=None):
    """numpy in, numpy out; xdev: a device tensor to read x from instead."""
    B, H, W, ci = x.shape
    co = w.shape[3]
    xd = xdev if xdev is not None else _dev(x)
    wd, bd = _dev(w), _dev(bias)
    bnd = [_dev(a) for a in bn] if bn is not None else [None] * 3
    y = torch.full((B, H // 2, W // 2, co), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.wun_op_conv2d_s2(xd.data_ptr(), wd.data_ptr(), _ptr(bd), _ptr(bnd[0]), _ptr(bnd[1]), _ptr(bnd[2]), y.data_ptr(),
                                    B, H, W, ci, co, ACTS[act], _stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run_transpose(lib, x0, x1, w, bias=None, bn=None, act=None, x0dev=None):
    B, H, W, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[3]
    co = w.shape[2]
    x0d = x0dev if x0dev is not None else _dev(x0)
    x1d, wd, bd = _dev(x1), _dev(w), _dev(bias)
    bnd = [_dev(a) for a in bn] if bn is not None else [None] * 3
    y = torch.full((B, 2 * H, 2 * W, co), float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.wun_op_conv2d_transpose_s2(x0d.data_ptr(), c0, _ptr(x1d), c1, wd.data_ptr(), _ptr(bd), _ptr(bnd[0]), _ptr(bnd[1]),
                                              _ptr(bnd[2]), y.data_ptr(), B, H, W, co, ACTS[act], _stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _t(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def _conv_fixture(case, seed=0):
    B, H, W, ci, co = case
    rng = np.random.RandomState(sum(case) + seed)
    return ((0.5 * rng.randn(B, H, W, ci)).astype(np.float32), (0.3 * rng.randn(5, 5, ci, co)).astype(np.float32),
            (0.1 * rng.randn(co)).astype(np.float32))


def _transpose_fixture(case, seed=0):
    B, H, W, c0, c1, co = case
    rng = np.random.RandomState(sum(case) + seed)
    x = (0.5 * rng.randn(B, H, W, c0 + c1)).astype(np.float32)
    return x, (0.3 * rng.randn(5, 5, co, c0 + c1)).astype(np.float32), (0.1 * rng.randn(co)).astype(np.float32)


def _bn(co, seed):
    rng = np.random.RandomState(seed)
    return ((0.1 * rng.randn(co)).astype(np.float32), rng.uniform(0.5, 2.0, co).astype(np.float32), (0.1 * rng.randn(co)).astype(np.float32))


def _epilogue_bound(z, e, bn, act):
    """The docstring's bounds; z float64 pre-activation (bias included), e its bound.  -> (want, bound)."""
    out, b = z, e
    if bn is not None:
        mean, var, beta = (np.asarray(a, np.float64) for a in bn)
        s = 1.0 / np.sqrt(var + 1e-3)
        out = (z - mean) * s + beta
        b = s * e + 8 * U * (s * (np.abs(z) + np.abs(mean)) + np.abs(beta))
    if act == "lrelu":
        out = np.where(out > 0, out, 0.2 * out)
        b = b + U * np.abs(out)
    elif act == "relu":
        out = np.maximum(out, 0.0)
    elif act == "sigmoid":
        out = 1.0 / (1.0 + np.exp(-out))
        b = b / 4 + 8 * U
    return out, b


def _check(name, got, want, bound):
    assert np.isfinite(got).all() and got.shape == want.shape        # every output was written
    ratio = (np.abs(got - want) / np.maximum(bound, 1e-300)).max()
    record(name, "max err / bound", ratio, 1.0)
    assert (np.abs(got - want) <= bound).all()


# ---------------------------------------------------------------------------------------------------- the strided conv
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_against_float64(lib, case):
    x, w, bias = _conv_fixture(case)
    got = run_conv(lib, x, w, bias)
    want = (ora.conv2d_s2(_t(x), _t(w)) + _t(bias)).numpy()
    bound = (25 * case[3] + 4) * U * (ora.abs_conv(x, w) + np.abs(bias))
    _check("test_conv2d_against_float64[%s]" % "x".join(map(str, case)), got, want, bound)
    # without a bias: the plain sum
    got0 = run_conv(lib, x, w)
    _check("test_conv2d_against_float64[%s]" % "x".join(map(str, case)), got0, ora.conv2d_s2(_t(x), _t(w)).numpy(),
           (25 * case[3] + 4) * U * ora.abs_conv(x, w))


@pytest.mark.parametrize("act, with_bn", [("lrelu", True), ("relu", True), ("sigmoid", False)])
@pytest.mark.parametrize("case", [(2, 4, 6, 1, 5), (1, 8, 16, 3, 17)], ids=["valu", "mfma"])
def test_conv2d_epilogues(lib, case, act, with_bn):
    x, w, bias = _conv_fixture(case, seed=1)
    bn = _bn(case[4], 5) if with_bn else None
    got = run_conv(lib, x, w, bias, bn, act)
    z = (ora.conv2d_s2(_t(x), _t(w)) + _t(bias)).numpy()
    e = (25 * case[3] + 4) * U * (ora.abs_conv(x, w) + np.abs(bias))
    want, bound = _epilogue_bound(z, e, bn, act)
    o = ora.epilogue(_t(z), None, None if bn is None else [_t(a) for a in bn], act).numpy()
    assert np.abs(o - want).max() <= 1e-12                   # the two statements of the epilogue agree
    _check("test_conv2d_epilogues[%s-%s]" % (act, "x".join(map(str, case))), got, want, bound)


@pytest.mark.parametrize("case", [(1, 4, 6, 1, 5), (1, 6, 10, 16, 32), (1, 2, 34, 33, 16)], ids=lambda c: "x".join(map(str, c)))
def test_conv2d_bits_do_not_depend_on_batch_or_alignment(lib, case):
    x, w, bias = _conv_fixture(case, seed=2)
    bn = _bn(case[4], 6)
    alone = run_conv(lib, x, w, bias, bn, "lrelu")
    rng = np.random.RandomState(9)
    batch = np.concatenate([(0.5 * rng.randn(*x.shape)).astype(np.float32), x, (0.5 * rng.randn(*x.shape)).astype(np.float32)])
    inside = run_conv(lib, batch, w, bias, bn, "lrelu")
    assert np.array_equal(alone.view(np.uint32), inside[1:2].view(np.uint32))
    shifted = run_conv(lib, x, w, bias, bn, "lrelu", xdev=_offset_copy(_dev(x)))
    assert np.array_equal(alone.view(np.uint32), shifted.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- the transposed conv
@pytest.mark.parametrize("case", TRANSPOSE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv2d_transpose_against_float64(lib, case):
    """Two-range inputs against the oracle on the concatenated tensor."""
    x, w, bias = _transpose_fixture(case)
    c0, c1 = case[3], case[4]
    x0 = np.ascontiguousarray(x[..., :c0])
    x1 = np.ascontiguousarray(x[..., c0:]) if c1 else None
    got = run_transpose(lib, x0, x1, w, bias)
    want = (ora.conv2d_transpose_s2(_t(x), _t(w)) + _t(bias)).numpy()
    bound = (25 * (c0 + c1) + 4) * U * (ora.abs_transpose(x, w) + np.abs(bias))
    _check("test_conv2d_transpose_against_float64[%s]" % "x".join(map(str, case)), got, want, bound)


@pytest.mark.parametrize("act, with_bn", [("relu", True), ("lrelu", True), ("sigmoid", False)])
@pytest.mark.parametrize("case", [(1, 4, 8, 3, 5, 1), (2, 3, 5, 3, 5, 7)], ids=["valu", "mfma"])
def test_conv2d_transpose_epilogues(lib, case, act, with_bn):
    x, w, bias = _transpose_fixture(case, seed=1)
    c0 = case[3]
    bn = _bn(case[5], 7) if with_bn else None
    got = run_transpose(lib, np.ascontiguousarray(x[..., :c0]), np.ascontiguousarray(x[..., c0:]), w, bias, bn, act)
    z = (ora.conv2d_transpose_s2(_t(x), _t(w)) + _t(bias)).numpy()
    e = (25 * x.shape[3] + 4) * U * (ora.abs_transpose(x, w) + np.abs(bias))
    want, bound = _epilogue_bound(z, e, bn, act)
    _check("test_conv2d_transpose_epilogues[%s-%s]" % (act, "x".join(map(str, case))), got, want, bound)


@pytest.mark.parametrize("case", [(1, 3, 5, 5, 0, 3), (1, 4, 8, 17, 0, 1), (1, 4, 6, 16, 16, 16)], ids=lambda c: "x".join(map(str, c)))
def test_conv2d_transpose_bits_do_not_depend_on_batch_or_alignment(lib, case):
    x, w, bias = _transpose_fixture(case, seed=2)
    c0, c1 = case[3], case[4]
    split = lambda a: (np.ascontiguousarray(a[..., :c0]), np.ascontiguousarray(a[..., c0:]) if c1 else None)   # noqa: E731
    alone = run_transpose(lib, *split(x), w, bias, None, "relu")
    rng = np.random.RandomState(9)
    batch = np.concatenate([(0.5 * rng.randn(*x.shape)).astype(np.float32), x, (0.5 * rng.randn(*x.shape)).astype(np.float32)])
    inside = run_transpose(lib, *split(batch), w, bias, None, "relu")
    assert np.array_equal(alone.view(np.uint32), inside[1:2].view(np.uint32))
    x0, x1 = split(x)
    shifted = run_transpose(lib, x0, x1, w, bias, None, "relu", x0dev=_offset_copy(_dev(x0)))
    assert np.array_equal(alone.view(np.uint32), shifted.view(np.uint32))


def test_valu_and_mfma_kernels_agree_bit_for_bit(lib):
    """The thin layers run on the VALU with the MFMA's order (a k-ordered fmaf chain): a Cout == 1 transposed conv gives the bits
    of column 0 of the same layer widened to two columns, which runs on the MFMA."""
    x, w, bias = _transpose_fixture((1, 4, 8, 17, 0, 1), seed=3)
    thin = run_transpose(lib, x, None, w, bias)
    w2 = np.concatenate([w, 0.5 * w], axis=2)
    wide = run_transpose(lib, x, None, w2, np.concatenate([bias, bias]))
    assert np.array_equal(thin[..., 0].view(np.uint32), wide[..., 0].view(np.uint32))


# ---------------------------------------------------------------------------------------------------- refusals
def test_refusals(lib):
    x = torch.zeros(64, device="cuda")
    p = x.data_ptr()
    assert lib.wun_op_conv2d_s2(p, p, None, None, None, None, p, 1, 3, 2, 1, 1, 0, _stream()) == -1      # odd H
    assert lib.wun_op_conv2d_s2(p, p, None, None, None, None, p, 1, 2, 3, 1, 1, 0, _stream()) == -1      # odd W
    assert lib.wun_op_conv2d_s2(None, p, None, None, None, None, p, 1, 2, 2, 1, 1, 0, _stream()) == -1
    assert lib.wun_op_conv2d_s2(p, None, None, None, None, None, p, 1, 2, 2, 1, 1, 0, _stream()) == -1
    assert lib.wun_op_conv2d_s2(p, p, None, None, None, None, None, 1, 2, 2, 1, 1, 0, _stream()) == -1
    assert lib.wun_op_conv2d_transpose_s2(None, 1, None, 0, p, None, None, None, None, p, 1, 1, 1, 1, 0, _stream()) == -1
    assert lib.wun_op_conv2d_transpose_s2(p, 1, None, 0, None, None, None, None, None, p, 1, 1, 1, 1, 0, _stream()) == -1
    assert lib.wun_op_conv2d_transpose_s2(p, 1, None, 0, p, None, None, None, None, None, 1, 1, 1, 1, 0, _stream()) == -1
    assert lib.wun_op_conv2d_transpose_s2(p, 1, None, 3, p, None, None, None, None, p, 1, 1, 1, 1, 0, _stream()) == -1
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0                       # nothing ran
