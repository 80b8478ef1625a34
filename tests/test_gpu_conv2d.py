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
from _fma_chain_np import chain, conv_weights, gather_conv, gather_transpose, transpose_weights  # noqa: E402
from _unaligned import _offset_copy, _offset_full  # noqa: E402

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
    (2, 10, 14, 3, 40),     # M = 70: two row tiles (the second of 6 rows), an excerpt boundary inside the first; two column
                            # tiles (the second of 8 columns); a reduction of 75 = three chunks, the last of 11
    (1, 18, 16, 5, 70),     # M = 72; three column tiles, 6 columns in the last
    (1, 4, 6, 5, 1),        # Cout == 1 with Cin > 1: one live column on the MFMA
    (1, 2, 2, 4, 3),        # a map smaller than the filter, on the MFMA
    (1, 16, 18, 1, 33),     # the VALU kernel over several workgroups (2376 outputs)
]
# (B, H, W, c0, c1, Cout): the input is [c0 + c1] channels, given as two ranges when c1 > 0
TRANSPOSE_CASES = [
    (1, 1, 1, 1, 0, 1),
    (2, 3, 5, 5, 0, 3),
    (1, 4, 8, 17, 0, 1),    # the mask-layer shape (VALU)
    (2, 3, 5, 3, 5, 7),     # two ranges
    (1, 4, 6, 16, 16, 16),
    (1, 4, 8, 3, 5, 1),     # two ranges into the mask layer
    (2, 5, 7, 3, 2, 40),    # M = 70 per class: two row tiles, two column tiles, two ranges
    (1, 9, 8, 5, 0, 70),    # M = 72; three column tiles
    (1, 3, 4, 1, 0, 5),     # Cin == 1 on the MFMA: a reduction of 4 to 9, less than one staged chunk
    (1, 1, 5, 4, 0, 3),     # a one-row map on the MFMA
    (1, 5, 1, 4, 0, 3),     # a one-column map on the MFMA
    (1, 16, 18, 2, 3, 1),   # the VALU kernel over several workgroups per class (288 outputs each)
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


def _place(name, a, off):
    """A device copy of a numpy operand; one float behind an allocation's start if `off` names it."""
    d = _dev(a)
    return _offset_copy(d) if d is not None and name in off else d


def run_conv(lib, x, w, bias=None, bn=None, act=None, xdev=None, off=()):
    """numpy in, numpy out; xdev: a device tensor to read x from instead; off: the operands (of x, w, bias, mean, var, beta, y) to
    place at a pointer that is 4-byte but not 8-byte aligned."""
    B, H, W, ci = x.shape
    co = w.shape[3]
    xd = xdev if xdev is not None else _place("x", x, off)
    wd, bd = _place("w", w, off), _place("bias", bias, off)
    bnd = [_place(n, a, off) for n, a in zip(("mean", "var", "beta"), bn)] if bn is not None else [None] * 3
    shape = (B, H // 2, W // 2, co)
    y = _offset_full(shape, float("nan")) if "y" in off else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    _lib.check(lib.wun_op_conv2d_s2(xd.data_ptr(), wd.data_ptr(), _ptr(bd), _ptr(bnd[0]), _ptr(bnd[1]), _ptr(bnd[2]), y.data_ptr(),
                                    B, H, W, ci, co, ACTS[act], _stream()))
    torch.cuda.synchronize()
    return y.cpu().numpy()


def run_transpose(lib, x0, x1, w, bias=None, bn=None, act=None, x0dev=None, off=()):
    """off: as run_conv, of x0, x1, w, bias, mean, var, beta, y."""
    B, H, W, c0 = x0.shape
    c1 = 0 if x1 is None else x1.shape[3]
    co = w.shape[2]
    x0d = x0dev if x0dev is not None else _place("x0", x0, off)
    x1d, wd, bd = _place("x1", x1, off), _place("w", w, off), _place("bias", bias, off)
    bnd = [_place(n, a, off) for n, a in zip(("mean", "var", "beta"), bn)] if bn is not None else [None] * 3
    shape = (B, 2 * H, 2 * W, co)
    y = _offset_full(shape, float("nan")) if "y" in off else torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
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


# ---------------------------------------------------------------------------------------------------- the promised order
def _id(case):
    return "x".join(map(str, case))


def _assert_bits(name, got, want):
    assert got.shape == want.shape and np.isfinite(got).all()
    differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    record(name, "outputs with other bits", differ, 0.0)
    assert differ == 0


@pytest.mark.parametrize("case", CONV_CASES, ids=_id)
def test_conv2d_is_the_ascending_fmaf_chain(lib, case):
    """include/wun.h: "reduction in ascending (ky, kx, ci) order in one accumulator per output", VALU and MFMA "same bits" --
    against tests/_fma_chain_np.py, which states that order in exact arithmetic and shares nothing with the kernels."""
    x, w, _ = _conv_fixture(case, seed=4)
    got = run_conv(lib, x, w)
    want = chain(gather_conv(x), conv_weights(w)).reshape(got.shape)
    _assert_bits("test_conv2d_is_the_ascending_fmaf_chain[%s]" % _id(case), got, want)


@pytest.mark.parametrize("case", TRANSPOSE_CASES, ids=_id)
def test_conv2d_transpose_is_the_ascending_fmaf_chain(lib, case):
    x, w, _ = _transpose_fixture(case, seed=4)
    c0, c1 = case[3], case[4]
    got = run_transpose(lib, np.ascontiguousarray(x[..., :c0]), np.ascontiguousarray(x[..., c0:]) if c1 else None, w)
    want = chain(gather_transpose(x), transpose_weights(w)).reshape(got.shape)
    _assert_bits("test_conv2d_transpose_is_the_ascending_fmaf_chain[%s]" % _id(case), got, want)


# ---------------------------------------------------------------------------------------------------- the receptive field
def _probe_pixels(H, W):
    """The four corners, one element on each edge, one interior element."""
    return [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, 1), (H // 2, 0), (1, W - 1), (H // 2, W // 2 - 1)]


def _assert_footprint(got, clean, mask, what):
    """NaN exactly on mask [B, H, W] (every channel), the clean run's bits everywhere else."""
    nan = np.isnan(got)
    assert np.array_equal(nan, np.broadcast_to(mask[..., None], got.shape)), what
    assert np.array_equal(got.view(np.uint32)[~nan], clean.view(np.uint32)[~nan]), what


@pytest.mark.parametrize("case", [(2, 10, 14, 3, 40), (2, 4, 6, 1, 5)], ids=["mfma", "valu"])
def test_conv2d_footprint(lib, case):
    """Output (b, y, x, any co) depends on input (b, iy, ix, any ci) exactly when 2y - 1 <= iy <= 2y + 3 and 2x - 1 <= ix <= 2x + 3:
    one NaN in the input must come out there and nowhere else, and all other outputs keep their bits."""
    B, H, W, ci, co = case
    x, w, bias = _conv_fixture(case, seed=6)
    clean = run_conv(lib, x, w, bias)
    assert np.isfinite(clean).all()
    y, xx = np.arange(H // 2), np.arange(W // 2)
    for b in range(B):
        for k, (iy, ix) in enumerate(_probe_pixels(H, W)):
            xp = x.copy()
            xp[b, iy, ix, k % ci] = np.nan
            mask = np.zeros((B, H // 2, W // 2), bool)
            mask[b] = ((2 * y - 1 <= iy) & (iy <= 2 * y + 3))[:, None] & ((2 * xx - 1 <= ix) & (ix <= 2 * xx + 3))[None, :]
            assert mask.any()
            _assert_footprint(run_conv(lib, xp, w, bias), clean, mask, (b, iy, ix))
    # one NaN in the weights of one output channel (in the second column tile where there is one): that channel alone
    wp = w.copy()
    wp[2, 3, ci - 1, co - 2] = np.nan
    got = run_conv(lib, x, wp, bias)
    keep = np.arange(co) != co - 2
    assert np.isnan(got[..., co - 2]).all()                  # (a tap outside the map enters as 0 x NaN)
    assert np.array_equal(got[..., keep].view(np.uint32), clean[..., keep].view(np.uint32))


@pytest.mark.parametrize("case", [(2, 5, 7, 3, 2, 40), (1, 16, 18, 2, 3, 1)], ids=["mfma", "valu"])
def test_conv2d_transpose_footprint(lib, case):
    """Output (b, ty, tx) depends on input (b, iy, ix) of either range exactly when ty = 2 iy + ky - 1 and tx = 2 ix + kx - 1 for
    some ky, kx in 0..4."""
    B, H, W, c0, c1, co = case
    x, w, bias = _transpose_fixture(case, seed=6)
    split = lambda a: (np.ascontiguousarray(a[..., :c0]), np.ascontiguousarray(a[..., c0:]))   # noqa: E731
    clean = run_transpose(lib, *split(x), w, bias)
    assert np.isfinite(clean).all()
    ty, tx = np.arange(2 * H), np.arange(2 * W)
    for b in range(B):
        for k, (iy, ix) in enumerate(_probe_pixels(H, W)):
            my = np.zeros(2 * H, bool)
            mx = np.zeros(2 * W, bool)
            for kk in range(5):
                my |= ty == 2 * iy + kk - 1
                mx |= tx == 2 * ix + kk - 1
            mask = np.zeros((B, 2 * H, 2 * W), bool)
            mask[b] = my[:, None] & mx[None, :]
            for ch in (k % c0, c0 + k % c1):                 # an element of x0, an element of x1
                xp = x.copy()
                xp[b, iy, ix, ch] = np.nan
                _assert_footprint(run_transpose(lib, *split(xp), w, bias), clean, mask, (b, iy, ix, ch))
    wp = w.copy()
    n = max(co - 2, 0)
    wp[2, 3, n, c0 + c1 - 1] = np.nan
    got = run_transpose(lib, *split(x), wp, bias)
    keep = np.arange(co) != n
    assert np.isnan(got[..., n]).any()
    assert np.array_equal(got[..., keep].view(np.uint32), clean[..., keep].view(np.uint32))
    # the tap (2, 3) is one of the class (odd ty, even tx) only
    assert np.isnan(got[:, 1::2, 0::2, n]).all() and not np.isnan(got[:, 0::2, :, n]).any() and not np.isnan(got[:, :, 1::2, n]).any()


# ---------------------------------------------------------------------------------------------------- every operand's alignment
EVERY_CONV_OPERAND = ("x", "w", "bias", "mean", "var", "beta", "y")
EVERY_TRANSPOSE_OPERAND = ("x0", "x1", "w", "bias", "mean", "var", "beta", "y")


@pytest.mark.parametrize("off", [EVERY_CONV_OPERAND, ("w",), ("y",)], ids=["all", "w", "y"])
@pytest.mark.parametrize("case", [(2, 4, 6, 1, 5), (2, 10, 14, 3, 40)], ids=["valu", "mfma"])
def test_conv2d_bits_do_not_depend_on_any_operands_alignment(lib, case, off):
    x, w, bias = _conv_fixture(case, seed=7)
    bn = _bn(case[4], 8)
    aligned = run_conv(lib, x, w, bias, bn, "lrelu")
    moved = run_conv(lib, x, w, bias, bn, "lrelu", off=off)
    assert np.isfinite(aligned).all() and np.array_equal(aligned.view(np.uint32), moved.view(np.uint32))


@pytest.mark.parametrize("off", [EVERY_TRANSPOSE_OPERAND, ("w",), ("y",)], ids=["all", "w", "y"])
@pytest.mark.parametrize("case", [(1, 4, 8, 3, 5, 1), (2, 5, 7, 3, 2, 40)], ids=["valu", "mfma"])
def test_conv2d_transpose_bits_do_not_depend_on_any_operands_alignment(lib, case, off):
    x, w, bias = _transpose_fixture(case, seed=7)
    c0 = case[3]
    bn = _bn(case[5], 8)
    x0, x1 = np.ascontiguousarray(x[..., :c0]), np.ascontiguousarray(x[..., c0:])
    aligned = run_transpose(lib, x0, x1, w, bias, bn, "relu")
    moved = run_transpose(lib, x0, x1, w, bias, bn, "relu", off=off)
    assert np.isfinite(aligned).all() and np.array_equal(aligned.view(np.uint32), moved.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- non-finite values
SPECIALS = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, -0.0], dtype=np.float32)


def _run_specials(lib, kind, bn, act):
    """Zero weights on a 2 x 2 map, the bias SPECIALS: every output pixel of channel n is the epilogue of SPECIALS[n].
    -> [pixels, 6]"""
    rng = np.random.RandomState(11)
    if kind == "conv-valu" or kind == "conv-mfma":
        ci = 1 if kind == "conv-valu" else 2
        x = rng.randn(1, 2, 2, ci).astype(np.float32)
        return run_conv(lib, x, np.zeros((5, 5, ci, 6), np.float32), SPECIALS, bn, act).reshape(-1, 6)
    x = rng.randn(1, 2, 2, 2).astype(np.float32)
    if kind == "transpose-mfma":
        return run_transpose(lib, x, None, np.zeros((5, 5, 6, 2), np.float32), SPECIALS, bn, act).reshape(-1, 6)
    cols = []                                                # Cout == 1 is what sends the transposed conv to the VALU: a call per value
    for n in range(6):
        one = None if bn is None else [a[n:n + 1] for a in bn]
        cols.append(run_transpose(lib, x, None, np.zeros((5, 5, 1, 2), np.float32), SPECIALS[n:n + 1], one, act).reshape(-1))
    return np.stack(cols, axis=1)


@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("act", [None, "lrelu", "relu", "sigmoid"], ids=["none", "lrelu", "relu", "sigmoid"])
@pytest.mark.parametrize("kind", ["conv-valu", "conv-mfma", "transpose-valu", "transpose-mfma"])
def test_non_finite_values_go_through_the_epilogue(lib, kind, act, with_bn):
    """NaN, +Inf and -Inf at the pre-activation come out as the oracle's epilogue makes them in float32 (torch.relu and TF's ReLU
    propagate NaN; so must the kernels' -- a corrupted checkpoint must not be repaired silently).  Finite values: without batch
    norm the epilogue of these inputs is exact or one rounding (0.2 z), so the float32 oracle's bits; with batch norm or the sigmoid
    the kernel and the float32 oracle each lie within the module docstring's bound (e = 0: the pre-activation is exact) of the
    exact value, so within twice that of each other."""
    bn = _bn(6, 12) if with_bn else None
    got = _run_specials(lib, kind, bn, act)
    z32 = torch.zeros(6, dtype=torch.float32)
    want = ora.epilogue(z32, torch.from_numpy(SPECIALS), None if bn is None else [torch.from_numpy(a) for a in bn], act).numpy()
    assert want.dtype == np.float32 and np.isnan(want[0]) and not np.isnan(want[1:]).any()
    want = np.broadcast_to(want, got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    inf = np.isinf(want)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want[inf])
    fin = np.isfinite(want)
    if bn is None and act != "sigmoid":
        assert np.array_equal(got[fin].view(np.uint32), np.ascontiguousarray(want[fin]).view(np.uint32))
    else:
        with np.errstate(invalid="ignore", over="ignore"):
            _, bound = _epilogue_bound(SPECIALS.astype(np.float64), np.zeros(6), bn, act)
        bound = np.broadcast_to(bound, got.shape)
        assert (np.abs(got[fin].astype(np.float64) - want[fin]) <= 2 * bound[fin]).all()


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
