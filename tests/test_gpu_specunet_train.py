"""GPU tests of the spectrogram U-Net's training step (include/wun.h: wun_spec_train_forward, wun_spec_loss_backward,
wun_spec_adam_step, the two weight-gradient operators and wun_op_bn2d_stats) against the float64 oracle
tests/_specunet_train_np.py.

Bounds.  Weight-gradient operators, derived and not measured: an output is a sum of n_red products accumulated in fp32 by some
tree (a chain per chunk of 256 pixels, the chunks in ascending order), so |got - want| <= (n_red + 4) 2^-24 sum |Big| |Small|.
wun_op_bn2d_stats sums in float64, so only the input's and the output's roundings count: 4 * 2^-24 max|z| for the mean,
8 * 2^-24 max|z|^2 for the variance.  The model: DESIGN.md 5.17's rule, 8 x the float32-CPU oracle's own error on that tensor,
floored at 2^-20 max|value| (forward tensors, the loss) or at 2^-20 of the float64 oracle's sum |terms| of the tensor
(gradients: sum |Big| |Small| at the largest output of a kernel, sum |dz| for a bias, sum |g'| for a beta) -- the absolute floor
that makes the mathematically-zero conv-bias gradients under a batch norm testable.  The fixtures' seeds keep every kink of abs,
ReLU and LeakyReLU 64 float32 deviations away (test_specunet_train_host.py)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _specunet_np as ora  # noqa: E402
import _specunet_train_np as tro  # noqa: E402
from _observed import record  # noqa: E402
from _unaligned import _offset_copy  # noqa: E402

import wave_u_net_amd as wun  # noqa: E402
from wave_u_net_amd import _lib, checkpoint, datasets, training, validation  # noqa: E402
from wave_u_net_amd.spectrogram import UnetSpectrogramSeparator  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 64
_CACHE = {}


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _place(name, a, off):
    d = _dev(a)
    return _offset_copy(d) if d is not None and name in off else d


def _guarded(n, fill, off=0):
    """(buffer, view of n floats with GUARD sentinel floats on both sides, `off` floats further in)."""
    buf = torch.full((n + 2 * GUARD + off,), 12345.0, dtype=torch.float32, device="cuda")
    view = buf[GUARD + off:GUARD + off + n]
    view.fill_(fill)
    return buf, view


def _guards_intact(buf, n, off=0):
    b = buf.cpu().numpy()
    return bool((b[:GUARD + off] == 12345.0).all() and (b[GUARD + off + n:] == 12345.0).all())


# ================================================================================================ the weight-gradient operators
# (B, Hs, Ws, Cbig, c0, c1): the small map and the channel counts.  strided: Big = x [B, 2Hs, 2Ws, Cbig], Small = dz [.., c0];
# transposed: Big = dz [B, 2Hs, 2Ws, Cbig = cout], Small = [x0 (c0), x1 (c1)].  Rows of the GEMM: 25 Cbig, columns: c0 + c1,
# reduction: B Hs Ws in chunks of 256.
STRIDED_CASES = [
    (1, 1, 1, 2, 3, 0),       # a 2 x 2 big map: padding taps, a reduction of one pixel
    (1, 3, 5, 3, 5, 0),       # 75 rows: two row tiles, 11 rows in the second; a reduction shorter than one chunk (15)
    (2, 10, 17, 3, 40, 0),    # a reduction of 340: two chunks, 84 in the second; two column tiles, 8 columns in the second
    (1, 6, 7, 2, 70, 0),      # three column tiles, 6 columns in the last; a reduction of 42: two staged steps, 10 in the second
    (2, 4, 6, 1, 5, 0),       # C_big == 1 (the first down layer): VALU
    (1, 4, 6, 4, 1, 0),       # C_small == 1 with C_big > 1: VALU
    (2, 12, 16, 1, 16, 0),    # VALU over several workgroups (400 outputs) and two chunks (384)
    (1, 1, 7, 3, 4, 0),       # a one-row small map
    (1, 6, 1, 3, 4, 0),       # a one-column small map
    (2, 16, 16, 16, 32, 0),   # 400 rows (7 row tiles), a full column tile, exactly two chunks
]
TRANSPOSED_CASES = [
    (1, 1, 1, 2, 3, 0),
    (2, 3, 5, 7, 3, 5),       # both channel ranges; 175 rows: three row tiles
    (2, 10, 17, 3, 17, 23),   # two ranges across a column-tile boundary (40 columns), two chunks
    (1, 4, 8, 1, 3, 5),       # the mask layer: C_big == 1, two ranges, VALU
    (1, 4, 8, 1, 17, 0),      # the mask layer without a skip
    (1, 4, 6, 5, 1, 0),       # C_small == 1
    (1, 1, 5, 4, 2, 2),       # a one-row small map, two ranges
    (1, 5, 1, 4, 3, 0),       # a one-column small map
    (1, 6, 7, 2, 35, 35),     # three column tiles, the ranges meeting inside the second
]


def _wg_operands(case, seed):
    B, Hs, Ws, cb, c0, c1 = case
    rng = np.random.RandomState(seed)
    big = rng.randn(B, 2 * Hs, 2 * Ws, cb).astype(np.float32)
    s0 = rng.randn(B, Hs, Ws, c0).astype(np.float32)
    s1 = rng.randn(B, Hs, Ws, c1).astype(np.float32) if c1 else None
    return big, s0, s1


def run_wgrad(lib, form, big, s0, s1, off=(), scratch_fill=float("nan"), want_db=True):
    """numpy in -> (dw, db) numpy; every output and the scratch sit between guard floats, which are checked."""
    B, Hb, Wb, cb = big.shape
    Hs, Ws, c0 = Hb // 2, Wb // 2, s0.shape[3]
    c1 = 0 if s1 is None else s1.shape[3]
    bd, s0d, s1d = _place("big", big, off), _place("s0", s0, off), _place("s1", s1, off)
    if form == "strided":
        ns = lib.wun_op_conv2d_s2_wgrad_scratch(B, Hb, Wb, cb, c0)
        nw, ndb = 25 * cb * c0, c0
    else:
        ns = lib.wun_op_conv2d_transpose_s2_wgrad_scratch(B, Hs, Ws, c0 + c1, cb)
        nw, ndb = 25 * cb * (c0 + c1), cb
    assert ns > 0
    o = 1 if "out" in off else 0
    sbuf, scratch = _guarded(ns, scratch_fill, 1 if "scratch" in off else 0)
    wbuf, dw = _guarded(nw, float("nan"), o)
    bbuf, db = _guarded(ndb, float("nan"), o)
    if form == "strided":
        _lib.check(lib.wun_op_conv2d_s2_wgrad(bd.data_ptr(), s0d.data_ptr(), dw.data_ptr(), db.data_ptr() if want_db else None,
                                              scratch.data_ptr(), B, Hb, Wb, cb, c0, _stream()))
    else:
        _lib.check(lib.wun_op_conv2d_transpose_s2_wgrad(s0d.data_ptr(), c0, None if s1d is None else s1d.data_ptr(), c1,
                                                        bd.data_ptr(), dw.data_ptr(), db.data_ptr() if want_db else None,
                                                        scratch.data_ptr(), B, Hs, Ws, cb, _stream()))
    torch.cuda.synchronize()
    assert _guards_intact(sbuf, ns, 1 if "scratch" in off else 0) and _guards_intact(wbuf, nw, o) and _guards_intact(bbuf, ndb, o)
    return dw.cpu().numpy().reshape(5, 5, cb, -1), db.cpu().numpy()


def _wg_want(big, s0, s1):
    small = s0 if s1 is None else np.concatenate([s0, s1], axis=3)
    b64, s64 = torch.tensor(big, dtype=torch.float64), torch.tensor(small, dtype=torch.float64)
    return tro.wgrad(b64, s64).numpy(), tro.wgrad(b64.abs(), s64.abs()).numpy()


@pytest.mark.parametrize("form, case", [("strided", c) for c in STRIDED_CASES] + [("transposed", c) for c in TRANSPOSED_CASES],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_wgrad_against_float64(lib, form, case):
    B, Hs, Ws, cb, c0, c1 = case
    big, s0, s1 = _wg_operands(case, 11)
    dw, db = run_wgrad(lib, form, big, s0, s1)
    want, mag = _wg_want(big, s0, s1)
    n_red = B * Hs * Ws
    bound = (n_red + 4) * U * mag
    err = np.abs(dw - want)
    assert np.isfinite(dw).all() and dw.shape == want.shape
    frac = float((err / np.maximum(bound, 1e-300)).max())
    record("test_wgrad_against_float64[%s-%s]" % (form, "x".join(map(str, case))), "fraction of the bound", frac, 1.0)
    assert (err <= bound).all()
    dz = s0 if form == "strided" else big                    # db = sum dz: float64 sums, the rounding of the result
    want_db = dz.astype(np.float64).reshape(-1, dz.shape[3]).sum(0)
    assert (np.abs(db - want_db) <= 4 * U * np.abs(dz).astype(np.float64).reshape(-1, dz.shape[3]).sum(0)).all()


@pytest.mark.parametrize("form, case", [("strided", STRIDED_CASES[2]), ("strided", STRIDED_CASES[6]), ("transposed", TRANSPOSED_CASES[2]),
                                        ("transposed", TRANSPOSED_CASES[3])],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_wgrad_footprint_by_one_nan(lib, form, case):
    """One NaN in Big, then one in Small: exactly the outputs whose sum contains that element are NaN (the oracle's einsum
    propagates a NaN through its zero padding as the kernels' zero operands do)."""
    B, Hs, Ws, cb, c0, c1 = case
    big, s0, s1 = _wg_operands(case, 12)
    rng = np.random.RandomState(5)
    for which in ("big", "small"):
        b2, t0 = big.copy(), s0.copy()
        if which == "big":
            b2[B - 1, rng.randint(2 * Hs), rng.randint(2 * Ws), cb - 1] = np.nan
        else:
            t0[0, rng.randint(Hs), rng.randint(Ws), c0 // 2] = np.nan
        dw, _ = run_wgrad(lib, form, b2, t0, s1)
        want, _ = _wg_want(b2, t0, s1)
        assert np.isnan(want).any() and not np.isnan(want).all()
        assert np.array_equal(np.isnan(dw), np.isnan(want)), which


@pytest.mark.parametrize("form, case", [("strided", STRIDED_CASES[2]), ("strided", STRIDED_CASES[6]), ("transposed", TRANSPOSED_CASES[2]),
                                        ("transposed", TRANSPOSED_CASES[3])],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_wgrad_bits_depend_on_nothing_but_the_operands(lib, form, case):
    big, s0, s1 = _wg_operands(case, 13)
    ref = run_wgrad(lib, form, big, s0, s1)
    same = lambda a: all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, ref))
    assert same(run_wgrad(lib, form, big, s0, s1))                                        # repetition
    assert same(run_wgrad(lib, form, big, s0, s1, scratch_fill=0.0))                      # what the scratch held
    assert same(run_wgrad(lib, form, big, s0, s1, scratch_fill=float("inf")))
    for off in (("big",), ("s0",), ("s1",), ("scratch",), ("out",), ("big", "s0", "s1", "scratch", "out")):
        assert same(run_wgrad(lib, form, big, s0, s1, off=off)), off                      # one float off 8 bytes
    dw, db = run_wgrad(lib, form, big, s0, s1, want_db=False)                             # db is optional and then untouched
    assert np.array_equal(dw.view(np.uint32), ref[0].view(np.uint32)) and np.isnan(db).all()


# ================================================================================================ wun_op_bn2d_stats
# (B, H, W, C)
STATS_CASES = [
    (1, 1, 1, 3),             # n = 1: the variance is 0, and max(n - 1, 1) is what the moving average then divides by
    (1, 1, 1, 1),
    (2, 1, 1, 2),             # n = 2: the deepest batch norm of `five`
    (2, 30, 40, 5),           # n = 2400: three blocks of 1024 pixels, 352 in the last
    (1, 4, 7, 70),            # two channel tiles, 6 channels in the second
    (1, 32, 32, 1),           # one channel: one lane per pixel row
    (3, 5, 7, 16),
]


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn2d_stats_against_float64(lib, case):
    B, H, W, Cc = case
    rng = np.random.RandomState(sum(case))
    z = (rng.randn(B, H, W, Cc) * rng.uniform(0.5, 3.0, Cc) + rng.uniform(-2, 2, Cc)).astype(np.float32)
    ns = lib.wun_op_bn2d_stats_scratch(B, H, W, Cc)
    got = []
    for fill, off in ((float("nan"), 0), (0.0, 1)):
        sbuf, scratch = _guarded(ns, fill, off)
        mbuf, mean = _guarded(Cc, float("nan"), off)
        vbuf, var = _guarded(Cc, float("nan"), off)
        zd = _offset_copy(_dev(z)) if off else _dev(z)
        _lib.check(lib.wun_op_bn2d_stats(zd.data_ptr(), mean.data_ptr(), var.data_ptr(), scratch.data_ptr(), B, H, W, Cc, _stream()))
        torch.cuda.synchronize()
        assert _guards_intact(sbuf, ns, off) and _guards_intact(mbuf, Cc, off) and _guards_intact(vbuf, Cc, off)
        got.append((mean.cpu().numpy(), var.cpu().numpy()))
    z64 = z.astype(np.float64).reshape(-1, Cc)
    zmax = np.abs(z64).max()
    assert (np.abs(got[0][0] - z64.mean(0)) <= 4 * U * zmax).all()
    assert (np.abs(got[0][1] - z64.var(0)) <= 8 * U * zmax ** 2).all()
    if B * H * W == 1:
        assert (got[0][1] == 0.0).all() and np.array_equal(got[0][0], z.reshape(Cc))
    for a, b in zip(got[0], got[1]):                         # scratch contents and alignment do not matter
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ================================================================================================ the model
def _cfg(geo, **kw):
    n_fft, hop, L, nif, F, B = tro.GEOMETRIES[geo]
    base = dict(num_layers=L, num_initial_filters=nif, spec_frame_len=n_fft, spec_hop=hop, num_frames=(F - 1) * hop + n_fft,
                batch_size=B, spec_dropout_seed=tro.DROPOUT_SEED)
    base.update(kw)
    return wun.get_config("unet_spectrogram_l1", **base)


def _separator(geo, fx=None, **kw):
    sep = UnetSpectrogramSeparator(_cfg(geo, **kw), device="cuda:0")
    sep.load_variables((fx or tro.fixture(geo))["variables"])
    return sep


def _forward(sep, fx):
    outs = sep.get_output(torch.from_numpy(fx["mix"][:, :, None]), True, return_spectrogram=True)
    return np.stack([outs[k].cpu().numpy() for k in sep.source_names])


def _masks_of(sep, fx):
    """The dropout multipliers the last training forward used, read back through the accessor."""
    out = {}
    for s in range(2):
        for lv in range(fx["L"] - 1):
            m = sep.activation("dropout", s, lv)
            if m is not None:
                out[(s, lv)] = m.cpu().numpy()
    return out or None


def _oracles(geo, rate):
    """(fixture, masks, float64 and float32 forward, and their (loss, per, grads, floors, diffs)) -- computed once, never changed."""
    key = (geo, rate)
    if key not in _CACHE:
        fx = tro.fixture(geo)
        masks = tro.fixture_masks(fx, rate)
        args = (fx["mix"], fx["variables"], fx["L"], fx["nif"], fx["n_fft"], fx["hop"], masks)
        f64, f32 = tro.train_forward(*args), tro.train_forward(*args, dtype=torch.float32)
        b64 = tro.loss_and_gradients(f64, fx["targets"], fx["n_fft"], fx["hop"])
        b32 = tro.loss_and_gradients(f32, fx["targets"], fx["n_fft"], fx["hop"])
        _CACHE[key] = (fx, masks, f64, f32, b64, b32)
    return _CACHE[key]


def _rule(got, want64, want32, floor_scale=None):
    """DESIGN.md 5.17's rule -> (error, bound)."""
    want64, want32 = np.asarray(want64, np.float64), np.asarray(want32, np.float64)
    stand_in = np.abs(want32 - want64).max()
    scale = np.abs(want64).max() if floor_scale is None else floor_scale
    return float(np.abs(np.asarray(got, np.float64) - want64).max()), max(8.0 * stand_in, 2.0 ** -20 * scale)


@pytest.mark.parametrize("rate", [0.0, 0.5])
@pytest.mark.parametrize("geo", ["skip", "flat", "five"])
def test_training_forward_against_float64(geo, rate):
    fx, masks, f64, f32, _, _ = _oracles(geo, rate)
    sep = _separator(geo, fx, spec_dropout=rate)
    mags = _forward(sep, fx)
    got_masks = _masks_of(sep, fx)
    if masks is None:
        assert got_masks is None
    else:                                                    # the stored masks are wun.h's keep function
        assert set(got_masks) == set(masks)
        for k in masks:
            assert np.array_equal(got_masks[k], masks[k]), k
    name = "test_training_forward_against_float64[%s-%.1f]" % (geo, rate)
    L = fx["L"]
    worst = 0.0
    for s in range(2):
        checks = [("mags", mags[s], f64["mags"][s], f32["mags"][s]),
                  ("mask", sep.activation("act", s, 2 * L - 1).cpu().numpy(), f64["src"][s]["mask"], f32["src"][s]["mask"])]
        for j in range(2 * L - 1):
            for kind, key in (("z", "z"), ("mean", "mean"), ("var", "var"), ("act", "act")):
                checks.append(("%s[%d]" % (kind, j), sep.activation(kind, s, j).cpu().numpy(), f64["src"][s][key][j], f32["src"][s][key][j]))
        for what, got, w64, w32 in checks:
            assert got.shape == tuple(w64.shape), (what, got.shape, tuple(w64.shape))
            err, bound = _rule(got, w64.numpy(), w32.numpy())
            worst = max(worst, err / bound)
            assert np.isfinite(got).all() and err <= bound, (s, what, err, bound)
    record(name, "worst err / bound over the retained tensors", worst, 1.0)


def test_inference_is_untouched_by_a_training_forward():
    fx = tro.fixture("skip")
    sep = _separator("skip", fx)
    x = torch.from_numpy(fx["mix"][:, :, None])
    before = {s: {k: v.cpu().numpy().copy() for k, v in sep.get_output(x, False, return_spectrogram=s).items()} for s in (False, True)}
    p0 = sep.params.cpu().numpy().copy()
    _forward(sep, fx)
    assert np.array_equal(sep.params.cpu().numpy().view(np.uint32), p0.view(np.uint32))   # the forward updates no moving average
    for s in (False, True):
        after = sep.get_output(x, False, return_spectrogram=s)
        for k in after:
            assert np.array_equal(after[k].cpu().numpy().view(np.uint32), before[s][k].view(np.uint32))


@pytest.mark.parametrize("geo", ["skip", "flat", "five", "flat_b1"])
def test_loss_and_gradients_against_float64(geo):
    fx, masks, f64, f32, b64, b32 = _oracles(geo, 0.5)
    sep = _separator(geo, fx)                                # dropout 0.5 (the default) wherever the geometry has a level
    _forward(sep, fx)
    loss = sep.loss_and_gradients(torch.from_numpy(fx["targets"][..., None]))
    losses = sep.last_losses.cpu().numpy()
    name = "test_loss_and_gradients_against_float64[%s]" % geo
    err, bound = _rule(losses[0], float(b64[0]), float(b32[0]))
    record(name, "loss err", err, bound)
    assert err <= bound and float(loss.item()) == float(losses[0])
    for s in range(2):
        err, bound = _rule(losses[1 + s], float(b64[1][s]), float(b32[1][s]))
        assert err <= bound
    grads = sep.gradients()
    worst, worst_bias = 0.0, 0.0
    for k, g64 in b64[2].items():
        got = grads[k].cpu().numpy()
        assert got.shape == tuple(g64.shape), k
        if k.split("/")[-1].startswith("moving"):
            assert (got == 0.0).all(), k
            continue
        err, bound = _rule(got, g64.numpy(), b32[2][k].numpy(), floor_scale=b64[3][k])
        print("[grad] %-44s err %.3e bound %.3e max|g| %.3e floor scale %.3e" % (k, err, bound, float(g64.abs().max()), b64[3][k]))
        if k.endswith("/bias") and float(g64.abs().max()) < 1e-9 * b64[3][k]:          # a conv bias under a batch norm
            worst_bias = max(worst_bias, err / bound)
        worst = max(worst, err / bound)
        assert np.isfinite(got).all() and err <= bound, (k, err, bound)
    record(name, "worst gradient err / bound", worst, 1.0)
    record(name, "worst err / bound of the zero conv-bias gradients", worst_bias, 1.0)


def _ulps(got, want64, *operands):
    """|got - want| in float32 ulps of the largest of |want| and the |operands| the value was formed from: every rounding of a
    sum is relative to its operands, so a result that cancels below them is not held to its own, smaller, ulp."""
    scale = np.abs(np.asarray(want64, np.float64))
    for o in operands:
        scale = np.maximum(scale, np.abs(np.asarray(o, np.float64)))
    ulp = np.spacing(np.maximum(scale.astype(np.float32), np.float32(1e-37))).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want64, np.float64)) / ulp


@pytest.mark.parametrize("geo", ["skip", "flat_b1", "five"])
def test_one_step_updates_as_the_oracle(geo):
    """After adam_step: params, m, v and the moving statistics against the float64 update computed from the GPU's OWN gradients
    and batch statistics, from non-trivial slots at step 7.  theta, m and v within 4 ulp, the moving averages within 2 ulp of
    the stored value.  The ulp of theta, m and v is that of the largest operand of the sum that forms them (theta and the
    update; b m and (1 - b) g): a value that cancels is not held to its own ulp.  The first slot is given the gradient's sign,
    as a run of steps in one direction leaves it, so that m itself -- whose relative error the update inherits -- does not
    cancel."""
    fx = tro.fixture(geo)
    sep = _separator(geo, fx)
    sep.global_step = 6
    _forward(sep, fx)
    sep.loss_and_gradients(torch.from_numpy(fx["targets"][..., None]))
    sep.adam_m.copy_(torch.sign(sep.grads) * torch.from_numpy(np.abs(np.random.RandomState(1).randn(sep.num_params)).astype(np.float32) * 1e-3).cuda())
    sep.adam_v.copy_(torch.from_numpy(np.random.RandomState(2).rand(sep.num_params).astype(np.float32) * 1e-6))
    p0, m0, v0, g = (t.cpu().numpy().astype(np.float64) for t in (sep.params, sep.adam_m, sep.adam_v, sep.grads))
    L, B, F, W0 = fx["L"], fx["B"], fx["F"], fx["n_fft"] // 2
    stats = {}
    for s in range(2):
        down, up = tro.names(L, s)
        for j in range(2 * L - 1):
            stem = down[j][1] if j < L else up[j - L][1]
            sh = j + 1 if j < L else 2 * L - 1 - j
            stats[stem] = (sep.activation("mean", s, j).cpu().numpy().astype(np.float64),
                           sep.activation("var", s, j).cpu().numpy().astype(np.float64), B * (F >> sh) * (W0 >> sh))
    lr, b1, b2, eps = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))
    sep.adam_step(lr)
    assert sep.global_step == 7
    p1, m1, v1 = (t.cpu().numpy() for t in (sep.params, sep.adam_m, sep.adam_v))
    decay = float(np.float32(0.999))
    worst = {"theta": 0.0, "m": 0.0, "v": 0.0, "moving": 0.0}
    for name, off, shp in sep.variable_table():
        sl = slice(off, off + int(np.prod(shp)))
        leaf = name.split("/")[-1]
        if leaf.startswith("moving"):
            mu, var, n = stats[name.rsplit("/", 1)[0]]
            want = tro.moving_average(p0[sl], mu if leaf == "moving_mean" else tro.unbiased(var, n), decay)
            worst["moving"] = max(worst["moving"], float(_ulps(p1[sl], want).max()))
            assert (g[sl] == 0).all()                        # no gradient, and the slots are left alone
            assert np.array_equal(m1[sl].astype(np.float64), m0[sl]) and np.array_equal(v1[sl].astype(np.float64), v0[sl])
        else:
            t, m, v = tro.adam(p0[sl], g[sl], m0[sl], v0[sl], 7, lr, b1, b2, eps)
            worst["theta"] = max(worst["theta"], float(_ulps(p1[sl], t, p0[sl], t - p0[sl]).max()))
            worst["m"] = max(worst["m"], float(_ulps(m1[sl], m, b1 * m0[sl], (1 - b1) * g[sl]).max()))
            worst["v"] = max(worst["v"], float(_ulps(v1[sl], v).max()))
    for k, v in worst.items():
        record("test_one_step_updates_as_the_oracle[%s]" % geo, k + " ulps", v, 2.0 if k == "moving" else 4.0)
    assert worst["theta"] <= 4 and worst["m"] <= 4 and worst["v"] <= 4 and worst["moving"] <= 2
    if geo == "flat_b1":                                     # n = 16 at the only batch norm: the factor 16 / 15 is in the update
        mu, var, n = stats["separator/BatchNorm"]
        assert n == 16
        sl = [slice(o, o + 3) for nm, o, _ in sep.variable_table() if nm == "separator/BatchNorm/moving_variance"][0]
        plain = tro.moving_average(p0[sl], var, decay)
        assert (np.abs(p1[sl] - plain) > 8 * np.spacing(np.float32(1.0))).any()


def test_moving_statistics_keep_zero_slots():
    """grads, m and v of the moving statistics stay 0 through a step from the initial state."""
    fx = tro.fixture("skip")
    sep = _separator("skip", fx)
    for _ in range(2):
        _forward(sep, fx)
        sep.loss_and_gradients(torch.from_numpy(fx["targets"][..., None]))
        sep.adam_step(1e-3)
    g, m, v = (t.cpu().numpy() for t in (sep.grads, sep.adam_m, sep.adam_v))
    moved = 0
    for name, off, shp in sep.variable_table():
        sl = slice(off, off + int(np.prod(shp)))
        if name.split("/")[-1].startswith("moving"):
            assert (g[sl] == 0).all() and (m[sl] == 0).all() and (v[sl] == 0).all(), name
            moved += int((sep.params[sl].cpu().numpy() != fx["variables"][name]).any())
        else:
            assert (v[sl] >= 0).all()
    assert moved == 2 * 2 * 3                                # every moving mean and variance of both sources was updated


# ------------------------------------------------------------------------------------------------ dropout
def test_dropout_masks():
    fx = tro.fixture("five")
    sep = _separator("five", fx)
    L = fx["L"]

    def masks():
        _forward(sep, fx)
        return {(s, lv): (None if sep.activation("dropout", s, lv) is None else sep.activation("dropout", s, lv).cpu().numpy().copy())
                for s in range(2) for lv in range(L - 1)}

    a = masks()
    assert all(a[(s, 3)] is None for s in range(2))                               # levels i >= 3 have none
    shapes = tro.dropout_shapes(fx)
    for s in range(2):
        for lv in range(3):
            assert a[(s, lv)].shape == shapes[lv] and set(np.unique(a[(s, lv)])) == {0.0, 2.0}
    assert not np.array_equal(a[(0, 2)], a[(1, 2)])                               # source
    assert not np.array_equal(a[(0, 0)].ravel()[:64], a[(0, 1)].ravel()[:64])     # level
    b = masks()
    assert all(np.array_equal(a[k], b[k]) for k in a if a[k] is not None)         # equal arguments repeat
    sep.global_step = 1
    c = masks()
    assert all(not np.array_equal(a[k], c[k]) for k in a if a[k] is not None)     # step
    assert np.array_equal(c[(1, 1)], tro.dropout_multipliers(tro.DROPOUT_SEED, 1, 1, 1, shapes[1], 0.5))
    other = _separator("five", fx, spec_dropout_seed=7)
    _forward(other, fx)
    assert not np.array_equal(other.activation("dropout", 0, 0).cpu().numpy(), a[(0, 0)])   # seed


def test_rate_zero_gives_the_no_dropout_bits(lib):
    """At rate 0 nothing is materialised: the mask layer of `skip` is the inference kernel on the two retained channel ranges,
    bit for bit -- and the accessor shows no mask."""
    fx = tro.fixture("skip")
    sep = _separator("skip", fx, spec_dropout=0.0)
    _forward(sep, fx)
    assert sep.activation("dropout", 0, 0) is None
    for s in range(2):
        x0, x1 = sep.activation("act", s, 0).contiguous(), sep.activation("act", s, 2).contiguous()
        v = sep.variables()
        stem = tro.names(2, s)[1][1][0]
        y = torch.full((fx["B"], fx["F"], 32, 1), float("nan"), dtype=torch.float32, device="cuda")
        _lib.check(lib.wun_op_conv2d_transpose_s2(x0.data_ptr(), 3, x1.data_ptr(), 3, v[stem + "/kernel"].data_ptr(),
                                                  v[stem + "/bias"].data_ptr(), None, None, None, y.data_ptr(), fx["B"], 4, 16, 1, 3, _stream()))
        torch.cuda.synchronize()
        assert np.array_equal(y[..., 0].cpu().numpy().view(np.uint32), sep.activation("act", s, 3).cpu().numpy().view(np.uint32))


# ------------------------------------------------------------------------------------------------ independence
def _three_steps(sep, fx, stream=None):
    x, tg = torch.from_numpy(fx["mix"][:, :, None]).cuda(), torch.from_numpy(fx["targets"][..., None]).cuda()
    out = []
    with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
        for _ in range(3):
            mags = sep.get_output(x, True, return_spectrogram=True)
            loss = sep.loss_and_gradients(tg)
            out.append([torch.stack([mags[k] for k in sep.source_names]).clone(), sep.last_losses.clone(), sep.grads.clone()])
            sep.adam_step(1e-3)
        out.append([sep.params.clone(), sep.adam_m.clone(), sep.adam_v.clone()])
    torch.cuda.synchronize()
    return [[t.cpu().numpy() for t in row] for row in out]


def _same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for ra, rb in zip(a, b) for x, y in zip(ra, rb))


@pytest.mark.parametrize("geo", ["skip", "five"])
def test_step_bits_depend_on_nothing_but_the_inputs(geo):
    """Two fresh separators over three steps; then a NaN-filled against a zeroed workspace with guard floats around the
    workspace, grads and mags, every buffer one float off 16 bytes, on a side stream."""
    fx = tro.fixture(geo)
    ref = _three_steps(_separator(geo, fx), fx)
    assert all(np.isfinite(t).all() for row in ref for t in row)
    assert _same_bits(ref, _three_steps(_separator(geo, fx), fx))
    B, T, S, K = fx["B"], fx["T"], 2, fx["n_fft"] // 2 + 1
    for fill in (float("nan"), 0.0):
        sep = _separator(geo, fx)
        sep._ensure_variables()
        n = int(sep._lib.wun_spec_train_workspace_floats(C.byref(sep._scfg), B, T))
        wbuf, sep._tws[(B, T)] = _guarded(n, fill, 1)
        gbuf, sep.grads = _guarded(sep.num_params, fill, 1)
        obuf, out = _guarded(S * B * fx["F"] * K, fill, 1)
        sep._outs[(B, T, True)] = out.view(S, B, fx["F"], K)
        sep.params, sep.adam_m, sep.adam_v = (_offset_copy(t) for t in (sep.params, sep.adam_m, sep.adam_v))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        got = _three_steps(sep, fx, side)
        assert _same_bits(ref, got), fill
        assert _guards_intact(wbuf, n, 1) and _guards_intact(gbuf, sep.num_params, 1) and _guards_intact(obuf, S * B * fx["F"] * K, 1)
        assert all(t.data_ptr() % 8 == 4 for t in (sep._tws[(B, T)], sep.grads, out, sep.params, sep.adam_m, sep.adam_v))


def test_unaligned_inputs_give_the_same_bits():
    fx = tro.fixture("skip")
    a, b = _separator("skip", fx), _separator("skip", fx)
    x, tg = torch.from_numpy(fx["mix"][:, :, None]).cuda(), torch.from_numpy(fx["targets"][..., None]).cuda()
    res = []
    for sep, xx, tt in ((a, x, tg), (b, _offset_copy(x), _offset_copy(tg))):
        sep.get_output(xx, True, return_spectrogram=True)
        sep.loss_and_gradients(tt)
        res.append((sep.last_losses.cpu().numpy(), sep.grads.cpu().numpy()))
    assert _same_bits([res[0]], [res[1]])


# ------------------------------------------------------------------------------------------------ it learns
def test_it_learns():
    """200 steps on one fixed batch of `skip` at lr 1e-3 without dropout: the loss falls below half its first value.  The float32
    CPU restatement of the same steps (tests/_specunet_train_np.py::learn_fixture) goes from 0.9679 to 0.1985."""
    fx = tro.learn_fixture()
    sep = _separator("skip", fx, spec_dropout=0.0)
    x, tg = torch.from_numpy(fx["mix"][:, :, None]).cuda(), torch.from_numpy(fx["targets"][..., None]).cuda()
    losses = []
    for _ in range(200):
        sep.get_output(x, True, return_spectrogram=True)
        losses.append(sep.loss_and_gradients(tg))
        sep.adam_step(1e-3)
    first, last = float(losses[0].item()), float(losses[-1].item())
    record("test_it_learns", "loss at step 199 / loss at step 0", last / first, 0.5)
    assert abs(first - 0.9679) < 1e-3 and np.isfinite(last) and last < 0.5 * first
    assert sep.global_step == 200


# ------------------------------------------------------------------------------------------------ the public path
def _batch_source(cfg, fx):
    x = torch.from_numpy(fx["mix"][:, :, None]).cuda()
    tg = torch.from_numpy(fx["targets"][..., None]).cuda()
    return lambda: (x, tg)


@pytest.mark.parametrize("fmt", ["npz", "tf"])
def test_train_writes_a_log_and_a_checkpoint_and_resumes(tmp_path, fmt):
    """training.train on the magnitude objective: the test that fails without the feature."""
    fx = tro.fixture("skip")
    cfg = _cfg("skip", epoch_it=3, log_dir=str(tmp_path / "logs"), model_base_dir=str(tmp_path / "ck"), checkpoint_format=fmt)
    src = _batch_source(cfg, fx)
    path = training.train(cfg, "exp", batch_source=src)
    lines = [json.loads(ln) for ln in open(os.path.join(cfg["log_dir"], "exp", "train.jsonl"))]
    assert [ln["global_step"] for ln in lines] == [1, 2, 3] and all(np.isfinite(ln["sep_loss"]) for ln in lines)
    assert lines[2]["sep_loss"] < lines[0]["sep_loss"]
    assert os.path.exists(path if fmt == "npz" else path + ".index")
    # five steps in one go == three, a checkpoint, two more: parameters, both Adam slots and global_step resume with equal bits
    whole = training.train(dict(cfg, epoch_it=5, model_base_dir=str(tmp_path / "ck5"), log_dir=str(tmp_path / "logs5")), "exp", batch_source=src)
    resumed = training.train(dict(cfg, epoch_it=2), "exp", load_model=path, batch_source=src)
    a, b = UnetSpectrogramSeparator(cfg, device="cuda:0"), UnetSpectrogramSeparator(cfg, device="cuda:0")
    assert checkpoint.load_checkpoint(a, whole) == 5 == checkpoint.load_checkpoint(b, resumed)
    for t in ("params", "adam_m", "adam_v"):
        assert np.array_equal(getattr(a, t).cpu().numpy().view(np.uint32), getattr(b, t).cpu().numpy().view(np.uint32)), t
    assert float(a.adam_v.abs().max()) > 0
    # validation.test scores the result on magnitudes
    rng = np.random.default_rng(3)
    tracks = [datasets.make_track({k: rng.uniform(-0.3, 0.3, (n, 1)).astype(np.float32) for k in cfg["source_names"]}, cfg)
              for n in (900, 1200)]
    loss = validation.test(dict(cfg, num_snippets_per_track=3, cache_size=4), "valid", "exp", resumed, tracks=tracks)
    assert np.isfinite(loss) and loss > 0


def test_cli_trains_the_l1_config(tmp_path):
    """python -m wave_u_net_amd train with cfg.unet_spectrogram_l1 ... as a child process, with small overrides."""
    n_fft, hop, L, nif, F, B = tro.GEOMETRIES["skip"]
    cmd = [sys.executable, "-m", "wave_u_net_amd", "train", "with", "cfg.unet_spectrogram_l1", "synthetic=1", "experiment_id=7",
           "model_config.num_layers=%d" % L, "model_config.num_initial_filters=%d" % nif, "model_config.spec_frame_len=%d" % n_fft,
           "model_config.spec_hop=%d" % hop, "model_config.num_frames=%d" % ((F - 1) * hop + n_fft), "model_config.batch_size=%d" % B,
           "model_config.epoch_it=2", "model_config.log_dir=%s" % (tmp_path / "logs"), "model_config.model_base_dir=%s" % (tmp_path / "ck")]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Saved model at" in r.stdout and os.path.exists(str(tmp_path / "ck" / "7" / "7-2.npz"))
    lines = [json.loads(ln) for ln in open(str(tmp_path / "logs" / "7" / "train.jsonl"))]
    assert [ln["global_step"] for ln in lines] == [1, 2]
    # the raw-audio config is still refused, in plain words
    r = subprocess.run(cmd[:5] + ["cfg.unet_spectrogram"] + cmd[6:], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "inference only" in r.stderr
