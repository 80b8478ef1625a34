"""GPU tests of the polyphase resampler kernel (include/wun.h: wun_resample; wave-u-net_amd/csrc/wun_resample.hip) against
the float64 oracle scipy.signal.resample_poly, and of the bit-exactness it owes (copy at up == down, channel duplication,
downmix, independence of the output offset, nothing written outside the requested frames)."""
import functools

import numpy as np
import pytest
import torch
from scipy.signal import firwin, resample_poly

from wave_u_net_amd import resample as rs

pytestmark = pytest.mark.gpu

RATES = [(44100, 22050), (22050, 44100), (48000, 22050), (44100, 8192)]
CHANNELS = [(1, 1), (2, 2), (2, 1), (1, 2)]
LENGTHS = [1, 40, 41, 4099, 149822]
SENTINEL = 12345.0


@functools.lru_cache(maxsize=None)
def _abs_filter(up, down):
    """|h| of the design WITHOUT the factor `up`: scipy multiplies an array window by up itself."""
    mx = max(up, down)
    return np.abs(firwin(20 * mx + 1, 1.0 / mx, window=("kaiser", 5.0)))


def _map_channels(x, c_out):
    """The kernel's channel mapping in fp32 on the host: per channel, (x0 + x1) / 2, or duplicate."""
    if x.shape[1] == c_out:
        return x
    if c_out == 1:
        return ((x[:, 0] + x[:, 1]) / np.float32(2))[:, None]
    return np.tile(x, [1, 2])


def _run(x, c_out, up, down, y_offset=0, n_out=None, tail=0):
    """wun_resample into a sentinel-filled [y_offset + n_out + tail, c_out] buffer; returns the whole buffer."""
    xd = torch.from_numpy(x).cuda()
    n_out = rs.frames(x.shape[0], up, down) if n_out is None else n_out
    y = torch.full((y_offset + n_out + tail, c_out), SENTINEL, dtype=torch.float32, device="cuda")
    rs.resample_into(xd, y, y_offset, n_out, up, down)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("c_in,c_out", CHANNELS)
@pytest.mark.parametrize("rates", RATES)
def test_kernel_against_float64_oracle(rates, c_in, c_out, n):
    """|y - y64| <= (K + 2) 2^-24 (|h| * |v|)[n] + 2^-24 |y64[n]|: the bound of a length-K fp32 dot product accumulated in
    any order plus the rounding of the fp32 taps (K = taps per output row); (|h| * |v|) from the same scipy call."""
    up, down = rs.ratio(*rates)
    K = rs.design(up, down).shape[1]
    x = np.random.default_rng(n * 7 + c_in).uniform(-1, 1, (n, c_in)).astype(np.float32)
    got = _run(x, c_out, up, down)
    v = _map_channels(x, c_out).astype(np.float64)
    y64 = resample_poly(v, up, down, axis=0)
    mag = resample_poly(np.abs(v), up, down, axis=0, window=_abs_filter(up, down))
    assert got.shape == y64.shape == (rs.frames(n, up, down), c_out)
    bound = (K + 2) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(y64)
    err = np.abs(got.astype(np.float64) - y64)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("%d -> %d Hz, %d -> %d ch, n = %d: max err %.3g, worst err / bound %.3f" % (rates[0], rates[1], c_in, c_out, n, err.max(), worst))
    assert np.all(err <= bound), worst


@pytest.mark.parametrize("c_in,c_out", CHANNELS)
def test_equal_rates_copy_the_channel_mapped_input(c_in, c_out):
    x = np.random.default_rng(c_in + 2 * c_out).uniform(-1, 1, (4099, c_in)).astype(np.float32)
    got = _run(x, c_out, 1, 1, y_offset=3, tail=5)
    assert np.array_equal(got[3:3 + 4099], _map_channels(x, c_out))
    assert np.all(got[:3] == SENTINEL) and np.all(got[3 + 4099:] == SENTINEL)
    # through the public entry: the same rate in and out
    assert np.array_equal(rs.resample(torch.from_numpy(x).cuda(), 22050, 22050).cpu().numpy(), x)


@pytest.mark.parametrize("rates", RATES)
def test_duplication_and_downmix_are_exact(rates):
    up, down = rs.ratio(*rates)
    x = np.random.default_rng(11).uniform(-1, 1, (4099, 2)).astype(np.float32)
    mono = _run(x[:, :1].copy(), 1, up, down)
    dup = _run(x[:, :1].copy(), 2, up, down)
    assert np.array_equal(dup[:, 0], mono[:, 0]) and np.array_equal(dup[:, 1], mono[:, 0])
    mean = ((x[:, 0] + x[:, 1]) / np.float32(2))[:, None]                      # fp32 on the host
    assert np.array_equal(_run(x, 1, up, down), _run(mean, 1, up, down))
    # the two channels of 2 -> 2 are the two 1 -> 1 results
    both = _run(x, 2, up, down)
    assert np.array_equal(both[:, 0], mono[:, 0])
    assert np.array_equal(both[:, 1], _run(x[:, 1:].copy(), 1, up, down)[:, 0])


@pytest.mark.parametrize("c_in,c_out", CHANNELS)
@pytest.mark.parametrize("rates", RATES)
def test_result_does_not_depend_on_the_output_offset(rates, c_in, c_out):
    up, down = rs.ratio(*rates)
    n = 40000
    x = np.random.default_rng(4).uniform(-1, 1, (n, c_in)).astype(np.float32)
    n_out = rs.frames(n, up, down)
    at0 = _run(x, c_out, up, down, y_offset=0, tail=9)
    at_odd = _run(x, c_out, up, down, y_offset=65527, tail=9)
    assert np.array_equal(at0[:n_out], at_odd[65527:65527 + n_out])
    assert np.all(at0[n_out:] == SENTINEL)
    assert np.all(at_odd[:65527] == SENTINEL) and np.all(at_odd[65527 + n_out:] == SENTINEL)
    # a capped n_out is a prefix of the full result
    cap = n_out - 123
    capped = _run(x, c_out, up, down, y_offset=5, n_out=cap, tail=200)
    assert np.array_equal(capped[5:5 + cap], at0[:cap]) and np.all(capped[5 + cap:] == SENTINEL)
    # and it is the same from run to run
    assert np.array_equal(_run(x, c_out, up, down, tail=9), at0)


def test_resample_entry_on_gpu_tensors():
    x = np.random.default_rng(8).uniform(-1, 1, (4099, 2)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    y = rs.resample(xd, 44100, 22050)
    assert y.is_cuda and y.shape == (2050, 2)
    assert np.array_equal(y.cpu().numpy(), _run(x, 2, 1, 2))
    # numpy in, device named: uploaded, kernel, downloaded
    via = rs.resample(x, 44100, 22050, device="cuda:0")
    assert isinstance(via, np.ndarray) and np.array_equal(via, y.cpu().numpy())
    assert rs.resample(xd[:, 0].contiguous(), 44100, 22050).shape == (2050,)
    with pytest.raises(ValueError):
        rs.resample_into(xd, torch.empty((10, 2), device="cuda"), 0, 11, 1, 2)          # does not fit y
