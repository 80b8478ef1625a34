"""GPU tests of the blend kernels at operator level (include/wun.h: wun_blend_windows, wun_blend_finish)
against the numpy statement tests/_blend_np.py, BIT FOR BIT: the chain of every frame is float32 fused multiply-adds in table
order on both sides, the weights one correctly rounded division, the finish another.

Every case plants -0.0 and denormals in the random normal window rows, starts a window at a negative frame, runs one past
pred_frames, leaves a gap no window covers (+0 there), cuts the table into more than 64 runs (several launches), keeps preds,
den and outputs in poisoned buffers at a chosen offset from a 16-byte boundary (the guard bands must stay untouched) and
delivers the same table as one call and as chunks of 1, 3 and 16 windows (identical bits).  V = Tout - 1 piles dozens of
windows on one frame: far beyond the 4 covering rows one launch takes per run."""
import numpy as np
import pytest
import torch

import _blend_np as bn

from wave_u_net_amd import blend

pytestmark = pytest.mark.gpu
GUARD, POISON = 64, 777.25
S = 2


def _buffer(floats, offset, fill):
    """A poisoned flat device buffer and the view of `floats` floats that starts `offset` floats past a 16-byte boundary,
    GUARD or more floats inside it on either side."""
    flat = torch.full((floats + 2 * GUARD + 8,), POISON, dtype=torch.float32, device="cuda:0")
    k = GUARD + (offset - (flat.data_ptr() // 4 + GUARD)) % 4
    view = flat[k:k + floats]
    assert (view.data_ptr() // 4) % 4 == offset
    view.fill_(fill)
    return flat, view, k


def _guards_intact(flat, k, floats):
    host = flat.cpu().numpy()
    return bool(np.all(host[:k] == POISON) and np.all(host[k + floats:] == POISON))


def _planted(rng, shape):
    x = rng.standard_normal(shape).astype(np.float32)
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, size=24, replace=False)
    flat[idx[0::3]] = np.float32(-0.0)
    flat[idx[1::3]] = np.float32(1e-40)
    flat[idx[2::3]] = np.float32(-3e-39)
    return x


def _case(tout, v):
    """(windows [(pos, row, flags)], pred_frames, gap): two passes of 36 / 71 or more windows (shifts 0 and 3: the second starts at a
    negative frame), one more window wholly to the left but for two frames, and one behind a gap of nine uncovered frames
    that runs three frames past pred_frames."""
    h = tout - v
    n = tout + 70 if h == 1 else 35 * h + tout
    wins = bn.window_list(tout, n, v, [0, 3])
    end = max(p for p, _, _ in wins) + tout
    wins = wins + [(2 - tout, 0, 0), (end + 9, 0, bn.NO_FALL)]
    frames = end + 9 + tout - 3
    wins = [(p, g, f) for g, (p, _, f) in enumerate(wins)]     # every window its own row
    return wins, frames, (end, end + 9)


def _runs(wins, tout, frames):
    """The runs of constant cover the kernel's host side cuts: (count, largest covering set)."""
    edges = sorted({min(max(e, 0), frames) for p, _, _ in wins for e in (p, p + tout)})
    count, deepest = 0, 0
    for a, b in zip(edges[:-1], edges[1:]):
        cover = sum(1 for p, _, _ in wins if p <= a and p + tout >= b)
        count += cover > 0
        deepest = max(deepest, cover)
    return count, deepest


def _deliver(x_dev, wins, v, frames, chan, offset, chunk):
    pf, preds, pk = _buffer(S * frames * chan, offset, 0.0)
    df, den, dk = _buffer(frames, (offset + 2) % 4, 0.0)
    preds3 = preds.view(S, frames, chan)
    tab = np.array(wins, dtype=np.int64)
    for k in range(0, len(wins), chunk or len(wins)):
        blend.blend_windows(x_dev, tab[k:k + (chunk or len(wins))], v, preds3, den)
    acc = preds3.cpu().numpy().copy()
    den_host = den.cpu().numpy().copy()
    blend.blend_finish(preds3, den)
    torch.cuda.synchronize()
    assert _guards_intact(pf, pk, S * frames * chan) and _guards_intact(df, dk, frames)
    assert np.array_equal(den.cpu().numpy().view(np.uint32), den_host.view(np.uint32))      # the finish reads den only
    return acc, den_host, preds3.cpu().numpy()


def _check(tout, v, chan, offset):
    wins, frames, gap = _case(tout, v)
    count, deepest = _runs(wins, tout, frames)
    assert count > 64 and (deepest > 4 if v == tout - 1 else True), (count, deepest)
    rng = np.random.default_rng(1000 * tout + 10 * v + chan)
    x = _planted(rng, (S, len(wins), tout, chan))
    of, x_view, _ = _buffer(x.size, (2 * offset + 1) % 4, 0.0)
    x_dev = x_view.view(x.shape)
    x_dev.copy_(torch.from_numpy(x))
    acc_w = np.zeros((S, frames, chan), np.float32)
    den_w = np.zeros(frames, np.float32)
    bn.accumulate(x, wins, v, acc_w, den_w)
    want = bn.finish(acc_w, den_w)
    acc, den, got = _deliver(x_dev, wins, v, frames, chan, offset, None)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    assert np.array_equal(bits(den), bits(den_w))
    assert np.array_equal(bits(acc), bits(acc_w))
    assert np.array_equal(bits(got), bits(want))
    assert np.all(den[gap[0]:gap[1]] == 0) and np.all(bits(got[:, gap[0]:gap[1]]) == 0)       # uncovered: +0
    assert np.all(den[:gap[0]] > 0) and np.all(den[gap[1]:] > 0)
    for chunk in (1, 3, 16):
        acc_c, den_c, got_c = _deliver(x_dev, wins, v, frames, chan, offset, chunk)
        assert np.array_equal(bits(den_c), bits(den)) and np.array_equal(bits(acc_c), bits(acc)), chunk
        assert np.array_equal(bits(got_c), bits(got)), chunk


CASES = [(tout, v) for tout in (5, 37, 1031) for v in sorted({0, 1, tout // 3, tout - 1})]


@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("tout, v", CASES)
def test_blend_is_the_statement_bit_for_bit(tout, v, chan):
    _check(tout, v, chan, offset=(CASES.index((tout, v)) + chan) % 4)


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("chan", [1, 2])
@pytest.mark.parametrize("tout, v", [(37, 12), (5, 4)])
def test_every_alignment_of_source_and_destination(tout, v, chan, offset):
    """preds at `offset`, den at offset + 2 and outputs at 2 offset + 1 floats past a 16-byte boundary; with an odd Tout and
    odd window positions the rows and runs then start at every one of the four offsets inside a granule, on both sides."""
    _check(tout, v, chan, offset)


def test_refusals_reach_python():
    x = torch.zeros((S, 2, 5, 1), device="cuda:0")
    preds, den = torch.zeros((S, 9, 1), device="cuda:0"), torch.zeros(9, device="cuda:0")
    with pytest.raises(ValueError):
        blend.blend_windows(x, [(0, 2, 0)], 1, preds, den)                 # a row outside [0, B)
    with pytest.raises(ValueError):
        blend.blend_windows(x, [(0, 0, 0)], 5, preds, den)                 # V > Tout - 1
    with pytest.raises(ValueError):
        blend.blend_windows(x, [(0, 0, 0)], 1, preds, den[:8])
    assert bool((preds == 0).all()) and bool((den == 0).all())
