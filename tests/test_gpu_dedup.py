"""Round 6: a context plan computes every observed conv output ONCE -- the decimated stream of a down level is a slice of the
encoder output, as in the reference (/root/reference/Models/UnetAudioSeparator.py:98-100) -- instead of running a stride-2
conv AND a full-rate conv over the skip window (rounds 1 - 5: the even window positions twice, two summation orders).

* the new plan against the old launch sequence (`WUN_NO_DEDUP=1`) on the same weights / batch: same network -- outputs, loss and
  every gradient agree to fp32 summation order (two roundings of the even window positions in the old plan, one in the new);
* the forward activations the new plan leaves in the workspace: the skip window's even positions hold THE SAME BITS as the
  decimated stream (one value, one rounding);
* every schedule of the odd-window input gradients (`WUN_EARLY_WINDOW` = default (all levels early on the side streams) / deep /
  0 (none early: the non-nested fall-back path, window part after the row-wide part)), both fuse floors and both forms of the
  fused odd-window launch (aligned start with the shifted filter / odd start, `WUN_NO_ODD_ALIGN`) give the same gradients to fp32
  summation order (a + b + c in another order);
* stereo / difference / learned-upsampling heads.

Every case takes its length from get_padding, whose crops are symmetric and whose bottleneck has at least two positions: all
of them have even crop starts and windows of three or more positions.  Odd crop starts, windows with a single position and
levels whose window gradient cannot start early are tests/test_gpu_geometry.py's (tests/_geometry.py: the signature).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import wave_u_net_amd as wun                        # noqa: E402
from wave_u_net_amd import training                 # noqa: E402
from _observed import record                        # noqa: E402

CASES = [
    # (named config, overrides, batch)
    ("m1_context", dict(num_layers=5, num_initial_filters=8, num_frames=300), 3),
    ("m1_context", dict(num_layers=4, num_initial_filters=8, num_frames=70), 2),          # short windows
    ("m1_context", dict(num_layers=6, num_initial_filters=8, num_frames=33, filter_size=9, input_filter_size=9), 2),
    ("full", dict(num_layers=4, num_initial_filters=8, num_frames=210), 2),                # stereo, difference, learned
    ("full_multi_instrument", dict(num_layers=3, num_initial_filters=16, num_frames=500), 2),
    ("m1_context", dict(num_layers=5, num_initial_filters=8, num_frames=301, merge_filter_size=3, filter_size=5, input_filter_size=5), 2),
    ("m1_context", dict(), 2),                                                             # the headline architecture, B = 2
]
TOL = 2e-5      # x max|ref| per tensor: fp32 summation-order differences only (same forward pass, same LeakyReLU branches)
TOL_PLANS = 5e-4  # ... between the two PLANS: the old one rounds the even window positions twice (two summation orders), so a
                  # pre-activation within fp32 rounding of 0 can take the other LeakyReLU branch in one of them -- the flip floor
                  # of DESIGN.md section 2 (GRAD_TOL of tests/test_gpu_parity.py); observed 4.6e-5 on one bias of an 8-filter net.
                  # An indexing error of the parity split / windowed accumulate moves gradients by O(1).


def _run(cfg, batch, env, monkeypatch, want_acts=False):
    for k in ("WUN_NO_DEDUP", "WUN_EARLY_WINDOW", "WUN_ODD_FUSE_MIN", "WUN_NO_ODD_ALIGN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tr = training.Trainer(dict(cfg, batch_size=batch))
    mix, targets = training.synthetic_source(cfg, tr.batch, tr.t_in, tr.t_out, tr.device, seed=11)()
    outs = tr.sep.get_output(mix, True)
    outs = {k: v.detach().cpu().numpy().copy() for k, v in outs.items()}
    acts = None
    if want_acts:
        L = cfg["num_layers"]
        acts = [(tr.sep.activation("skip", i), tr.sep.activation("dec", i)) for i in range(L)]
        acts = [((s[0].cpu().numpy().copy(), s[1], s[2]), (d[0].cpu().numpy().copy(), d[1], d[2])) for s, d in acts]
    loss = float(tr.sep.loss_and_gradients(targets).item())
    grads = {k: v.detach().cpu().numpy().copy() for k, v in tr.sep.gradients().items()}
    info = tr.sep.plan_info()
    flops = (info.fwd_flops + info.bwd_flops, info.fwd_flops_unique + info.bwd_flops_unique)
    return outs, loss, grads, acts, flops


def _close(a, b, tag, tol=TOL):
    worst = 0.0
    for k in a[0]:
        worst = max(worst, np.abs(a[0][k] - b[0][k]).max())
    assert worst <= 5e-6, (tag, "outputs", worst)
    assert abs(a[1] - b[1]) <= 2e-6 * max(1.0, abs(b[1])), (tag, a[1], b[1])
    wg = (0.0, "")
    for k in a[2]:
        scale = max(1e-12, np.abs(b[2][k]).max())
        e = np.abs(a[2][k] - b[2][k]).max() / scale
        if e > wg[0]:
            wg = (e, k)
    assert wg[0] <= tol, (tag, wg)
    return wg[0]


@pytest.mark.parametrize("case", CASES, ids=[c[0] + str(sorted(c[1].items())) for c in CASES])
def test_every_output_once_equals_the_two_launch_plan(case, monkeypatch):
    name, over, batch = case
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = wun.get_config(name, **over)
    new = _run(cfg, batch, {}, monkeypatch, want_acts=True)
    old = _run(cfg, batch, {"WUN_NO_DEDUP": "1"}, monkeypatch)
    e = _close(new, old, "dedup vs rounds 1-5 launch sequence", TOL_PLANS)
    record("dedup_plan_vs_two_launch_plan_gradients", "%s %s" % (name, sorted(over.items())), e, TOL_PLANS)
    # nothing is computed twice any more; the old plan's executed FLOPs exceed its unique FLOPs
    assert new[4][0] == new[4][1] and old[4][0] > old[4][1] and abs(old[4][1] - new[4][1]) <= 1e-6 * new[4][1]
    # one value, one rounding: the window's even ABSOLUTE positions are the decimated stream's elements, bit for bit
    shared = 0
    for (sv, s0, sstep), (dv, d0, dstep) in new[3]:
        assert (sstep, d0, dstep) == (1, 0, 2)
        e0 = s0 + (s0 & 1)
        n_even = len(range(e0, s0 + sv.shape[2], 2))
        if n_even:
            assert np.array_equal(sv[:, :, e0 - s0::2], dv[:, :, e0 // 2:e0 // 2 + n_even])
            shared += n_even
    assert shared > 0


@pytest.mark.parametrize("case", CASES[:4] + CASES[-1:], ids=[c[0] + str(sorted(c[1].items())) for c in CASES[:4] + CASES[-1:]])
def test_every_schedule_of_the_odd_window_gradients_gives_the_same_network(case, monkeypatch):
    name, over, batch = case
    monkeypatch.setenv("WUN_NO_TUNE", "1")
    cfg = wun.get_config(name, **over)
    ref = _run(cfg, batch, {}, monkeypatch)
    worst = 0.0
    for env in ({"WUN_EARLY_WINDOW": "deep"}, {"WUN_EARLY_WINDOW": "0"}, {"WUN_ODD_FUSE_MIN": "256"},
                {"WUN_ODD_FUSE_MIN": "1"}, {"WUN_EARLY_WINDOW": "0", "WUN_ODD_FUSE_MIN": "1"},
                {"WUN_NO_ODD_ALIGN": "1"}, {"WUN_NO_ODD_ALIGN": "1", "WUN_ODD_FUSE_MIN": "1", "WUN_EARLY_WINDOW": "0"}):
        got = _run(cfg, batch, env, monkeypatch)
        worst = max(worst, _close(got, ref, str(env)))
    record("dedup_schedule_modes_gradients", "%s %s" % (name, sorted(over.items())), worst, TOL)
