"""Host tests of the single-operator entry points of the elementwise family (include/wun.h: wun_op_upsample,
wun_op_upsample_backward, wun_op_head_*, wun_op_btc_to_ncw, wun_op_set_conv_upsample, wun_op_conv1d_upsample_adjoint,
wun_op_last_path) and of the references the GPU tests compare them with (tests/_elementwise_np.py):
  * every argument error returns before any GPU work (fake pointers, no device needed), struct size and bindings;
  * the references against the oracle's whole network (wt.get_output / wt.train_step) on one small config each of
    linear/same, linear/context, learned/same, learned/context;
  * SENSITIVITY: mutant references miss the true ones by more than the bounds tests/test_gpu_elementwise.py asserts, on every
    case of that file they apply to -- with the coverage assertions there, the evidence that those tests can fail."""
import ctypes as C

import numpy as np
import pytest
import torch

import _elementwise_np as E
from oracle import shapes, waveunet_torch as wt
from wave_u_net_amd import _lib

_FAKE = C.c_void_p(0x1000)          # non-null, 16-byte aligned, never dereferenced: every call below fails a check first
INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_struct_and_binding(lib):
    assert lib.wun_op_head_abi_size() == C.sizeof(_lib.WunOpHeadDesc) == 17 * 4
    assert lib.wun_op_last_path(99) == INVALID
    for op in range(7):
        assert lib.wun_op_last_path(op) in range(10)               # (PATH_NONE until this thread launches the operator)


def test_upsample_argument_errors_without_a_device(lib):
    def up(x=_FAKE, y=_FAKE, w=None, B=2, Cn=3, n=5, tup=10, xp=8, yp=12, bf=0):
        return lib.wun_op_upsample(x, y, w, B, Cn, n, tup, xp, yp, bf, None)

    def bwd(dy=_FAKE, x=_FAKE, dz=_FAKE, w=None, dw=None, part=None, B=2, Cn=3, n=5, tup=10, yp=12, xp=8, bf=0, acc=0):
        return lib.wun_op_upsample_backward(dy, x, dz, w, dw, part, B, Cn, n, tup, yp, xp, bf, acc, None)

    for f in (up, bwd):
        for kw in ({"x": None}, {"B": 0}, {"Cn": 0}, {"n": 0}, {"tup": 8}, {"tup": 11}, {"tup": 12}, {"xp": 4}, {"yp": 9},
                   {"tup": 9, "yp": 8}, {"n": 1, "tup": 3}):
            assert f(**kw) == INVALID, (f.__name__, kw)
            assert lib.wun_last_error()
    assert up(y=None) == INVALID
    assert bwd(dy=None) == INVALID and bwd(dz=None) == INVALID
    assert bwd(dw=_FAKE) == INVALID                                  # dw without w


def _desc(**over):
    d = dict(C=2, F=3, S=3, difference=1, Ko=3, padl=1, Tfeat=9, Tout=9, B=2, tanh=1, training=1, feat_bf16=0,
             mix_pitch=16, feat_pitch=12, dpre_pitch=12, mix_off_feat=2, mix_off_diff=3)
    d.update(over)
    return _lib.WunOpHeadDesc(**d)


HEAD_BAD = [{"C": 0}, {"C": 3}, {"S": 1}, {"S": 6}, {"S": 5, "difference": 0}, {"difference": 2}, {"F": 0}, {"Ko": 0},
            {"padl": -1}, {"padl": 3}, {"Tfeat": 0}, {"Tout": 0}, {"B": 0}, {"feat_pitch": 8}, {"dpre_pitch": 8},
            {"F": 4000, "Ko": 3}]                                    # the last: 4 * 2 * (3 * 4002 * 2 + 2) floats exceed the LDS


def test_head_argument_errors_without_a_device(lib):
    hoff = (C.c_int64 * 4)(0, 40, 80, 120)
    neg = (C.c_int64 * 4)(0, -1, 0, 0)

    def fwd(d=None, mix=_FAKE, feat=_FAKE, par=_FAKE, ho=hoff, out=_FAKE):
        return lib.wun_op_head_forward(C.byref(d) if d is not None else None, mix, feat, par, ho, out, None)

    def lossb(d=None, feat=_FAKE, par=_FAKE, ho=hoff, out=_FAKE, tgt=_FAKE, dpre=_FAKE, dzf=_FAKE, loss=_FAKE):
        return lib.wun_op_head_loss_backward(C.byref(d) if d is not None else None, feat, par, ho, out, tgt, dpre, dzf, loss, None)

    def gradb(d=None, feat=_FAKE, par=_FAKE, ho=hoff, out=_FAKE, dout=_FAKE, dpre=_FAKE, dzf=_FAKE):
        return lib.wun_op_head_backward(C.byref(d) if d is not None else None, feat, par, ho, out, dout, dpre, dzf, None)

    for f in (fwd, lossb, gradb):
        assert f(d=None) == INVALID, f.__name__
        for bad in HEAD_BAD:
            assert f(d=_desc(**bad)) == INVALID, (f.__name__, bad)
        for kw in ({"feat": None}, {"par": None}, {"ho": None}, {"out": None}, {"ho": neg}):
            assert f(d=_desc(), **kw) == INVALID, (f.__name__, kw)
    for bad in ({"mix_pitch": 10}, {"mix_off_feat": -1}, {"mix_off_diff": -1}, {"mix_off_diff": 8}):
        assert fwd(d=_desc(**bad)) == INVALID, bad                   # the mix row is read by the forward entry only
    assert fwd(d=_desc(), mix=None) == INVALID
    for kw in ({"tgt": None}, {"dpre": None}, {"dzf": None}, {"loss": None}):
        assert lossb(d=_desc(), **kw) == INVALID, kw
    for kw in ({"dout": None}, {"dpre": None}, {"dzf": None}):
        assert gradb(d=_desc(), **kw) == INVALID, kw


def test_layout_and_fused_argument_errors_without_a_device(lib):
    def btc(src=_FAKE, dst=_FAKE, B=2, T=5, Cn=3, pitch=8):
        return lib.wun_op_btc_to_ncw(src, dst, B, T, Cn, pitch, None)

    for kw in ({"src": None}, {"dst": None}, {"B": 0}, {"T": 0}, {"Cn": 0}, {"pitch": 4}):
        assert btc(**kw) == INVALID, kw

    assert lib.wun_op_set_conv_upsample(_FAKE, 8, 10, None) == INVALID           # pitch below length
    assert lib.wun_op_set_conv_upsample(_FAKE, 8, 0, None) == INVALID
    try:
        def ex(t_out=5, stride=1, ostride=1, ooff=0, acc=0, mask=None, t_y=5):
            return lib.wun_op_conv1d_ex(_FAKE, 16, None, 0, _FAKE, None, _FAKE, mask, 2, 8, 5, 9, t_out, t_y, stride, 0, 1, acc,
                                        ostride, ooff, None)
        assert lib.wun_op_set_conv_upsample(_FAKE, 12, 10, None) == 0
        for kw in ({"t_out": 4}, {"t_out": 6, "t_y": 6}, {"ostride": 2, "t_y": 10}, {"ooff": 1, "t_y": 6}, {"acc": 1},
                   {"mask": _FAKE}):
            assert ex(**kw) == INVALID, kw                           # ups_tup is neither 2 t_out - 1 nor 2 t_out; not a plain launch
        assert lib.wun_op_set_conv_upsample(C.c_void_p(0x1004), 12, 10, None) == 0
        assert ex() == INVALID                                       # the upsampled copy must be 16-byte aligned
    finally:
        assert lib.wun_op_set_conv_upsample(None, 0, 0, None) == 0

    def adj(dz=_FAKE, wt_=_FAKE, dsk=_FAKE, dup=_FAKE, dzp=_FAKE, xp=_FAKE, B=2, cin=16, nsk=3, ncur=5, k=5, t_in=14, tup=10,
            pad=0, n=5, pp=8):
        return lib.wun_op_conv1d_upsample_adjoint(dz, wt_, dsk, dup, dzp, xp, B, cin, nsk, ncur, k, t_in, tup, pad, n, pp, None)

    for kw in ({"dz": None}, {"wt_": None}, {"dsk": None}, {"dup": None}, {"dzp": None}, {"xp": None}, {"B": 0}, {"cin": 0},
               {"nsk": 0}, {"ncur": 0}, {"k": 0}, {"t_in": 0}, {"n": 0}, {"tup": 8}, {"tup": 11}, {"pp": 4}):
        assert adj(**kw) == INVALID, kw


# ---------------------------------------------------------------------------------------------------------------------------
# the references against the oracle's whole network
# ---------------------------------------------------------------------------------------------------------------------------
NET_CASES = {
    "linear_same": dict(upsampling="linear", context=False, output_type="direct", output_activation="tanh", mono_downmix=True,
                        task="voice", output_filter_size=1),
    "linear_context": dict(upsampling="linear", context=True, output_type="difference", output_activation="linear",
                           mono_downmix=False, task="voice", output_filter_size=3),
    "learned_same": dict(upsampling="learned", context=False, output_type="difference", output_activation="tanh",
                         mono_downmix=False, task="multi_instrument", output_filter_size=3),
    "learned_context": dict(upsampling="learned", context=True, output_type="direct", output_activation="linear",
                            mono_downmix=True, task="multi_instrument", output_filter_size=1),
}


def _wgrad(inp, dz, K, same):
    """dL/dW [K][Cin][Cout] of conv1d_tf(inp, W) for the output gradient dz."""
    W = torch.zeros(K, inp.shape[1], dz.shape[1], dtype=torch.float64, requires_grad=True)
    (wt.conv1d_tf(inp, W, None, same) * dz).sum().backward()
    return W.grad.numpy()


def _dgrad(inp, W, dz, same):
    x = inp.clone().requires_grad_(True)
    (wt.conv1d_tf(x, W, None, same) * dz).sum().backward()
    return x.grad.numpy()


@pytest.mark.parametrize("name", sorted(NET_CASES))
def test_references_against_the_oracle_network(name):
    """One-level network: down0 -> bottleneck -> 2x upsampling -> up conv -> head.  The upsampling reference fed the oracle's
    bottleneck gives the oracle's up-conv output; the head reference fed the oracle's feature map gives its outputs and loss;
    chained backwards (head -> up conv's input gradient -> upsampling adjoint) they give the oracle's gradients of the head
    kernels, the interpolation weights and the bottleneck kernel."""
    cfg = shapes.finalize_config(dict(shapes.BASE_MODEL_CONFIG, num_layers=1, num_initial_filters=3, filter_size=5,
                                      merge_filter_size=3, input_filter_size=5, **NET_CASES[name]))
    same, learned = not cfg["context"], cfg["upsampling"] == "learned"
    i_shape, o_shape = shapes.get_padding(cfg, [2, 22, cfg["num_channels"]])
    mix, targets = wt.synthetic_batch(cfg, 2, i_shape[1], o_shape[1], seed=5)
    tp = wt.params_to_torch(wt.init_params(cfg, seed=3), dtype=torch.float64, requires_grad=True)
    with torch.no_grad():
        for n_, p in tp:
            if n_.endswith("/bias"):
                p.uniform_(-0.3, 0.3, generator=torch.Generator().manual_seed(1))
    mix_t = torch.tensor(mix, dtype=torch.float64)
    tg = {k: torch.tensor(v, dtype=torch.float64) for k, v in targets.items()}
    oloss, ograds = wt.train_step(cfg, tp, mix_t, tg)
    grads = {n_: g.numpy() for (n_, _), g in zip(tp, ograds)}
    names = [n_ for n_, _ in tp]
    par = [p.detach() for _, p in tp]
    k_bott = 2
    i_interp = 4 if learned else None
    i_up = 5 if learned else 4
    i_head = i_up + 2
    S, Cc = cfg["num_sources"], cfg["num_channels"]
    Sh = S - (cfg["output_type"] == "difference")
    assert len(par) == i_head + 2 * Sh

    for training in (True, False):
        outs, inter = wt.get_output(cfg, tp, mix_t, training, return_intermediates=True)
        x = inter["bottleneck"].detach()
        n = x.shape[2]
        tup = 2 * n - 1 if cfg["context"] else 2 * n
        w = par[i_interp].numpy() if learned else None
        ups, _, _ = E.upsample_ref(x.numpy(), w, tup)
        skip = wt.crop(inter["down0"].detach(), tup)
        cat = torch.cat([skip, torch.tensor(ups)], dim=1)
        up0 = wt.leaky_relu(wt.conv1d_tf(cat, par[i_up], par[i_up + 1], same))
        assert np.abs(up0.numpy() - inter["up0"].detach().numpy()).max() < 1e-12
        # head
        Tfeat = up0.shape[2]
        Ko = cfg["output_filter_size"]
        Tout = Tfeat if same else Tfeat - Ko + 1
        hc = E.HeadCase(Cc, 3, Sh, S != Sh, Ko, (Ko - 1) // 2 if same else 0, Tfeat, Tout, 2, cfg["output_activation"] == "tanh",
                        training)
        x_in = mix_t.permute(0, 2, 1)
        mix_feat = wt.crop(x_in, Tfeat).numpy()
        mix_diff = wt.crop(torch.tensor(mix_feat), Tout).numpy()
        Ws = [par[i_head + 2 * s].numpy() for s in range(Sh)]
        bs = [par[i_head + 2 * s + 1].numpy() for s in range(Sh)]
        feat = inter["up0"].detach().numpy()
        out, _ = E.head_forward_ref(hc, mix_feat, mix_diff, feat, Ws, bs)
        for s, nm in enumerate(cfg["source_names"]):
            assert np.abs(out[s] - outs[nm].detach().numpy()).max() < 1e-12, (nm, training)
        assert np.abs(E.head_forward_model(hc, mix_feat, mix_diff, feat, Ws, bs) - out).max() < 1e-12
    # backward: the training graph
    hc = hc.in_training()
    out, _ = E.head_forward_ref(hc, mix_feat, mix_diff, feat, Ws, bs)
    tgt = np.stack([targets[nm] for nm in cfg["source_names"]])
    r = E.head_backward_ref(hc, mix_feat, mix_diff, feat, Ws, bs, targets=tgt)
    assert abs(r["loss"] - float(oloss)) <= 1e-13 * max(1.0, abs(float(oloss)))
    inp = torch.cat([torch.tensor(mix_feat), torch.tensor(feat)], dim=1)
    for s in range(Sh):
        dp = torch.tensor(r["dpre"][s])
        gw = _wgrad(inp, dp, Ko, same)
        assert np.abs(gw - grads[names[i_head + 2 * s]]).max() < 1e-13, names[i_head + 2 * s]
        assert np.abs(dp.sum(dim=(0, 2)).numpy() - grads[names[i_head + 2 * s + 1]]).max() < 1e-13
    dcat = _dgrad(cat, par[i_up], torch.tensor(r["dzfeat"]), same)
    dy = dcat[:, skip.shape[1]:, :]
    ub = E.upsample_backward_ref(dy, x.numpy(), w, tup)
    if learned:
        assert np.abs(ub["dw"] - grads[names[i_interp]]).max() < 1e-13
    dec = inter["down0"].detach()[:, :, ::2]
    gb = _wgrad(dec, torch.tensor(ub["dz"]), par[k_bott].shape[0], same)
    assert np.abs(gb - grads[names[k_bott]]).max() < 1e-13
    # the element-wise models say the same
    dzm, dwm = E.upsample_backward_model(dy, x.numpy(), w, tup)
    assert np.abs(dzm - ub["dz"]).max() < 1e-13 and (not learned or np.abs(dwm - ub["dw"]).max() < 1e-13)
    dpm, _ = E.head_dpre_model(hc, out, targets=tgt)
    assert np.abs(dpm - r["dpre"]).max() < 1e-13
    assert np.abs(E.head_dfeat_model(hc, dpm, feat, Ws) - r["dzfeat"]).max() < 1e-13


# ---------------------------------------------------------------------------------------------------------------------------
# models == references on the GPU tests' own cases, and the case tables cover what they claim
# ---------------------------------------------------------------------------------------------------------------------------
def _ups_cases(ns=E.UPS_N):
    for B, Cn in E.UPS_BC:
        for n in ns:
            for tup in (2 * n - 1, 2 * n):
                for learned in (0, 1):
                    for bf in (0, 1):
                        yield B, Cn, n, tup, learned, bf


def test_upsampling_cases_cover_the_residues():
    assert {(B * Cn) % 4 for B, Cn in E.UPS_BC} == {3, 2, 0}
    for m in (4, 8):
        assert {(2 * n - 1) % m for n in E.UPS_N} | {(2 * n) % m for n in E.UPS_N} == set(range(m))
    assert {n % 4 for n in E.UPS_N} == set(range(4)) and 1 in E.UPS_N and max(E.UPS_N) // 2 > 1024 // 2
    x, _, _ = E.ups_inputs(2, 1, 1, 1, 0, 0)
    assert x.size == 2 and x.reshape(-1)[1] == 0                       # even the smallest case has a tie
    x, _, _ = E.ups_inputs(3, 5, 9, 18, 1, 1)
    z = x[x == 0]
    assert np.signbit(z).any() and not np.signbit(z).all() and (x < 0).any() and (x > 0).any()
    assert np.array_equal(E.bf16_round(x), x)


def test_head_cases_cover_what_they_claim():
    allc = [(hc, bf) for F in E.HEAD_F for hc, bf in E.head_cases(F)]
    assert len(allc) == 7 * 2 * 9 * 4
    four = [(hc, bf) for hc, bf in allc if hc.Ko == 1 and hc.Tout >= 4]         # shapes the four-position forms take
    for group in (allc, four):
        assert {(hc.Sh, hc.difference) for hc, _ in group} == {(s, d) for s in range(1, 5) for d in (0, 1)}
        assert {(hc.tanh, hc.training, bf) for hc, bf in group} == {(t, tr, b) for t, tr in E.HEAD_ACT for b in (0, 1)}
        assert {(hc.F, hc.C, hc.Tout % 4) for hc, _ in group} >= {(F, Cn, r) for F in E.HEAD_F for Cn in (1, 2) for r in range(4)}
    assert {hc.B for hc, _ in allc} == {1, 2, 3}
    # |pre-activation| > 1 occurs: the clip of the linear head at inference does something, on both sides
    lo = hi = 0
    for hc, bf in E.head_cases(5):
        if not hc.tanh and not hc.training:
            d = E.head_inputs(hc, bf)
            free, _ = E.head_forward_ref(hc.in_training(), d["mix_feat"], d["mix_diff"], d["feat"], d["Ws"], d["bs"])
            lo += int((free[:hc.Sh] < -1).sum())
            hi += int((free[:hc.Sh] > 1).sum())
    assert lo > 10 and hi > 10
    hoff, n = E.head_param_layout(allc[5][0])
    assert hoff == sorted(hoff, reverse=True) or len(hoff) == 1


# ---------------------------------------------------------------------------------------------------------------------------
# sensitivity
# ---------------------------------------------------------------------------------------------------------------------------
def _store(a, bf, mode="nearest"):
    """What a correct kernel would store of the float64 value a."""
    return E.bf16_round(a, mode) if bf else np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def test_unmutated_models_pass_every_upsampling_case():
    for B, Cn, n, tup, learned, bf in _ups_cases():
        x, dy, w = E.ups_inputs(B, Cn, n, tup, learned, bf)
        y, mag, big = E.upsample_ref(x, w, tup)
        assert E.ups_verdict(_store(E.upsample_model(x, w, tup), bf), y, w, bf, mag, big) <= 1
        r = E.upsample_backward_ref(dy, x, w, tup)
        dz, dw = E.upsample_backward_model(dy, x, w, tup)
        assert E.dz_verdict(_store(dz, bf), r, w, bf) <= 1
        if learned:
            assert np.abs(dw - r["dw"]).max() <= 1e-12 * max(1.0, np.abs(r["dw"]).max())


UPS_MUTANTS = [
    # (mutant, applies(n, tup, learned, C), which results it must move)
    ("half_clamp", lambda n, tup, learned, Cn: not learned and tup == 2 * n, ("y", "dz")),
    ("tie_one", lambda n, tup, learned, Cn: True, ("dz",)),
    ("x_n_repeats", lambda n, tup, learned, Cn: learned and tup == 2 * n, ("y", "dw")),
    ("channel_xor", lambda n, tup, learned, Cn: learned and Cn >= 2 and n >= 2, ("y", "dz", "dw")),
    ("tail_unwritten", lambda n, tup, learned, Cn: True, ("y", "dz")),
]


@pytest.mark.parametrize("mutant", [m[0] for m in UPS_MUTANTS])
def test_upsampling_mutants_fail_every_case_they_apply_to(mutant):
    _, applies, moves = [m for m in UPS_MUTANTS if m[0] == mutant][0]
    ran = 0
    for B, Cn, n, tup, learned, bf in _ups_cases():
        if not applies(n, tup, learned, Cn):
            continue
        ran += 1
        x, dy, w = E.ups_inputs(B, Cn, n, tup, learned, bf)
        key = (mutant, B, Cn, n, tup, learned, bf)
        if "y" in moves:
            y, mag, big = E.upsample_ref(x, w, tup)
            assert E.ups_verdict(_store(E.upsample_model(x, w, tup, mutant), bf), y, w, bf, mag, big) > 1, key
        r = E.upsample_backward_ref(dy, x, w, tup)
        dz, dw = E.upsample_backward_model(dy, x, w, tup, mutant)
        if "dz" in moves:
            assert E.dz_verdict(_store(dz, bf), r, w, bf) > 1, key
        if "dw" in moves:
            assert np.abs(dw - r["dw"]).max() > E.op_tol(r["dw"]), key
    assert ran >= 39


def test_bf16_truncation_passes_the_element_bound_and_fails_the_share_cap():
    """Truncation instead of round-to-nearest-even on the bf16 store stays inside one spacing per element -- the pooled share
    of elements that differ from the reference is what catches it; the correct store stays far below the cap."""
    for learned in (0, 1):
        good_y, bad_y, good_z, bad_z = [0, 0], [0, 0], [0, 0], [0, 0]
        for B, Cn, n, tup, lr, bf in _ups_cases():
            if not bf or lr != learned:
                continue
            x, dy, w = E.ups_inputs(B, Cn, n, tup, learned, 1)
            y, mag, big = E.upsample_ref(x, w, tup)
            ym = E.upsample_model(x, w, tup)
            assert E.ups_verdict(_store(ym, 1), y, w, 1, mag, big, good_y) <= 1
            assert E.ups_verdict(_store(ym, 1, "truncate"), y, w, 1, mag, big, bad_y) <= 1
            r = E.upsample_backward_ref(dy, x, w, tup)
            dz, _ = E.upsample_backward_model(dy, x, w, tup)
            assert E.dz_verdict(_store(dz, 1), r, w, 1, good_z) <= 1
            assert E.dz_verdict(_store(dz, 1, "truncate"), r, w, 1, bad_z) <= 1
        for good, bad in ((good_y, bad_y), (good_z, bad_z)):
            assert good[0] == 0 and good[1] > 10000
            assert bad[0] / bad[1] > 10 * E.BF16_DIFF_SHARE, (learned, bad)
    # the rounding helper itself: ties to even, against torch's fp32 -> bf16
    v = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -1.0 - 2.0 ** -8, 0.3, -7.77, 1e-3, 255.5, 3.0 ** 0.5])
    assert np.array_equal(E.bf16_round(v), torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).double().numpy())
    assert E.bf16_round(1.0 + 2.0 ** -8) == 1.0 and E.bf16_round(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6
    assert E.bf16_round(1.0 + 3 * 2.0 ** -8, "truncate") == 1.0 + 2.0 ** -7
    assert np.array_equal(E.from_bf16_bits(E.to_bf16_bits(E.bf16_round(v))).astype(np.float64), E.bf16_round(v))
    assert E.bf16_spacing(1.0) == 2.0 ** -7 and E.bf16_spacing(0.75) == 2.0 ** -8


def _head_refs(hc, bf):
    d = E.head_inputs(hc, bf)
    a = (d["mix_feat"], d["mix_diff"], d["feat"], d["Ws"], d["bs"])
    out, mag = E.head_forward_ref(hc, *a)
    out_t, _ = E.head_forward_ref(hc.in_training(), *a)
    out32 = out_t.astype(np.float32).astype(np.float64)                  # what the backward entries are fed
    return d, a, out, mag, out32


HEAD_MUTANTS = ["tie_one", "no_tanh_derivative", "glast_sign", "channel_xor", "tail_unwritten"]


@pytest.mark.parametrize("F", E.HEAD_F)
def test_head_models_pass_and_mutants_fail_every_case_they_apply_to(F):
    ran = {m: 0 for m in HEAD_MUTANTS}
    for hc, bf in E.head_cases(F):
        d, a, out, mag, out32 = _head_refs(hc, bf)
        ob = E.head_out_bound(hc, out, mag)
        assert E.worst_ratio(E.head_forward_model(hc, *a), out, ob) <= 1
        for mut in ("channel_xor", "tail_unwritten"):
            if mut == "channel_xor" and hc.C < 2:
                continue
            assert E.worst_ratio(E.head_forward_model(hc, *a, mutant=mut), out, ob) > 1, (mut, hc)
        for kw in ({"targets": d["targets"]}, {"d_outputs": d["d_outputs"]}):
            r = E.head_backward_ref(hc, *a, **kw)
            # the reference is the graph at the float64 outputs; the entries are fed their fp32 rounding
            dp, dp_mag = E.head_dpre_model(hc, out32, **kw)
            pb = E.dpre_bound(hc, dp_mag, r["dpre"])
            assert E.worst_ratio(dp, r["dpre"], pb) <= 1, hc
            dzf = E.head_dfeat_model(hc, dp, d["feat"], d["Ws"])
            assert E.dzfeat_verdict(hc, _store(dzf, bf), r, dp_mag, bf) <= 1, hc
            for mut in HEAD_MUTANTS:
                applies = {"tie_one": bool((d["feat"] == 0).any()), "no_tanh_derivative": bool(hc.tanh), "glast_sign": bool(hc.difference),
                           "channel_xor": hc.C == 2, "tail_unwritten": True}[mut]
                if not applies:
                    continue
                ran[mut] += 1
                if mut in ("no_tanh_derivative", "glast_sign"):
                    bad, _ = E.head_dpre_model(hc, out32, mutant=mut, **kw)
                    assert E.worst_ratio(bad, r["dpre"], pb) > 1, (mut, hc)
                else:
                    bad = E.head_dfeat_model(hc, dp, d["feat"], d["Ws"], mutant=mut)
                    assert E.dzfeat_verdict(hc, _store(bad, bf), r, dp_mag, bf) > 1, (mut, hc)
    assert all(v >= 20 for v in ran.values()), ran
