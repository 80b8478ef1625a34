"""Operator-level GPU tests of the elementwise family (wave-u-net_amd/csrc/wun_elementwise.hip: 2x upsampling and its adjoint,
the learned-interpolation weight gradient, the output head with its loss and gradients, the [B, T, C] -> NCW layout change) and
of the two fused forms of the split-K epilogue (wun_kernels.hip), each against the float64 references of
tests/_elementwise_np.py, at the residues, alignments and sizes where each form of each kernel can go wrong.

Everywhere: outputs are NaN-prefilled with NaN guards before and behind them and in the row padding between length and pitch --
afterwards every element inside a row is finite and every element outside is still NaN (the footprint contract, DESIGN.md
section 2); results are bit-identical across the forms of one operator; wun_op_last_path() says which form ran, the layouts
assert the form they are meant to reach, and the last test asserts that every form of every operator was seen.

Bounds (tests/_elementwise_np.py; judged against mutants on these very cases by tests/test_elementwise_host.py): exact arithmetic
bit-exact; other fp32 values (terms + 2) 2^-24 sum|terms| + 2^-24 |ref|; values through __expf / tanhf and dw OP_TOL (5e-6 x
max(1, max|ref|): 10x the largest error observed); the loss LOSS_TOL; bf16 rows one spacing + the fp32 bound per element, and at most 1e-3 of all elements of a test function differing from
the once-rounded float64 reference at all."""
import ctypes as C

import numpy as np
import pytest
import torch

import _elementwise_np as E
from _observed import record
from wave_u_net_amd import _lib

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 64                                   # guard elements before and behind every buffer (keeps 16-byte alignment)
SEEN = {op: set() for op in range(7)}        # wun_op_last_path values per operator, for the last test
FUSED_SEEN = set()                           # (kind, n mod 4, tup parity) that reported the fused epilogue
POOL = {}                                    # test function -> [bf16 elements that differ from the reference, elements]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sync():
    """Wait for the launch; a device fault ends the whole run here (nothing more is started on a faulted device)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error, stopping: %s" % e, returncode=3)


def _path(lib, op):
    p = lib.wun_op_last_path(op)
    SEEN[op].add(p)
    return p


def _pad(t, m):
    return (t + m - 1) // m * m


class Rows:
    """R rows of `length` elements, `pitch` apart, `off` elements behind a 16-byte aligned address, inside a NaN-filled
    allocation with guards: inputs carry `data`, outputs stay NaN until the kernel writes them."""

    def __init__(self, R, length, pitch, off=0, bf=False, data=None):
        self.R, self.length, self.pitch = R, length, pitch
        dt = torch.bfloat16 if bf else torch.float32
        self.buf = torch.full((GUARD + off + R * pitch + GUARD,), NAN, dtype=dt, device="cuda")
        self.view = self.buf[GUARD + off:GUARD + off + R * pitch].view(R, pitch)
        assert (self.buf.data_ptr() % 16) == 0 and self.view.data_ptr() % 16 == (off * self.buf.element_size()) % 16
        if data is not None:
            self.view[:, :length] = torch.as_tensor(np.asarray(data, dtype=np.float32).reshape(R, length)).to(dt).cuda()

    @property
    def ptr(self):
        return self.view.data_ptr()

    def reset(self):
        self.buf.fill_(NAN)

    def get(self, shape=None):
        a = self.view[:, :self.length].float().cpu().numpy().astype(np.float64)
        return a if shape is None else a.reshape(shape)

    def check_footprint(self, what):
        host = self.buf.float().cpu().numpy()
        inside = np.zeros(host.shape, dtype=bool)
        start = self.view.data_ptr() - self.buf.data_ptr()
        start //= self.buf.element_size()
        for r in range(self.R):
            inside[start + r * self.pitch:start + r * self.pitch + self.length] = True
        assert np.isfinite(host[inside]).all(), "%s: an element inside a row was left unwritten" % (what,)
        assert np.isnan(host[~inside]).all(), "%s: an element outside the rows was written" % (what,)


def _pool(name):
    return POOL.setdefault(name, [0, 0])


# ---------------------------------------------------------------------------------------------------------------------------
# upsampling and its adjoint
# ---------------------------------------------------------------------------------------------------------------------------
LAYOUTS = ("aligned", "x_unpadded", "out_offset", "pitch4")


def _ups_geometry(layout, n, tup):
    """-> xpitch, ypitch, element offset of the OUTPUT's base (y forward, dz backward)."""
    xp, yp, off = _pad(n, 8) + 8, _pad(tup, 8) + 8, 0
    if layout == "x_unpadded":
        xp = n
    elif layout == "out_offset":
        off = 1
    elif layout == "pitch4":                 # a multiple of 4 but not of 8
        xp, yp = _pad(n, 8) + 4, _pad(tup, 8) + 4
    return xp, yp, off


def _expected_forward(layout, n, bf):
    if layout == "out_offset":
        return _lib.PATH_SCALAR
    if not bf or layout == "pitch4":
        return _lib.PATH_VEC4
    if layout == "x_unpadded" and n % 4:
        return _lib.PATH_VEC4                # the generic bf16 vector form: x rows not 8-byte aligned
    return _lib.PATH_VEC8_BF16


def _expected_backward(layout, n):
    if layout == "out_offset" or (layout == "x_unpadded" and n % 4):
        return _lib.PATH_SCALAR
    return _lib.PATH_VEC4


def _ups_forward(lib, x, w, B, Cn, n, tup, bf, layout):
    xp, yp, off = _ups_geometry(layout, n, tup)
    xr = Rows(B * Cn, n, xp, 0, bf, x)
    yr = Rows(B * Cn, tup, yp, off, bf)
    wd = None if w is None else torch.tensor(w, device="cuda")
    _lib.check(lib.wun_op_upsample(xr.ptr, yr.ptr, None if w is None else wd.data_ptr(), B, Cn, n, tup, xp, yp, int(bf), _stream()))
    _sync()
    path = _path(lib, _lib.OP_UPSAMPLE)
    yr.check_footprint(("upsample", layout, B, Cn, n, tup, bf))
    return yr.get((B, Cn, tup)), path


def _ups_backward(lib, x, dy, w, B, Cn, n, tup, bf, layout, dw_mode=None, dw_init=None):
    """dw_mode: None, or (two_stage, accumulate).  -> dz, dw (or None), path of the adjoint, path of the weight gradient."""
    xp, yp, off = _ups_geometry(layout, n, tup)
    dyr = Rows(B * Cn, tup, yp, 0, bf, dy)
    xr = Rows(B * Cn, n, xp, 0, bf, x)
    dzr = Rows(B * Cn, n, xp, off, bf)
    wd = None if w is None else torch.tensor(w, device="cuda")
    dwr = part = None
    if dw_mode is not None:
        two_stage, accumulate = dw_mode
        dwr = Rows(1, Cn, Cn, 0, False, dw_init if accumulate else None)
        part = Rows(1, B * Cn, B * Cn) if two_stage else None
    _lib.check(lib.wun_op_upsample_backward(dyr.ptr, xr.ptr, dzr.ptr, None if w is None else wd.data_ptr(),
                                            None if dwr is None else dwr.ptr, None if part is None else part.ptr,
                                            B, Cn, n, tup, yp, xp, int(bf), int(bool(dw_mode and dw_mode[1])), _stream()))
    _sync()
    path = _path(lib, _lib.OP_UPSAMPLE_BACKWARD)
    dzr.check_footprint(("upsample_backward", layout, B, Cn, n, tup, bf))
    dw = gpath = None
    if dwr is not None:
        gpath = _path(lib, _lib.OP_INTERP_GRAD)
        dwr.check_footprint(("interp_grad dw", layout, B, Cn, n, tup, bf, dw_mode))
        dw = dwr.get().reshape(-1)
        if part is not None and gpath == _lib.PATH_TWO_STAGE:
            part.check_footprint(("interp_grad partial", layout, B, Cn, n, tup))
    return dzr.get((B, Cn, n)), dw, path, gpath


@pytest.mark.parametrize("bf", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("learned", [0, 1], ids=["linear", "learned"])
@pytest.mark.parametrize("B,Cn", E.UPS_BC)
def test_upsample_forward(lib, B, Cn, learned, bf):
    worst = raw = 0.0
    for n in E.UPS_N:
        for tup in (2 * n - 1, 2 * n):
            x, _, w = E.ups_inputs(B, Cn, n, tup, learned, bf)
            ref, mag, big = E.upsample_ref(x, w, tup)
            first = None
            for layout in LAYOUTS if bf else LAYOUTS[:3]:
                key = (layout, B, Cn, n, tup, learned, bf)
                got, path = _ups_forward(lib, x, w, B, Cn, n, tup, bf, layout)
                assert path == _expected_forward(layout, n, bf), key
                ratio = E.ups_verdict(got, ref, w, bf, mag, big, _pool("test_upsample_forward") if bf else None)
                worst = max(worst, ratio)
                if learned and not bf:
                    raw = max(raw, float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max())))
                assert ratio <= 1, (key, ratio)
                if not bf:
                    assert np.array_equal(got[:, :, 0::2], x[:, :, :(tup + 1) // 2]), key          # even outputs are copies
                first = got if first is None else first
                assert np.array_equal(got, first), ("forms differ", key)
    record("op_upsample", "B%d C%d %s %s err/bound" % (B, Cn, "learned" if learned else "linear", "bf16" if bf else "fp32"), worst, 1.0)
    if learned and not bf:
        record("op_upsample", "B%d C%d learned fp32 rel" % (B, Cn), raw, E.OP_TOL)


@pytest.mark.parametrize("bf", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("learned", [0, 1], ids=["linear", "learned"])
@pytest.mark.parametrize("B,Cn", E.UPS_BC)
def test_upsample_backward_and_interp_grad(lib, B, Cn, learned, bf):
    worst = raw = raw_dw = 0.0
    for n in E.UPS_N:
        for tup in (2 * n - 1, 2 * n):
            x, dy, w = E.ups_inputs(B, Cn, n, tup, learned, bf)
            r = E.upsample_backward_ref(dy, x, w, tup)
            init = (np.arange(Cn) * 0.37 - 1.0).astype(np.float32)                  # known values for the accumulate mode
            first = None
            for layout in LAYOUTS if bf else LAYOUTS[:3]:
                key = (layout, B, Cn, n, tup, learned, bf)
                modes = [(True, False), (False, False), (True, True), (False, True)] if learned else [None]
                stored = {}
                for mode in modes:
                    dz, dw, path, gpath = _ups_backward(lib, x, dy, w, B, Cn, n, tup, bf, layout, mode, init)
                    assert path == _expected_backward(layout, n), key
                    if mode is modes[0]:
                        ratio = E.dz_verdict(dz, r, w, bf, _pool("test_upsample_backward_and_interp_grad") if bf else None)
                        worst = max(worst, ratio)
                        if learned and not bf:
                            raw = max(raw, float(np.abs(dz - r["dz"]).max()) / max(1.0, float(np.abs(r["dz"]).max())))
                        assert ratio <= 1, (key, ratio)
                        first = dz if first is None else first
                    assert np.array_equal(dz, first), ("forms differ", key, mode)
                    if mode is None:
                        continue
                    two_stage, accumulate = mode
                    # (the two-stage form reads dy and x by vectors: it does not care where dz lies)
                    rows_ok = not (layout == "x_unpadded" and n % 4)
                    want = _lib.PATH_TWO_STAGE if two_stage and rows_ok else _lib.PATH_ONE_STAGE
                    assert gpath == want, (key, mode)
                    if not accumulate:
                        stored[gpath] = dw
                        err = float(np.abs(dw - r["dw"]).max())
                        raw_dw = max(raw_dw, err / max(1.0, float(np.abs(r["dw"]).max())))
                        assert err <= E.op_tol(r["dw"]), (key, mode, err)
                    else:
                        # one IEEE add of the stored form's value to what dw held
                        expect = (init + stored[gpath].astype(np.float32)).astype(np.float64)
                        assert np.array_equal(dw, expect), (key, mode)
    tag = "B%d C%d %s %s" % (B, Cn, "learned" if learned else "linear", "bf16" if bf else "fp32")
    record("op_upsample_backward", tag + " err/bound", worst, 1.0)
    if learned:
        record("op_upsample_backward", tag + " dw rel", raw_dw, E.OP_TOL)
        if not bf:
            record("op_upsample_backward", tag + " dz rel", raw, E.OP_TOL)


def test_upsample_scalar_forms_take_a_second_grid_trip(lib):
    """The scalar forms cap their grid at 8192 blocks of 256 threads: above 2 097 152 elements every thread loops."""
    B, Cn, n = 1, 2, 1048601
    tup = 2 * n
    assert B * Cn * n > 8192 * 256
    x, dy, _ = E.ups_inputs(B, Cn, n, tup, 0, 0)
    ref, mag, big = E.upsample_ref(x, None, tup)
    got, path = _ups_forward(lib, x, None, B, Cn, n, tup, 0, "out_offset")
    assert path == _lib.PATH_SCALAR and E.ups_verdict(got, ref, None, 0, mag, big) <= 1
    r = E.upsample_backward_ref(dy, x, None, tup)
    dz, _, path, _ = _ups_backward(lib, x, dy, None, B, Cn, n, tup, 0, "out_offset")
    ratio = E.dz_verdict(dz, r, None, 0)
    record("op_upsample_backward", "scalar second trip err/bound", ratio, 1.0)
    assert path == _lib.PATH_SCALAR and ratio <= 1


# ---------------------------------------------------------------------------------------------------------------------------
# head
# ---------------------------------------------------------------------------------------------------------------------------
HEAD_LAYOUTS = ("aligned", "offset", "dpre_unpadded")


def _head_geometry(hc, layout, mix_len):
    """-> feature pitch, element offset of the feature map / its gradient, dpre pitch, mix pitch."""
    if layout == "offset":
        return hc.Tfeat + 1, 1, hc.Tout, mix_len
    fp = _pad(hc.Tfeat, 8) + 8
    return fp, 0, (hc.Tout if layout == "dpre_unpadded" else _pad(hc.Tout, 4) + 4), _pad(mix_len, 4)


def _four_ok(hc, layout):
    return layout != "offset" and hc.Ko == 1 and hc.padl == 0 and hc.Tfeat == hc.Tout and hc.Tout >= 4


def _dfeat_four_ok(hc, layout, dpp):
    return _four_ok(hc, layout) and dpp % 4 == 0 and (hc.C * dpp) % 4 == 0 and (hc.B * hc.C * dpp) % 4 == 0


class HeadRun:
    """One head problem on the device in one layout."""

    def __init__(self, lib, hc, bf, d, layout):
        self.lib, self.hc, self.bf, self.layout = lib, hc, bf, layout
        self.fp, self.foff, self.dpp, self.mp = _head_geometry(hc, layout, d["mix_len"])
        self.desc = _lib.WunOpHeadDesc(C=hc.C, F=hc.F, S=hc.S, difference=hc.difference, Ko=hc.Ko, padl=hc.padl, Tfeat=hc.Tfeat,
                                       Tout=hc.Tout, B=hc.B, tanh=hc.tanh, training=hc.training, feat_bf16=int(bf),
                                       mix_pitch=self.mp, feat_pitch=self.fp, dpre_pitch=self.dpp,
                                       mix_off_feat=d["off_feat"], mix_off_diff=d["off_diff"])
        self.mix = Rows(hc.B * hc.C, d["mix_len"], self.mp, 0, False, d["mix"])
        self.feat = Rows(hc.B * hc.F, hc.Tfeat, self.fp, self.foff, bf, d["feat"])
        hoff, arena = E.head_param_arena(hc, d["Ws"], d["bs"])
        self.params = torch.tensor(arena, device="cuda")
        self.hoff = (C.c_int64 * 4)(*(hoff + [0] * (4 - len(hoff))))

    def forward(self, training=None):
        hc = self.hc
        desc = self.desc
        if training is not None:
            desc = _lib.WunOpHeadDesc.from_buffer_copy(self.desc)
            desc.training = training
        out = Rows(1, hc.S * hc.B * hc.Tout * hc.C, hc.S * hc.B * hc.Tout * hc.C)
        _lib.check(self.lib.wun_op_head_forward(C.byref(desc), self.mix.ptr, self.feat.ptr, self.params.data_ptr(), self.hoff,
                                                out.ptr, _stream()))
        _sync()
        path = _path(self.lib, _lib.OP_HEAD_FORWARD)
        assert path == (_lib.PATH_FOUR_POSITION if _four_ok(hc, self.layout) else _lib.PATH_GENERIC), (hc, self.layout)
        out.check_footprint(("head_forward", hc, self.layout))
        return out.get((hc.S, hc.B, hc.Tout, hc.C))

    def backward(self, out32, targets=None, d_outputs=None):
        """-> dpre [Sh, B, C, Tout], dzfeat [B, F, Tfeat], loss (or None)."""
        hc = self.hc
        od = torch.tensor(np.asarray(out32, dtype=np.float32), device="cuda")
        dpre = Rows(hc.Sh * hc.B * hc.C, hc.Tout, self.dpp)
        dzf = Rows(hc.B * hc.F, hc.Tfeat, self.fp, self.foff, self.bf)
        loss = None
        if targets is not None:
            td = torch.tensor(np.asarray(targets, dtype=np.float32), device="cuda")
            loss = Rows(1, 1, 1)
            _lib.check(self.lib.wun_op_head_loss_backward(C.byref(self.desc), self.feat.ptr, self.params.data_ptr(), self.hoff,
                                                          od.data_ptr(), td.data_ptr(), dpre.ptr, dzf.ptr, loss.ptr, _stream()))
        else:
            gd = torch.tensor(np.asarray(d_outputs, dtype=np.float32), device="cuda")
            _lib.check(self.lib.wun_op_head_backward(C.byref(self.desc), self.feat.ptr, self.params.data_ptr(), self.hoff,
                                                     od.data_ptr(), gd.data_ptr(), dpre.ptr, dzf.ptr, _stream()))
        _sync()
        path = _path(self.lib, _lib.OP_HEAD_DFEAT)
        want = _lib.PATH_FOUR_POSITION if _dfeat_four_ok(hc, self.layout, self.dpp) else _lib.PATH_GENERIC
        assert path == want, (hc, self.layout)
        dpre.check_footprint(("head dpre", hc, self.layout))
        dzf.check_footprint(("head dzfeat", hc, self.layout))
        if loss is not None:
            loss.check_footprint(("head loss", hc, self.layout))
            loss = float(loss.get()[0, 0])
        return dpre.get((hc.Sh, hc.B, hc.C, hc.Tout)), dzf.get((hc.B, hc.F, hc.Tfeat)), loss


def _check_head_case(lib, hc, bf, layouts, obs, pool_name):
    d = E.head_inputs(hc, bf)
    a = (d["mix_feat"], d["mix_diff"], d["feat"], d["Ws"], d["bs"])
    ref_out, mag = E.head_forward_ref(hc, *a)
    ref_train, _ = E.head_forward_ref(hc.in_training(), *a)
    out32 = ref_train.astype(np.float32).astype(np.float64)          # the backward entries' input: the reference, rounded
    ob = E.head_out_bound(hc, ref_out, mag)
    refs = {"targets": E.head_backward_ref(hc, *a, targets=d["targets"]),
            "d_outputs": E.head_backward_ref(hc, *a, d_outputs=d["d_outputs"])}
    first = {}
    for layout in layouts:
        run = HeadRun(lib, hc, bf, d, layout)
        key = (hc, bf, layout)
        out = run.forward()
        ratio = E.worst_ratio(out, ref_out, ob)
        obs["out"] = max(obs.get("out", 0.0), ratio)
        if hc.tanh:
            obs["out tanh rel"] = max(obs.get("out tanh rel", 0.0),
                                      float(np.abs(out[:hc.Sh] - ref_out[:hc.Sh]).max()) / max(1.0, float(np.abs(ref_out[:hc.Sh]).max())))
        assert ratio <= 1, (key, ratio)
        assert np.array_equal(out, first.setdefault("out", out)), ("forms differ", key)
        for kind in ("targets", "d_outputs"):
            r = refs[kind]
            dpre, dzf, loss = run.backward(out32, **{kind: d[kind]})
            _, dp_mag = E.head_dpre_model(hc, out32, **{kind: d[kind]})
            ratio = E.worst_ratio(dpre, r["dpre"], E.dpre_bound(hc, dp_mag, r["dpre"]))
            obs["dpre"] = max(obs.get("dpre", 0.0), ratio)
            assert ratio <= 1, (key, kind, "dpre", ratio)
            ratio = E.dzfeat_verdict(hc, dzf, r, dp_mag, bf, _pool(pool_name) if bf else None)
            k = "dzfeat bf16" if bf else "dzfeat"
            obs[k] = max(obs.get(k, 0.0), ratio)
            assert ratio <= 1, (key, kind, "dzfeat", ratio)
            if loss is not None:
                rel = abs(loss - r["loss"]) / max(abs(r["loss"]), 1e-30)
                obs["loss rel"] = max(obs.get("loss rel", 0.0), rel)
                assert rel <= E.LOSS_TOL, (key, loss, r["loss"])
            assert np.array_equal(dpre, first.setdefault(kind + " dpre", dpre)), ("forms differ", key, kind)
            assert np.array_equal(dzf, first.setdefault(kind + " dzfeat", dzf)), ("forms differ", key, kind)


def _record_head(tag, obs):
    for k, v in sorted(obs.items()):
        record("op_head", "%s %s" % (tag, k), v, E.LOSS_TOL if k == "loss rel" else (E.OP_TOL if k.endswith("rel") else 1.0))


@pytest.mark.parametrize("F", E.HEAD_F)
def test_head_forward_loss_and_gradients(lib, F):
    obs = {}
    for hc, bf in E.head_cases(F):
        _check_head_case(lib, hc, bf, HEAD_LAYOUTS, obs, "test_head_forward_loss_and_gradients")
    _record_head("F%d" % F, obs)


def test_head_four_position_forms_take_a_second_grid_trip(lib):
    """head_fwd4_kernel / head_dfeat4_kernel cap their grid at 4096 workgroups of 256 threads, four positions each."""
    Tout = 4096 * 256 * 4 + 4 * 300 + 3
    hc = E.HeadCase(1, 1, 1, 0, 1, 0, Tout, Tout, 1, 0, 1)
    assert hc.B * (hc.Tout // 4) > 4096 * 256
    obs = {}
    _check_head_case(lib, hc, 0, ("aligned",), obs, "second_trip")
    _record_head("four-position second trip", obs)


def test_head_loss_and_gradient_kernels_take_a_second_grid_trip(lib):
    """head_bwd_kernel / head_grad_kernel cap their grid at 1024 workgroups of 256 threads, one position each."""
    hc = E.HeadCase(2, 3, 2, 1, 1, 0, 87500, 87500, 3, 1, 1)
    assert hc.B * hc.Tout > 1024 * 256
    obs = {}
    _check_head_case(lib, hc, 0, ("aligned", "offset"), obs, "second_trip")
    _record_head("loss / gradient second trip", obs)


# ---------------------------------------------------------------------------------------------------------------------------
# layout change
# ---------------------------------------------------------------------------------------------------------------------------
def _btc(lib, src, B, T, Cn, pitch, off):
    sd = torch.tensor(src, device="cuda")
    dst = Rows(B * Cn, T, pitch, off)
    _lib.check(lib.wun_op_btc_to_ncw(sd.data_ptr(), dst.ptr, B, T, Cn, pitch, _stream()))
    _sync()
    path = _path(lib, _lib.OP_BTC_TO_NCW)
    want = _lib.PATH_VEC4 if (Cn <= 2 and pitch % 4 == 0 and off == 0) else _lib.PATH_SCALAR
    assert path == want, (B, T, Cn, pitch, off)
    dst.check_footprint(("btc_to_ncw", B, T, Cn, pitch, off))
    return dst.view[:, :T].cpu().numpy().reshape(B, Cn, T)


@pytest.mark.parametrize("Cn", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 1023, 1024, 1025, 1027])
def test_btc_to_ncw_is_a_bit_exact_transpose(lib, T, Cn):
    B = 3
    src = np.random.default_rng(T * 4 + Cn).uniform(-1, 1, (B, T, Cn)).astype(np.float32)
    for pitch in (_pad(T, 4) + 4, T):
        for off in (0, 1):
            got = _btc(lib, src, B, T, Cn, pitch, off)
            assert np.array_equal(got.view(np.uint32), E.btc_to_ncw_ref(src).view(np.uint32)), (T, Cn, pitch, off)


def test_btc_to_ncw_scalar_form_takes_a_second_grid_trip(lib):
    B, T, Cn = 1, 700001, 3
    assert B * T * Cn > 8192 * 256
    src = np.random.default_rng(5).uniform(-1, 1, (B, T, Cn)).astype(np.float32)
    got = _btc(lib, src, B, T, Cn, T, 0)
    assert np.array_equal(got.view(np.uint32), E.btc_to_ncw_ref(src).view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------------
# the fused forms in the split-K epilogue
# ---------------------------------------------------------------------------------------------------------------------------
FUSED_N = tuple(n for n in E.UPS_N if n <= 129)
CIN, KW, BATCH = 16, 5, 16
# Output channels.  8: no tile of the menu is a legal FORCED choice (more than a third of its columns would be padding), the
# dispatcher's own choice splits K and fuses.  16: the forced (variant, split) choices run too.
COUTS = (8, 16)


def _conv64(x, w, bias, lrelu):
    y = torch.nn.functional.conv1d(torch.tensor(x, dtype=torch.float64), torch.tensor(w, dtype=torch.float64).permute(2, 1, 0),
                                   None if bias is None else torch.tensor(bias, dtype=torch.float64))
    return (torch.maximum(0.2 * y, y) if lrelu else y).numpy()


def _choices(lib):
    """The dispatcher's own choice, then every (variant, split-K factor); split 1 never reaches the epilogue kernel."""
    return [(-1, 0)] + [(v, ks) for v in range(lib.wun_op_num_conv_variants()) for ks in (1, 2, 3, 4)]


@pytest.mark.parametrize("COUT", COUTS)
@pytest.mark.parametrize("n", FUSED_N)
def test_fused_upsampling_in_the_split_k_epilogue(lib, n, COUT):
    """A conv launch that ends in the split-K epilogue writes the upsampled copy of its output there: against float64, and
    against wun_op_upsample on the conv output the same launch stored (bit for bit with linear weights, within one rounding
    of the interpolation with learned ones)."""
    rng = np.random.default_rng(n + 7 * COUT)
    x = rng.uniform(-1, 1, (BATCH, CIN, n + KW - 1)).astype(np.float32)
    w = (rng.uniform(-1, 1, (KW, CIN, COUT)) / np.sqrt(KW * CIN)).astype(np.float32)
    bias = rng.uniform(-0.1, 0.1, COUT).astype(np.float32)
    iw = rng.uniform(-4, 4, COUT).astype(np.float32)
    y64 = _conv64(x, w, bias, True)
    xd, wd, bd, iwd = (torch.tensor(a, device="cuda") for a in (x, w, bias, iw))
    fused = worst = 0
    try:
        for tup in (2 * n - 1, 2 * n):
            for learned in (0, 1):
                ref, _, _ = E.upsample_ref(y64, iw if learned else None, tup)
                for pitch in (_pad(tup, 4) + 4, tup):
                    y, up, alone = Rows(BATCH * COUT, n, n), Rows(BATCH * COUT, tup, pitch), Rows(BATCH * COUT, tup, pitch)
                    _lib.check(lib.wun_op_set_conv_upsample(up.ptr, pitch, tup, iwd.data_ptr() if learned else None))
                    for v, ks in _choices(lib):
                        lib.wun_op_force_conv_variant(v, ks)
                        rc = lib.wun_op_conv1d_ex(xd.data_ptr(), CIN, None, 0, wd.data_ptr(), bd.data_ptr(), y.ptr, None, BATCH, COUT,
                                                  KW, n + KW - 1, n, n, 1, 0, 1, 0, 1, 0, _stream())
                        if rc != 0:
                            continue                   # not a legal choice for this shape: rejected before any launch
                        _sync()
                        key = (n, tup, learned, pitch, v, ks)
                        path = _path(lib, _lib.OP_CONV_EPILOGUE)
                        assert ks < 1 or path == (_lib.PATH_FUSED if ks >= 2 else _lib.PATH_NOT_FUSED), key
                        if path == _lib.PATH_FUSED:
                            fused += 1
                            FUSED_SEEN.add(("upsample", n % 4, tup % 2))
                        y.check_footprint(("conv output", key))
                        up.check_footprint(("fused upsampling", key))
                        yg, ug = y.get((BATCH, COUT, n)), up.get((BATCH, COUT, tup))
                        assert np.abs(yg - y64).max() <= E.CONV_TOL * max(1.0, np.abs(y64).max()), key
                        err = float(np.abs(ug - ref).max()) / max(1.0, float(np.abs(ref).max()))
                        worst = max(worst, err)
                        assert err <= E.OP_TOL, (key, err)
                        # the stand-alone kernel on the conv output this very launch stored
                        _lib.check(lib.wun_op_upsample(y.ptr, alone.ptr, iwd.data_ptr() if learned else None, BATCH, COUT, n, tup, n,
                                                       pitch, 0, _stream()))
                        _sync()
                        ag = alone.get((BATCH, COUT, tup))
                        if not learned:
                            assert np.array_equal(ug, ag), key
                        else:
                            _, mag, _ = E.upsample_ref(yg, iw, tup)
                            assert np.all(np.abs(ug - ag) <= 4 * E.EPS32 * mag), key           # one rounding of s a + (1 - s) b each
                        for rows in (y, up, alone):
                            rows.reset()
    finally:
        lib.wun_op_force_conv_variant(-1, 0)
        lib.wun_op_set_conv_upsample(None, 0, 0, None)
    record("op_fused_upsample", "n%d cout%d rel" % (n, COUT), worst, E.OP_TOL)
    assert fused >= 8, fused


@pytest.mark.parametrize("NSK,NCUR", [(3, 5), (5, 11)])
@pytest.mark.parametrize("n", FUSED_N)
def test_fused_upsampling_adjoint_in_the_split_k_epilogue(lib, n, NSK, NCUR):
    """The input gradient of an up conv over concat(skip, upsampled): the split-K epilogue applies the adjoint of the linear
    upsampling to the last n_cur columns.  Against float64, and bit for bit against the same (variant, split) launch with one
    destination followed by wun_op_upsample_backward."""
    rng = np.random.default_rng(1000 + n + 7 * NCUR)
    worst = fused = 0
    try:
        for tup in (2 * n - 1, 2 * n):
            dz = rng.uniform(-1, 1, (BATCH, CIN, tup + KW - 1)).astype(np.float32)
            wt_ = (rng.uniform(-1, 1, (KW, CIN, NSK + NCUR)) / np.sqrt(KW * CIN)).astype(np.float32)
            xprev, _, _ = E.ups_inputs(BATCH, NCUR, n, tup, 0, 0)
            g64 = _conv64(dz, wt_, None, False)
            r = E.upsample_backward_ref(g64[:, NSK:], xprev, None, tup)
            dzd, wd = torch.tensor(dz, device="cuda"), torch.tensor(wt_, device="cuda")
            for pp in (_pad(n, 4) + 4, n):
                xr = Rows(BATCH * NCUR, n, pp, 0, False, xprev)
                dsk, dup, dzp = Rows(BATCH * NSK, tup, tup), Rows(BATCH * NCUR, tup, tup), Rows(BATCH * NCUR, n, pp)
                full, alone = Rows(BATCH * (NSK + NCUR), tup, tup), Rows(BATCH * NCUR, n, pp)
                for v, ks in _choices(lib):
                    lib.wun_op_force_conv_variant(v, ks)
                    rc = lib.wun_op_conv1d_upsample_adjoint(dzd.data_ptr(), wd.data_ptr(), dsk.ptr, dup.ptr, dzp.ptr, xr.ptr, BATCH, CIN,
                                                            NSK, NCUR, KW, tup + KW - 1, tup, 0, n, pp, _stream())
                    if rc != 0:
                        continue
                    _sync()
                    key = (n, tup, pp, v, ks)
                    path = _path(lib, _lib.OP_CONV_EPILOGUE)
                    assert ks < 1 or path == (_lib.PATH_FUSED if ks >= 2 else _lib.PATH_NOT_FUSED), key
                    dsk.check_footprint(("d_skip", key))
                    dzp.check_footprint(("fused adjoint", key))
                    if path == _lib.PATH_FUSED:
                        fused += 1
                        FUSED_SEEN.add(("adjoint", n % 4, tup % 2))
                        assert torch.isnan(dup.buf).all(), ("d_up written by a fused launch", key)
                    else:
                        dup.check_footprint(("d_up", key))
                    got = dzp.get((BATCH, NCUR, n))
                    assert np.abs(dsk.get((BATCH, NSK, tup)) - g64[:, :NSK]).max() <= E.CONV_TOL * max(1.0, np.abs(g64).max()), key
                    err = float(np.abs(got - r["dz"]).max()) / max(1.0, float(np.abs(r["dz"]).max()))
                    worst = max(worst, err)
                    assert err <= E.OP_TOL, (key, err)
                    # the same launch with one destination, then the stand-alone adjoint
                    _lib.check(lib.wun_op_conv1d_ex(dzd.data_ptr(), CIN, None, 0, wd.data_ptr(), None, full.ptr, None, BATCH, NSK + NCUR,
                                                    KW, tup + KW - 1, tup, tup, 1, 0, 0, 0, 1, 0, _stream()))
                    _sync()
                    fg = full.get((BATCH, NSK + NCUR, tup))
                    assert np.array_equal(dsk.get((BATCH, NSK, tup)), fg[:, :NSK]), key
                    dyr = Rows(BATCH * NCUR, tup, tup, 0, False, fg[:, NSK:])
                    _lib.check(lib.wun_op_upsample_backward(dyr.ptr, xr.ptr, alone.ptr, None, None, None, BATCH, NCUR, n, tup, tup, pp,
                                                            0, 0, _stream()))
                    _sync()
                    assert np.array_equal(got, alone.get((BATCH, NCUR, n))), key
                    for rows in (dsk, dup, dzp, full, alone):
                        rows.reset()
    finally:
        lib.wun_op_force_conv_variant(-1, 0)
    record("op_fused_upsample_adjoint", "n%d ncur%d rel" % (n, NCUR), worst, E.OP_TOL)
    assert fused >= 4, fused


# ---------------------------------------------------------------------------------------------------------------------------
# coverage: these run last
# ---------------------------------------------------------------------------------------------------------------------------
def test_bf16_rows_rarely_differ_from_the_once_rounded_reference():
    """Pooled over all cases of a test function: a store that truncated instead of rounding to nearest even would change about
    half of the inexact elements by one spacing while passing the per-element bound."""
    for name in ("test_upsample_forward", "test_upsample_backward_and_interp_grad", "test_head_forward_loss_and_gradients"):
        differ, total = POOL[name]
        record("bf16_differ_share", name, differ / total, E.BF16_DIFF_SHARE)
        assert total > 100000 and differ / total <= E.BF16_DIFF_SHARE, (name, differ, total)


def test_every_fused_residue_was_exercised():
    want = {(kind, r, p) for kind in ("upsample", "adjoint") for r in range(4) for p in (0, 1)}
    assert FUSED_SEEN >= want, sorted(want - FUSED_SEEN)


def test_every_form_of_every_operator_was_exercised():
    L = _lib
    want = {L.OP_UPSAMPLE: {L.PATH_SCALAR, L.PATH_VEC4, L.PATH_VEC8_BF16},
            L.OP_UPSAMPLE_BACKWARD: {L.PATH_SCALAR, L.PATH_VEC4},
            L.OP_INTERP_GRAD: {L.PATH_ONE_STAGE, L.PATH_TWO_STAGE},
            L.OP_HEAD_FORWARD: {L.PATH_GENERIC, L.PATH_FOUR_POSITION},
            L.OP_HEAD_DFEAT: {L.PATH_GENERIC, L.PATH_FOUR_POSITION},
            L.OP_CONV_EPILOGUE: {L.PATH_NOT_FUSED, L.PATH_FUSED},
            L.OP_BTC_TO_NCW: {L.PATH_SCALAR, L.PATH_VEC4}}
    for op, forms in want.items():
        assert SEEN[op] == forms, (op, SEEN[op], forms)
