"""The weight-gradient kernels in the forms the PLAN launches them (run with -m gpu on an MI355X), through wun_op_wgrad_ex:
two virtual sources with crop offsets, windows inside longer rows, the two-part launches of a down level into one partial
buffer, the direct epilogue, the accumulating instantiations, the 4- and 16-lane split reductions, bf16 rows the caller made,
and the narrow kernels' plane / two-part / bf16 forms -- none of which wun_op_conv1d_wgrad (one repacked source at offset 0, one
part, always the split reduction, never accumulating) can reach.

Every launch reads views of ONE arena: a row's window holds uniform(-1, 1), everything else in the row (before the window,
behind it, the pitch padding, dz beyond Tq) finite values around 1e4, so one foreign element in a sum misses by orders of
magnitude; grads sits between guard bands that are compared bit for bit after every launch, and starts as NaN (storing launches)
or as a random prior (accumulating ones).  Storing launches are compared with the float64 reference of tests/_wgrad_np.py (bf16
launches: on the bf16 values the rows hold) at OP_TOL x max(1, max|ref|), weights and bias separately; an accumulating launch
must equal float32 prior + stored BIT FOR BIT (grad_acc_add), where `stored` is what the same launch -- family,
geometry, split counts -- wrote without the flag.  The last test asserts, from what the entry reported, that every reachable cell
of {direct, split} x {store, accumulate} x {one, two sources} x {one, two parts} ran for every kernel family."""
import ctypes as C

import numpy as np
import pytest
import torch

import _wgrad_np as W
from _observed import record

pytestmark = pytest.mark.gpu

from wave_u_net_amd import _lib                   # noqa: E402

OP_TOL = 2e-5            # x max(1, max|ref|): the neighbouring operator tests' value (B * Tq <= 2800, K * Cin <= 3000)
BAND = 64                # guard floats on either side of grads
BAND_BITS = 0x5A17C0DE
SCRATCH_CAP = 1 << 21    # floats of the arena kept for split partials
UNSUPPORTED, INVALID = -2, -1

F32_GEOMS = [(0, 0)] + [(m, n) for m in (1, 2, 4) for n in (1, 2, 3, 4, 5)] + [(6, 1), (6, 2), (6, 3)]
BF16_GEOMS = [(0, 0)] + [(4, n) for n in (1, 2, 3, 4, 5)] + [(8, n) for n in (1, 2, 3)]
MFMA_FAMILIES = (W.LDS, W.WIN, W.BF16)

# family -> {(path, accumulate, sources, parts)} as the entry reported them
_RAN = {f: set() for f in (W.LDS, W.WIN, W.BF16, W.NARROW)}
_FAULT = []              # a HIP error met by a launch: nothing more is started on the device by this module


def geoms_of(family, K):
    if family == W.LDS:
        return F32_GEOMS
    if family == W.BF16:
        return BF16_GEOMS
    return [(0, 0)] + [(1, nw) for nw in range(1, 6 if K == 15 else 7)] + [(2, 0)]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _align(n, a):
    return (n + a - 1) // a * a


def _region(a, bf):
    """A numpy float32 array as the flat float32 tensor that holds it in the arena (bf16 elements: two per float)."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).reshape(-1)
    if not bf:
        return t
    t = t.to(torch.bfloat16)
    if t.numel() % 2:
        t = torch.cat([t, torch.zeros(1, dtype=torch.bfloat16)])
    return t.view(torch.float32)


class Job:
    """One launch shape with its inputs in an arena on the device, its reference, and the launches made on it."""

    def __init__(self, lib, shape, family, seed, et=0, galign=0):
        assert not _FAULT, "an earlier launch of this module met a HIP error: %s" % _FAULT[0]
        self.lib, self.shape, self.family, self.et = lib, shape, family, et
        bf = family == W.BF16
        self.bf = (bf, bf or bool(et & 2), bf or bool(et & 4))
        self.x0, self.x1, self.dzs = W.make_inputs(shape, seed, *self.bf)
        K, Ct, N, planes = shape["K"], shape["C0"] + shape["C1"], shape["N"], shape["planes"]
        B, Nper = shape["B"], N // planes
        self.ref_w, self.ref_b = W.reference(self.x0, self.x1, self.dzs, K, shape["parts"])
        self.sw, self.sb = max(1.0, np.abs(self.ref_w).max()), max(1.0, np.abs(self.ref_b).max())
        # ---- grads: per plane {weights [K][Ct][Nper], bias [Nper]}; several planes: in reverse order with gaps nobody owns
        blk, gap = K * Ct * Nper + Nper, (0 if planes == 1 else 5)
        self.plane_off = [(planes - 1 - s) * (blk + gap) for s in range(planes)]
        self.G = planes * (blk + gap) - gap
        ref = np.full(self.G, np.nan)
        self.wmask, self.bmask = np.zeros(self.G, dtype=bool), np.zeros(self.G, dtype=bool)
        for s, off in enumerate(self.plane_off):
            ref[off:off + K * Ct * Nper] = self.ref_w[:, :, s * Nper:(s + 1) * Nper].reshape(-1)
            ref[off + K * Ct * Nper:off + blk] = self.ref_b[s * Nper:(s + 1) * Nper]
            self.wmask[off:off + K * Ct * Nper] = True
            self.bmask[off + K * Ct * Nper:off + blk] = True
        self.ref = ref
        self.owned = torch.from_numpy(self.wmask | self.bmask)
        self.prior = torch.from_numpy(np.random.default_rng(seed + 1000).uniform(-2, 2, self.G).astype(np.float32))
        # ---- dz planes: plane s of a part at + s * zss elements (a gap of 8 behind every plane)
        self.zss = [0 if planes == 1 else B * Nper * p["dz_pitch"] + 8 for p in shape["parts"]]
        assert len(set(self.zss)) == 1
        dzflat = []
        for p, z, zss in zip(shape["parts"], self.dzs, self.zss):
            if planes == 1:
                dzflat.append(z)
                continue
            per = B * Nper * p["dz_pitch"]
            flat = np.full((planes - 1) * zss + per, 0.75 * W.FILL, dtype=np.float32)
            for s in range(planes):
                flat[s * zss:s * zss + per] = z[:, s * Nper:(s + 1) * Nper, :].reshape(-1)
            dzflat.append(flat)
        # ---- the arena: [rows of x0][x1][dz per part] ... [band][grads][band] ... [scratch]
        regs = [_region(self.x0, self.bf[0])]
        if self.x1 is not None:
            regs.append(_region(self.x1, self.bf[1]))
        regs += [_region(z, self.bf[2]) for z in dzflat]
        pos, offs = 16, []
        for r in regs:
            pos = _align(pos, 4)
            offs.append(pos)
            pos += r.numel() + 8
        self.g0 = _align(pos, 4) + BAND + galign            # galign = 1: a block that is not 16-byte aligned
        self.s0 = _align(self.g0 + self.G + BAND, 64)
        self.arena = torch.full((self.s0 + SCRATCH_CAP + 64,), 7777.0, dtype=torch.float32, device="cuda")
        for r, off in zip(regs, offs):
            self.arena[off:off + r.numel()].copy_(r)
        self.band = torch.full((BAND,), BAND_BITS, dtype=torch.int32)
        for lo in (self.g0 - BAND, self.g0 + self.G):
            self.arena[lo:lo + BAND].view(torch.int32).fill_(BAND_BITS)
        base = self.arena.data_ptr()
        ptrs = [base + 4 * off for off in offs]
        self.p_x0 = ptrs.pop(0)
        self.p_x1 = ptrs.pop(0) if self.x1 is not None else None
        self.p_dz = ptrs + [None] * (2 - len(ptrs))
        self.p_g, self.p_s = base + 4 * self.g0, base + 4 * self.s0
        self.nsrc = 2 if shape["C1"] else 1
        self.nparts = len(shape["parts"])

    def desc(self, nsplit=(0, 0), accumulate=0, force=(0, 0)):
        sh, d = self.shape, _lib.WunOpWgradDesc()
        d.family, d.B, d.C0, d.C1, d.N, d.K = self.family, sh["B"], sh["C0"], sh["C1"], sh["N"], sh["K"]
        d.x0_pitch, d.x1_pitch, d.rows_bf16, d.nparts = sh["x0_pitch"], sh["x1_pitch"], int(self.family == W.BF16), self.nparts
        for i, p in enumerate(sh["parts"]):
            d.loader[i], d.x0_off[i], d.x1_off[i], d.Tin[i] = p["loader"], p["x0_off"], p["x1_off"], p["Tin"]
            d.shift[i], d.Tq[i], d.dz_pitch[i], d.nsplit[i] = p["shift"], p["Tq"], p["dz_pitch"], nsplit[i]
        d.accumulate, d.force_mtw, d.force_nw = accumulate, force[0], force[1]
        if self.family == W.NARROW:
            d.planes, d.zss, d.et = sh["planes"], self.zss[0], self.et
            for s, off in enumerate(self.plane_off):
                d.plane_off[s] = off
        return d

    def set_grads(self, t):
        self.arena[self.g0:self.g0 + self.G].copy_(t)

    def read(self):
        """grads as a CPU tensor, after asserting both guard bands bit for bit."""
        try:
            torch.cuda.synchronize()
            reg = self.arena[self.g0 - BAND:self.g0 + self.G + BAND].cpu()
        except RuntimeError as e:
            _FAULT.append(str(e))
            raise
        assert torch.equal(reg[:BAND].view(torch.int32), self.band), "guard band below grads was written"
        assert torch.equal(reg[BAND + self.G:].view(torch.int32), self.band), "guard band above grads was written"
        return reg[BAND:BAND + self.G].clone()

    def launch(self, d):
        """-> (rc, path, total splits).  Scratch starts as NaN: a partial nobody wrote would surface."""
        need = int(self.lib.wun_op_wgrad_ex_scratch(C.byref(d)))
        if need < 0:
            return need, 0, 0
        assert need <= SCRATCH_CAP, need
        self.arena[self.s0:self.s0 + need].fill_(float("nan"))
        rc = self.lib.wun_op_wgrad_ex(C.byref(d), self.p_x0, self.p_x1, self.p_dz[0], self.p_dz[1], self.p_g, self.p_s, _stream())
        if rc == -3:
            _FAULT.append(self.lib.wun_last_error().decode("utf-8", "replace"))
        return rc, self.lib.wun_op_last_path(_lib.OP_WGRAD), self.lib.wun_op_wgrad_last_splits()

    def refused(self, d, code, ptrs=None):
        """The launch is refused with `code` and grads (NaN before) and the bands keep their bits."""
        nan = torch.full((self.G,), float("nan"))
        self.set_grads(nan)
        p = dict(x0=self.p_x0, x1=self.p_x1, dz0=self.p_dz[0], dz1=self.p_dz[1], g=self.p_g, s=self.p_s)
        p.update(ptrs or {})
        rc = self.lib.wun_op_wgrad_ex(C.byref(d), p["x0"], p["x1"], p["dz0"], p["dz1"], p["g"], p["s"], _stream())
        assert rc == code, (rc, code, self.lib.wun_last_error())
        assert torch.equal(self.read().view(torch.int32), nan.view(torch.int32))

    def store_and_accumulate(self, nsplit=(0, 0), force=(0, 0)):
        """One storing launch against the reference, then the same launch accumulating onto the prior, bit for bit.
        -> None when the forced geometry does not resolve, else (error, why it fails or None, path, splits)."""
        nan = torch.full((self.G,), float("nan"))
        self.set_grads(nan)
        rc, path, splits = self.launch(self.desc(nsplit, 0, force))
        if rc == UNSUPPORTED and force != (0, 0):
            assert torch.equal(self.read().view(torch.int32), nan.view(torch.int32))
            return None
        _lib.check(rc)
        stored = self.read()
        got = stored.numpy().astype(np.float64)
        why = None
        if not np.isfinite(got[self.wmask | self.bmask]).all():
            return float("inf"), "non-finite gradient", path, splits
        if not torch.equal(stored[~self.owned].view(torch.int32), nan[~self.owned].view(torch.int32)):
            why = "an element between the planes' blocks was written"
        ew = np.abs(got[self.wmask] - self.ref[self.wmask]).max() / self.sw
        eb = np.abs(got[self.bmask] - self.ref[self.bmask]).max() / self.sb
        if max(ew, eb) > OP_TOL:
            why = "weights %.3e bias %.3e above OP_TOL" % (ew, eb)
        _RAN[self.family].add((path, 0, self.nsrc, self.nparts))
        # ---- accumulate
        self.set_grads(self.prior)
        rc, apath, asplits = self.launch(self.desc(nsplit, 1, force))
        _lib.check(rc)
        acc = self.read()
        want = self.prior.clone()
        want[self.owned] = self.prior[self.owned] + stored[self.owned]                      # float32, one rounding
        if (apath, asplits) != (path, splits):
            why = "the accumulating launch took path %d with %d splits, the storing one %d with %d" % (apath, asplits, path, splits)
        elif not torch.equal(acc.view(torch.int32), want.view(torch.int32)):
            nbad = int((acc.view(torch.int32) != want.view(torch.int32)).sum())
            why = "accumulate: %d of %d floats differ from prior + stored" % (nbad, self.G)
        _RAN[self.family].add((apath, 1, self.nsrc, self.nparts))
        return max(ew, eb), why, path, splits


def sweep(job, splits_list, expect=None, min_ran=1):
    """Every geometry of the family that resolves x the split requests.  -> worst error; asserts after all figures are in.
    expect(nsplit, path, splits): an assertion on what the entry reported."""
    fails, worst, ran = [], 0.0, 0
    for force in geoms_of(job.family, job.shape["K"]):
        for ns in splits_list:
            r = job.store_and_accumulate(ns, force)
            if r is None:
                continue
            err, why, path, splits = r
            worst, ran = max(worst, err), ran + 1
            if why:
                fails.append((force, ns, why))
            if expect is not None:
                expect(job, ns, force, path, splits)
    assert ran >= min_ran, ran
    return worst, fails


def granted(job, nsplit, force=(0, 0)):
    """The total split count the entry must report for explicit requests: min(request, work units) per part."""
    d = job.desc(nsplit, 0, force)
    total = 0
    for i in range(job.nparts):
        units = job.lib.wun_op_wgrad_max_units(C.byref(d), i)
        assert units >= 1, units
        total += min(nsplit[i], units)
    return total


def expect_requested(job, ns, force, path, splits):
    if all(n > 0 for n in ns[:job.nparts]):
        want = granted(job, ns, force)
        assert splits == want, (ns, force, splits, want)
    assert path == (_lib.PATH_WGRAD_DIRECT if splits == 1 else _lib.PATH_WGRAD_SPLIT), (ns, force, path, splits)


def finish(name, what, worst, fails):
    record(name, what, worst, OP_TOL)
    for f in fails:
        print("[parity] %s %s FAILS: %s" % (name, what, (f,)))
    assert not fails, (len(fails), fails[:4], fails[-4:])
    if worst > OP_TOL / 3:
        print("[parity] %s %s: observed error %.3e is within 3x of OP_TOL" % (name, what, worst))


# ---- up convs: concat(crop(skip), upsampled), every offset pair, every family that serves the shape ----
UP_DIMS = [W.UP_MAIN] + sorted({d for d, _ in W.UP_OTHER}, key=lambda d: -d[1])


@pytest.mark.parametrize("family", MFMA_FAMILIES, ids=[W.FAMILY_NAMES[f] for f in MFMA_FAMILIES])
@pytest.mark.parametrize("dims", UP_DIMS, ids=[str(d) for d in UP_DIMS])
def test_up_conv_two_sources_with_crop_offsets(lib, dims, family):
    """delta0 != delta1, row tiles and channel pairs that straddle the two sources, windows inside longer rows."""
    offsets = W.UP_OFFSETS if dims == W.UP_MAIN else [o for d, o in W.UP_OTHER if d == dims]
    shapes = [W.up_shape(*dims, a, b) for a, b in offsets]
    if dims == W.UP_MAIN:
        shapes.append(W.up_shape(*dims, 0, 0, shift=2))           # 'same' padding: zero columns on both sides
    worst, fails = 0.0, []
    for i, shape in enumerate(shapes):
        job = Job(lib, shape, family, seed=100 * UP_DIMS.index(dims) + i, galign=i & 1)
        if dims == (2, 7, 9, 24, 5, 77) and family == W.BF16:
            # an odd C0 with two sources: a staged channel pair would straddle them -- refused, not computed
            job.refused(job.desc(), UNSUPPORTED)
            continue
        w, f = sweep(job, [(0, 0), (1, 0), (3, 0)], expect_requested, min_ran=6)
        worst, fails = max(worst, w), fails + [(offsets[i] if i < len(offsets) else "same",) + x for x in f]
    finish("wgrad_ops_up_conv_two_sources", "%s %s" % (W.FAMILY_NAMES[family], dims), worst, fails)


# ---- the short deep levels: one split in all, the direct epilogue ----
@pytest.mark.parametrize("family", MFMA_FAMILIES, ids=[W.FAMILY_NAMES[f] for f in MFMA_FAMILIES])
@pytest.mark.parametrize("dims", W.DEEP, ids=[str(d) for d in W.DEEP])
def test_deep_level_direct_epilogue(lib, dims, family):
    def direct(job, ns, force, path, splits):
        if ns[0] == 1:
            assert (path, splits) == (_lib.PATH_WGRAD_DIRECT, 1), (force, path, splits)
        expect_requested(job, ns, force, path, splits)

    worst, fails = 0.0, []
    for i, (a, b) in enumerate(W.DEEP_OFFSETS):
        job = Job(lib, W.deep_shape(*dims, a, b if dims[2] else 0), family, seed=700 + 10 * W.DEEP.index(dims) + i, galign=i)
        w, f = sweep(job, [(1, 0), (0, 0)], direct, min_ran=4)
        worst, fails = max(worst, w), fails + [((a, b),) + x for x in f]
    finish("wgrad_ops_deep_level_direct", "%s %s" % (W.FAMILY_NAMES[family], dims), worst, fails)


# ---- a down level: two parts into one partial buffer, one reduction ----
DOWN_FORMS = [("direct", 9), ("direct", 10), ("dedup", 0)]


@pytest.mark.parametrize("family", MFMA_FAMILIES, ids=[W.FAMILY_NAMES[f] for f in MFMA_FAMILIES])
@pytest.mark.parametrize("form", DOWN_FORMS, ids=["%s%d" % f for f in DOWN_FORMS])
def test_down_level_two_parts(lib, form, family):
    """Part 0 = the decimated positions (de-interleaving loader); part 1 = the skip-window positions (direct loader at
    off = cs) or the odd positions (de-interleaving loader at off = 11): consecutive splits through split_base."""
    def two(job, ns, force, path, splits):
        assert path == _lib.PATH_WGRAD_SPLIT and splits >= 2, (ns, force, path, splits)
        expect_requested(job, ns, force, path, splits)

    job = Job(lib, W.down_shape(*form), family, seed=900 + DOWN_FORMS.index(form), galign=DOWN_FORMS.index(form) & 1)
    worst, fails = sweep(job, [(1, 1), (0, 0), (3, 2)], two, min_ran=3)
    finish("wgrad_ops_down_level_two_parts", "%s %s%d" % ((W.FAMILY_NAMES[family],) + form), worst, fails)


@pytest.mark.parametrize("family", MFMA_FAMILIES, ids=[W.FAMILY_NAMES[f] for f in MFMA_FAMILIES])
def test_down_level_first_part_alone(lib, family):
    """One split of the decimated positions alone: the direct epilogue behind the de-interleaving loader; and the library's
    own split count."""
    def alone(job, ns, force, path, splits):
        if ns[0] == 1:
            assert (path, splits) == (_lib.PATH_WGRAD_DIRECT, 1), (force, path, splits)
        expect_requested(job, ns, force, path, splits)

    job = Job(lib, W.down_shape("alone"), family, seed=950)
    worst, fails = sweep(job, [(1, 0), (0, 0), (2, 0)], alone, min_ran=3)
    finish("wgrad_ops_down_level_first_part_alone", W.FAMILY_NAMES[family], worst, fails)


# ---- few tiles, many splits: the 4- and 16-lane split reductions ----
REDUCE_CASES = [(W.BF16, 16, 8, 4), (W.BF16, 32, 64, 16), (W.LDS, 16, 8, 4), (W.LDS, 32, 64, 16), (W.WIN, 16, 16, 4), (W.WIN, 32, 64, 4),
                (W.WIN, 32, 128, 16)]


@pytest.mark.parametrize("case", REDUCE_CASES, ids=["%s B%d ask%d" % (W.FAMILY_NAMES[c[0]], c[1], c[2]) for c in REDUCE_CASES])
def test_split_reduction_widths(lib, case):
    """(Cin, N, K) = (24, 16, 5), Tq = 130: one row group x one column group (1024 accumulator vectors per split, far below the
    2^16 / 2^18 of the launchers' rule), two units of 128 positions per excerpt.  wgrad_bf16_reduce_kernel / wgrad_reduce_kernel
    spread the splits over 4 lanes from 8 splits and over 16 from 64; wgrad_win_reduce_kernel over 4 from 16 and over 16 from 128.  The assertion is
    on what the entry GRANTED (min(request, work units)), which must reach the width's threshold.
    B = 32 x Tq = 130 is above the 2800 positions the other cases keep to: the case is the stated one, the tolerance unchanged."""
    family, B, ask, lanes = case
    job = Job(lib, W.reduce_shape(B), family, seed=1200 + B)
    want = granted(job, (ask, 0))
    floor = {(W.BF16, 4): 8, (W.BF16, 16): 64, (W.LDS, 4): 8, (W.LDS, 16): 64, (W.WIN, 4): 16, (W.WIN, 16): 128}[(family, lanes)]
    assert want >= floor and (lanes == 16 or want < (128 if family == W.WIN else 64)), (want, floor)
    err, why, path, splits = job.store_and_accumulate((ask, 0))
    assert (path, splits) == (_lib.PATH_WGRAD_SPLIT, want), (path, splits, want)
    finish("wgrad_ops_split_reduction_widths", "%s B%d granted %d" % (W.FAMILY_NAMES[family], B, splits), err, [why] if why else [])


# ---- the narrow kernels' plan-only forms ----
HEAD_CASES = [(K, planes, et) for K in (1, 3) for planes in (2, 4) for et in (0, 2)]


@pytest.mark.parametrize("case", HEAD_CASES, ids=["K%d planes%d et%d" % c for c in HEAD_CASES])
def test_narrow_head_two_sources_and_planes(lib, case):
    """The output head: fp32 audio cropped at 37 + the feature map (fp32, or bf16: et = 2), dz planes zss apart, one gradient
    block per plane at its own offset (reverse order, gaps between them that keep their bits)."""
    K, planes, et = case
    job = Job(lib, W.head_shape(K, planes, x1_off=0 if K == 1 else 3), W.NARROW, seed=1300 + HEAD_CASES.index(case), et=et, galign=planes == 4)
    fails = []
    worst = 0.0
    for ns in ((0, 0), (3, 0)):
        err, why, path, splits = job.store_and_accumulate(ns)
        assert path == _lib.PATH_WGRAD_SPLIT and splits >= 1
        worst, fails = max(worst, err), fails + ([(ns, why)] if why else [])
    finish("wgrad_ops_narrow_head", "K%d planes%d et%d" % case, worst, fails)


AUDIO_CASES = [(Cc, et, two) for Cc in (1, 2) for et in (0, 4) for two in (True, False)]


@pytest.mark.parametrize("case", AUDIO_CASES, ids=["C%d et%d %s" % (c[0], c[1], "two parts" if c[2] else "part 0") for c in AUDIO_CASES])
def test_narrow_audio_input_conv(lib, case):
    """The audio-input conv, mono and stereo: the stride-2 positions over rows of 5000, then stride-1 positions at an odd offset,
    consecutive splits of one partial list; fp32 dz, or bf16 dz (et = 4).  Part 0 alone is the one-part form."""
    Cc, et, two = case
    job = Job(lib, W.audio_shape(Cc, two), W.NARROW, seed=1400 + AUDIO_CASES.index(case), et=et)
    fails, worst = [], 0.0
    for ns in ((0, 0), (4, 1), (1, 1)):
        err, why, path, splits = job.store_and_accumulate(ns)
        assert path == _lib.PATH_WGRAD_SPLIT
        if ns[0]:
            assert splits == granted(job, ns), (ns, splits)
        worst, fails = max(worst, err), fails + ([(ns, why)] if why else [])
    finish("wgrad_ops_narrow_audio", "C%d et%d parts%d" % (Cc, et, 2 if two else 1), worst, fails)


# ---- refusals: by return code, before any GPU work, grads untouched ----
def test_refusals_leave_grads_untouched(lib):
    up = Job(lib, W.up_shape(*W.UP_MAIN, 1, 2), W.LDS, seed=1)

    def edited(job, **kw):
        d = job.desc()
        for k, v in kw.items():
            if isinstance(v, tuple):
                for i, x in enumerate(v):
                    getattr(d, k)[i] = x
            else:
                setattr(d, k, v)
        return d

    up.refused(edited(up, Tin=(up.shape["x0_pitch"], 0)), INVALID)                # window beyond its pitch
    up.refused(edited(up, x0_pitch=up.shape["x0_pitch"] + 2), INVALID)            # pitch not a multiple of 4
    up.refused(edited(up, rows_bf16=1), INVALID)                                  # bf16 rows on an fp32 family
    up.refused(edited(up, nparts=3), INVALID)
    up.refused(edited(up, shift=(5, 0)), INVALID)                                 # shift >= K
    up.refused(edited(up), INVALID, dict(x0=up.p_x0 + 4))                         # x0 off 16 bytes
    up.refused(edited(up), INVALID, dict(x1=None))                                # a second source without rows
    up.refused(edited(up, shift=(2, 0)), UNSUPPORTED)                             # shift > 0 with window offsets: never built
    up.refused(edited(up, force_mtw=6, force_nw=5), UNSUPPORTED)                  # 30 accumulator tiles: resolves to (4, 5)
    up.refused(edited(up, family=W.NARROW, planes=1), UNSUPPORTED)                # 48 x 40 (channel, row) pairs
    # two parts with two sources: never built
    two = edited(up, nparts=2)
    for k in ("loader", "x0_off", "x1_off", "Tin", "shift", "Tq", "dz_pitch"):
        getattr(two, k)[1] = getattr(two, k)[0]
    up.refused(two, UNSUPPORTED, dict(dz1=up.p_dz[0]))
    # the window kernel: taps other than 15 / 5; 15 taps with C0 % 8 != 0 in front of a second source
    win9 = Job(lib, W.up_shape(2, 24, 0, 32, 9, 60, 0, 0), W.WIN, seed=2)
    win9.refused(win9.desc(), UNSUPPORTED)
    win15 = Job(lib, W.up_shape(2, 36, 12, 48, 15, 60, 0, 0), W.WIN, seed=3)
    win15.refused(win15.desc(), UNSUPPORTED)
    # the narrow family: unknown et bits; an element-type mix no kernel is instantiated for (bf16 audio)
    head = Job(lib, W.head_shape(1, 2), W.NARROW, seed=4)
    head.refused(edited(head, et=8), INVALID)
    head.refused(edited(head, et=1), UNSUPPORTED)
    head.refused(edited(head, planes=3), INVALID)                                 # 3 planes do not divide 4 rows
    head.refused(edited(head, force_nw=2), INVALID)


# ---- coverage, from what the entry reported ----
def test_every_reachable_form_ran_for_every_family(lib):
    """{direct, split} x {store, accumulate} x {one, two sources} x {one, two parts} per family.  Cells no launch can reach:
      * direct with two parts (every family): two parts are at least two splits, and the direct epilogue runs at one;
      * two sources with two parts (every family): no layer of the plan launches it (a down level has one input tensor), the
        entry refuses it (test_refusals_leave_grads_untouched);
      * direct, narrow family: the narrow kernels always write partials, their reduction writes the block."""
    D, S = _lib.PATH_WGRAD_DIRECT, _lib.PATH_WGRAD_SPLIT
    missing = []
    for family in (W.LDS, W.WIN, W.BF16, W.NARROW):
        for path in (D, S):
            for acc in (0, 1):
                for nsrc in (1, 2):
                    for nparts in (1, 2):
                        reachable = not (path == D and nparts == 2) and not (nsrc == 2 and nparts == 2) and \
                            not (path == D and family == W.NARROW)
                        ran = (path, acc, nsrc, nparts) in _RAN[family]
                        assert reachable or not ran, (family, path, acc, nsrc, nparts)
                        if reachable and not ran:
                            missing.append((W.FAMILY_NAMES[family], "direct" if path == D else "split", acc, nsrc, nparts))
    assert not missing, missing
