"""Float64 references of the bf16 convs as single operators (wave-u-net_amd/csrc/wun_bf16.hip: conv_bf16_kernel in its three
modes and first_conv_kernel), the cases tests/test_gpu_bf16_ops.py runs them on, and the verdicts it asserts -- shared with
tests/test_bf16_ops_host.py, which judges MUTANT references by exactly those verdicts on exactly those cases.

  conv_ref        plain float64 conv (stride 1 / 2) or transposed stride-2 conv of the operands AS GIVEN (the callers hand over
                  bf16-valued arrays), bias included; per element also sum|terms|, the largest |term| and the term count
  epilogue_ref    what conv_out1 / conv_out_vec (wun_device.h) do with a finished value: LeakyReLU, mask (1 where the mask
                  operand is > 0, else 0.2f), accumulate inside [acc_lo, acc_lo + acc_len), the column split, the compact copy
                  of the even positions, one rounding to bf16 on a bf16 store
Mutants are keyword switches of the two (MUTANTS below says what each one breaks and where it applies)."""
import collections

import numpy as np

import _elementwise_np as E

SLOPE = float(np.float32(0.2))           # the kernels' 0.2f (LeakyReLU and its derivative mask)
PAD_VALUE = 1.0                          # what a mutant that admits a pad element reads there (the GPU tests put NaN there)
NCODES = 27                              # tile codes: (log2 MT) * 9 + (NW - 2) * 3 + (NCK - 1)
S1, S2, T2 = 0, 1, 2                     # modes: stride-1 loader, stride-2 loader, fused two-phase transposed stride-2 conv
FINE, COARSE = 1, 2                      # input grids of case_inputs / first_inputs


def code_tile(code):
    """-> (MT, NW, NCK)"""
    return 1 << (code // 9), 2 + (code // 3) % 3, 1 + code % 3


def kt_of(mode, taps):
    """The KT instantiation a launch of `taps` taps takes (conv_bf16_launch_m): taps = the launch's own count, which for the
    two-phase conv is (k + 1) / 2."""
    shipped = {S1: (15, 5), S2: (15,), T2: (8,)}[mode]
    return taps if taps in shipped else 0


# ---------------------------------------------------------------------------------------------------------------------------
# the reachable tile codes per mode and KT instantiation (derived from wun_op_conv_bf16_choice_ok by
# tests/test_bf16_ops_host.py over GRID below)
# ---------------------------------------------------------------------------------------------------------------------------
_M0 = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 13, 15, 16, 18, 19, 21, 22, 24, 25)
LEGAL = {
    (S1, 0): _M0,
    (S1, 5): _M0,
    (S1, 15): tuple(c for c in _M0 if c not in (8, 25)),
    (S2, 0): (0, 3, 6, 9, 12, 15, 18, 21, 24),
    (S2, 15): (0, 3, 6, 9, 12, 15, 18, 21, 24),
    (T2, 0): (0, 1, 2, 6, 7, 8, 9, 10, 15, 16, 18, 19, 24, 25),
    (T2, 8): (0, 1, 2, 6, 7, 8, 9, 10, 15, 16, 18, 19, 24, 25),
}
# the grid the host test searches: channels read x columns x length; taps per KT instantiation
GRID_C = (8, 16, 24, 40, 64, 72, 96, 136, 264)
GRID_N = (8, 12, 16, 24, 40, 48, 64, 72, 144)
GRID_T = (1, 17, 20, 64, 65, 129, 257, 1025)
GRID_TAPS = {(S1, 0): (1, 3, 4, 7, 9, 14), (S1, 5): (5,), (S1, 15): (15,), (S2, 0): (1, 4, 7, 9, 14), (S2, 15): (15,),
             (T2, 0): (1, 2, 3, 4, 7), (T2, 8): (8,)}


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
# mode; batch; channels read from source 0 / 1; columns (a.N) and split point N0; k = taps of the CONV (two-phase: of the forward
# conv whose input gradient this is -- the launch has (k + 1) / 2); Tin / Tout = row lengths read / written; shift = pad_left
Case = collections.namedtuple("Case", "mode B C0 C1 N N0 k Tin Tout shift")


def taps_of(c):
    return (c.k + 1) // 2 if c.mode == T2 else c.k


def _fwd(mode, C, N, k, Tout, shift=None, short=3, C1=0, N0=None, B=2):
    """A forward case whose input rows are `short` samples shorter than the taps reach on the right and `shift` on the left, so
    that zero fill is part of every case (a pad element admitted there changes the result)."""
    s = 2 if mode == S2 else 1
    shift = k // 2 if shift is None else shift
    need = (Tout - 1) * s + k - shift
    return Case(mode, B, C - C1, C1, N, N if N0 is None else N0, k, need - short, Tout, shift)


def _t2(C, N, k, Tout, B=2):
    """Input gradient of a valid stride-2 conv of k taps: rows read = (Tout - k) / 2 + 1 positions of dz."""
    return Case(T2, B, C, 0, N, N, k, (Tout - k) // 2 + 1, Tout, 0)


# batch 2; 129 positions: the shortest row that admits the 256-row tiles, a partial third 64-row tile; 40 columns: a partial
# last column tile for every NW; 72 channels: three stages at NCK = 1, one at NCK = 3; 24 channels: several groups for stride 2
SWEEP_CASES = (
    _fwd(S1, 72, 40, 5, 129), _fwd(S1, 72, 40, 7, 129), _fwd(S1, 40, 40, 15, 129), _fwd(S1, 72, 24, 15, 20),
    _fwd(S1, 40, 40, 7, 129), _fwd(S1, 40, 40, 5, 129), _fwd(S1, 8, 40, 15, 129),
    _fwd(S2, 8, 40, 15, 129), _fwd(S2, 8, 40, 7, 129), _fwd(S2, 24, 40, 15, 129), _fwd(S2, 24, 40, 7, 129),
    _t2(72, 16, 7, 257), _t2(40, 16, 15, 257), _t2(72, 16, 15, 39),
)
ODD_OFF, EVEN_OFF = 5, 0                 # first-element offsets of the input rows in the sweep

# store-path cases (test b): name -> (case, dict of epilogue options).  y_off: element offset of the first output inside its
# 16-byte aligned row (non-zero: the scalar stores); Tout = 0 / != 0 mod 4: vector stores with / without a scalar tail
StoreCase = collections.namedtuple("StoreCase", "name case code x_off y_off lrelu mask acc dec")
STORE_CASES = (
    StoreCase("s1_vec", _fwd(S1, 40, 40, 5, 132), 13, 0, 0, 1, 0, None, 1),
    StoreCase("s1_tail", _fwd(S1, 40, 40, 5, 129), 4, 3, 0, 1, 0, None, 1),
    StoreCase("s1_ties", _fwd(S1, 40, 40, 5, 129), 6, 1, 0, 0, 0, (0, 0), 1),
    StoreCase("s1_scalar", _fwd(S1, 40, 40, 5, 129), 0, 0, 3, 1, 0, None, 1),
    StoreCase("s1_two_sources", _fwd(S1, 40, 40, 5, 129, C1=16), 9, 1, 0, 0, 1, (30, 61), 0),
    StoreCase("s1_two_sources_scalar", _fwd(S1, 40, 40, 5, 130, C1=16), 1, 0, 2, 0, 1, (30, 61), 0),
    StoreCase("s1_split", _fwd(S1, 40, 40, 5, 129, N0=24), 3, 0, 0, 0, 1, (0, 0), 1),
    StoreCase("s1_split_scalar", _fwd(S1, 72, 40, 7, 129, N0=24), 2, 1, 1, 1, 0, None, 1),
    StoreCase("s2_vec", _fwd(S2, 24, 40, 15, 132), 12, 0, 0, 1, 0, None, 1),
    StoreCase("s2_tail", _fwd(S2, 24, 40, 7, 129), 3, 1, 0, 0, 1, (17, 40), 0),
    StoreCase("s2_scalar", _fwd(S2, 24, 40, 7, 129), 0, 0, 1, 1, 0, None, 1),
    StoreCase("t2_vec", _t2(40, 16, 15, 264), 9, 0, 0, 0, 1, (31, 100), 0),
    StoreCase("t2_tail", _t2(72, 16, 7, 257), 1, 1, 0, 0, 1, (0, 0), 0),
    StoreCase("t2_scalar", _t2(72, 16, 7, 257), 7, 0, 2, 0, 1, (31, 100), 0),
)


def store_grid(sc):
    """The input grid of a store case: COARSE (bf16 rounding ties) where no 0.2f product is involved, else FINE."""
    return FINE if (sc.lrelu or sc.mask) else COARSE


def _seed(*key):
    return E._seed(*key)


def case_inputs(c, grid=False, tag=0):
    """Operands of a case, all float64 arrays holding bf16 values (bias: fp32 values): x [B, C0 + C1, Tin], w -- forward modes
    [k, C0 + C1, N]; two-phase: the FORWARD conv's [k, N, C0] -- bias [N] (None for the two-phase conv), mask and prior
    [B, N, Tout] (the mask with +-0 in it).  grid: values on a dyadic grid on which every partial sum is exact in fp32, in any
    order (FINE: products are multiples of 2^-18 and partial sums stay far below 2^6) -- the fp32 conv result then IS the
    float64 one, and a bf16 store can differ from the once-rounded reference only through the 0.2f products and the accumulate
    add.  COARSE (multiples of 2^-9, for a case without 0.2f products): a large share of the results are exact TIES of the
    bf16 rounding, where nearest-even, nearest-away and truncation all part ways.  (With 0.2f products a coarse grid is no fair
    input: v / 5 lands on such ties, the float64 product with the fp32 constant 0.2f = 0.2 (1 + 1.5e-8) lies just above them
    and the fp32 product exactly on them -- 0.6 % of all elements differ by double rounding alone.  The FINE grid still has
    0.1 % of them where a 0.2f product acts on a bare grid sum; its bias is therefore an ordinary fp32 number, added last and
    rounded once, which leaves the bias-free two-phase conv's masked outputs as the only such elements.)"""
    rng = np.random.default_rng(_seed(*c, int(grid), tag))
    C = c.C0 + c.C1
    wshape = (c.k, c.N, c.C0) if c.mode == T2 else (c.k, C, c.N)
    if grid == COARSE:
        x = rng.integers(-8, 9, (c.B, C, c.Tin)) / 8.0
        w = rng.integers(-16, 17, wshape) / 64.0
        bias = rng.integers(-64, 65, c.N) / 128.0
        prior = rng.integers(-128, 129, (c.B, c.N, c.Tout)) / 64.0
    elif grid:
        x = rng.integers(-255, 256, (c.B, C, c.Tin)) / 256.0
        w = rng.integers(-255, 256, wshape) / 1024.0
        bias = rng.uniform(-0.1, 0.1, c.N).astype(np.float32).astype(np.float64)        # (off the grid: see below)
        prior = rng.integers(-255, 256, (c.B, c.N, c.Tout)) / 128.0
    else:
        x = E.bf16_round(rng.uniform(-1, 1, (c.B, C, c.Tin)).astype(np.float32))
        w = E.bf16_round((rng.uniform(-1, 1, wshape) / np.sqrt(taps_of(c) * C)).astype(np.float32))
        bias = rng.uniform(-0.1, 0.1, c.N).astype(np.float32).astype(np.float64)
        prior = E.bf16_round(rng.uniform(-1, 1, (c.B, c.N, c.Tout)).astype(np.float32))
    mask = E._with_zeros(E.bf16_round(rng.uniform(-1, 1, (c.B, c.N, c.Tout)).astype(np.float32)).astype(np.float32)).astype(np.float64)
    return {"x": x, "w": w, "bias": None if c.mode == T2 else bias, "mask": mask, "prior": prior}


# ---------------------------------------------------------------------------------------------------------------------------
# the conv
# ---------------------------------------------------------------------------------------------------------------------------
def _gather(x, idx, Tin, pad_value):
    """x[..., idx] with zeros (pad_value for the elements next to the row: index -1 and Tin) outside [0, Tin)."""
    ok = (idx >= 0) & (idx < Tin)
    g = np.where(ok, x[..., np.clip(idx, 0, Tin - 1)], 0.0)
    if pad_value is not None:
        g = np.where((idx == -1) | (idx == Tin), pad_value, g)
    return g


def conv_ref(c, x, w, bias, mutant=None, x_off=0):
    """-> value [B, N, Tout] (bias included), sum|terms| (with |bias|), largest |term|, terms (int).  x_off: only the
    `odd_pair_partner` mutant reads it."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    B, C, Tin = x.shape
    assert (B, C, Tin) == (c.B, c.C0 + c.C1, c.Tin)
    if mutant == "drop_last_group":
        x = x.copy()
        x[:, (C - 1) // 8 * 8:] = 0.0
    if mutant == "swap_stage_groups":                 # the first 8-channel group of stage 0 <-> of stage 1 (32-channel stages)
        x = x.copy()
        x[:, 0:8], x[:, 32:40] = x[:, 32:40].copy(), x[:, 0:8].copy()
    if mutant == "odd_pair_partner" and x_off % 2:
        x = x.copy()                                  # the row's first sample is the HIGH half of its dword pair: the low half
        x[:, :, 0] = PAD_VALUE                        # is the pad element in front of the row
    pad_value = PAD_VALUE if mutant == "admit_pad" else None
    val = np.zeros((B, c.N, c.Tout))
    mag = np.zeros((B, c.N, c.Tout))
    big = np.zeros((B, c.N, c.Tout))
    aw = np.abs(w)
    q = np.arange(c.Tout)
    if c.mode == T2:
        # dx[b, n, t] = sum_{k, m} w[k, n, m] dz[b, m, (t - k) / 2]  where t - k is even and inside the row
        for k in range(c.k):
            if mutant == "drop_tap" and k == c.k // 2:
                continue
            t = q ^ 1 if mutant == "swap_phases" else q
            num = t - k + (2 if mutant == "shift_taps" else 0)
            g = np.where(num % 2 == 0, _gather(x, num // 2, Tin, pad_value), 0.0)          # [B, C, Tout]
            val += np.einsum("bmt,nm->bnt", g, w[k])
            mag += np.einsum("bmt,nm->bnt", np.abs(g), aw[k])
            big = np.maximum(big, (np.abs(g)[:, None] * aw[k][None, :, :, None]).max(axis=2))
        terms = taps_of(c) * C
    else:
        s = 2 if c.mode == S2 else 1
        for k in range(c.k):
            if mutant == "drop_tap" and k == c.k // 2:
                continue
            idx = q * s + k - c.shift + (1 if mutant == "shift_taps" else 0)
            if mutant == "swap_planes":
                idx = idx ^ 1
            g = _gather(x, idx, Tin, pad_value)
            val += np.einsum("bct,cn->bnt", g, w[k])
            mag += np.einsum("bct,cn->bnt", np.abs(g), aw[k])
            big = np.maximum(big, (np.abs(g)[:, :, None] * aw[k][None, :, :, None]).max(axis=1))
        terms = c.k * C
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)[None, :, None]
        val, mag, big, terms = val + b, mag + np.abs(b), np.maximum(big, np.abs(b)), terms + 1
    if mutant == "zero_last_col_tile":
        val[:, (c.N - 1) // 16 * 16:] = 0.0
    return val, mag, big, terms


def epilogue_ref(c, val, lrelu=False, mask=None, prior=None, acc=None, y_off=0, mutant=None):
    """val [B, N, Tout] -> the value stored, BEFORE any rounding to bf16.  acc: None, or (acc_lo, acc_len) in row positions
    y_off + q, acc_len 0 = the whole row; prior = what the destination held."""
    v = np.array(val, dtype=np.float64)
    if lrelu:
        v = np.maximum(SLOPE * v, v)
    if mask is not None:
        hi, lo = (SLOPE, 1.0) if mutant == "mask_slope" else (1.0, SLOPE)
        v = v * np.where(mask > 0, hi, lo)
    if acc is not None:
        lo, ln = acc
        pos = y_off + np.arange(c.Tout)
        inside = np.ones(c.Tout, dtype=bool) if (ln == 0 or mutant == "acc_outside") else (pos >= lo) & (pos < lo + ln)
        v = v + np.where(inside[None, None, :], prior, 0.0)
    return v


def dec_ref(stored, N0, mutant=None):
    """The compact copy: dec[b, n, q >> 1] = stored[b, n, q] at even q, of the first N0 columns."""
    return stored[:, :N0, (1 if mutant == "dec_odd" else 0)::2]


def stored_bf16(v, mutant=None):
    return E.bf16_round(v, "truncate" if mutant == "truncate" else "nearest")


# ---------------------------------------------------------------------------------------------------------------------------
# verdicts (> 1 fails)
# ---------------------------------------------------------------------------------------------------------------------------
def fp32_bound(c_factor, terms, mag, ref):
    """|err| <= c (terms + 2) 2^-24 sum|terms| + 2^-24 |ref|: E.fp32_bound with the measured factor c on its first part."""
    return c_factor * (terms + 2) * E.EPS32 * np.asarray(mag) + E.EPS32 * np.abs(ref)


def extra_roundings(lrelu, mask, acc, ref, prior_mag):
    """fp32 roundings the epilogue adds behind the conv's own: the 0.2f products and the accumulate add, one 2^-24 each of the
    magnitudes they act on."""
    n = int(bool(lrelu)) + int(mask is not None) + int(acc is not None)
    return n * E.EPS32 * (np.abs(ref) + prior_mag)


def fp32_verdict(got, ref, bound):
    return E.worst_ratio(got, ref, bound)


def bf16_verdict(got, ref, big, fp32_part, pool=None):
    """bf16 rows against float64 (tests/test_gpu_elementwise.py's rule): one bf16 spacing + the fp32 bound per element; pool
    collects [elements that differ from the once-rounded reference, elements]."""
    r = E.bf16_round(ref)
    if pool is not None and np.isfinite(got).all():
        d, t = E.differ_count(got, r)
        pool[0] += d
        pool[1] += t
    return E.worst_ratio(got, r, E.bf16_bound(r, big, fp32_part))


def case_reference(c, inp, lrelu=False, mask=False, acc=None, y_off=0, x_off=0, mutant=None, c_factor=1.0):
    """-> the float64 value stored (before a bf16 rounding), its fp32 bound, the largest |term| (for the bf16 spacing)."""
    val, mag, big, terms = conv_ref(c, inp["x"], inp["w"], inp["bias"], mutant, x_off)
    ref = epilogue_ref(c, val, lrelu, inp["mask"] if mask else None, inp["prior"], acc, y_off, mutant)
    pm = np.abs(inp["prior"]) if acc is not None else 0.0
    bound = fp32_bound(c_factor, terms, mag, ref) + extra_roundings(lrelu, True if mask else None, acc, ref, pm)
    return ref, bound, np.maximum(big, pm)


def standin_fp32(c, inp, lrelu=False, mask=False, acc=None, y_off=0, bias_first=False):
    """The same operator in float32 numpy, taps in DESCENDING order and channels summed by a float32 einsum: another valid fp32
    execution, for the condition on the share of bf16 elements that may differ from the once-rounded float64 reference.
    bias_first: the accumulator starts at the bias (the audio-input conv), so that every later add rounds."""
    x, w = inp["x"].astype(np.float32), inp["w"].astype(np.float32)
    val = np.zeros((c.B, c.N, c.Tout), dtype=np.float32)
    if bias_first:
        val = val + inp["bias"].astype(np.float32)[None, :, None]
    q = np.arange(c.Tout)
    for k in reversed(range(c.k)):
        if c.mode == T2:
            num = q - k
            g = np.where(num % 2 == 0, _gather(x, num // 2, c.Tin, None), np.float32(0)).astype(np.float32)
            val += np.einsum("bmt,nm->bnt", g, w[k]).astype(np.float32)
        else:
            g = _gather(x, q * (2 if c.mode == S2 else 1) + k - c.shift, c.Tin, None).astype(np.float32)
            val += np.einsum("bct,cn->bnt", g, w[k]).astype(np.float32)
    if inp["bias"] is not None and not bias_first:
        val = val + inp["bias"].astype(np.float32)[None, :, None]
    s = np.float32(0.2)
    if lrelu:
        val = np.maximum(s * val, val)
    if mask:
        val = val * np.where(inp["mask"] > 0, np.float32(1), s)
    if acc is not None:
        pos = y_off + q
        inside = np.ones(c.Tout, dtype=bool) if acc[1] == 0 else (pos >= acc[0]) & (pos < acc[0] + acc[1])
        val = val + np.where(inside[None, None, :], inp["prior"], 0.0).astype(np.float32)
    assert val.dtype == np.float32
    return val


def _pad8(t):
    return (t + 7) // 8 * 8


def desc_fields(c, x_off=0, y_off=0, lrelu=0, acc=None, dec=0, out_bf16=0):
    """The fields of wun_op_conv_bf16_desc for a case; pitches: the row and its offset padded to 8 elements, plus 8."""
    xp = _pad8(x_off + c.Tin) + 8
    yp = _pad8(y_off + c.Tout) + 8
    return dict(mode=c.mode, B=c.B, C0=c.C0, C1=c.C1, N=c.N, N0=c.N0, K=c.k, Tin=c.Tin, Tout=c.Tout, shift=c.shift,
                lrelu=int(lrelu), out_bf16=int(out_bf16), accumulate=int(acc is not None), acc_lo=acc[0] if acc else 0,
                acc_len=acc[1] if acc else 0, x0_pitch=xp, x1_pitch=xp if c.C1 else 0, x_off=x_off, y0_pitch=yp, y0_off=y_off,
                y1_pitch=yp if c.N0 < c.N else 0, y1_off=y_off if c.N0 < c.N else 0,
                dec_pitch=_pad8((c.Tout + 1) // 2) + 8 if dec else 0)


# mutant -> does it apply to (case, options)?  options: dict with x_off, mask, acc, dec, bf16
MUTANTS = {
    "drop_tap": lambda c, o: True,
    "shift_taps": lambda c, o: True,
    "drop_last_group": lambda c, o: True,
    "swap_stage_groups": lambda c, o: c.C0 + c.C1 >= 40,
    "odd_pair_partner": lambda c, o: o.get("x_off", 0) % 2 == 1,
    "admit_pad": lambda c, o: True,                    # every case zero-fills (the case builders above)
    "zero_last_col_tile": lambda c, o: True,
    "swap_planes": lambda c, o: c.mode == S2,
    "swap_phases": lambda c, o: c.mode == T2,
    "dec_odd": lambda c, o: bool(o.get("dec")),
    "acc_outside": lambda c, o: o.get("acc") is not None and o["acc"][1] != 0,
    "mask_slope": lambda c, o: bool(o.get("mask")),
    "truncate": lambda c, o: bool(o.get("bf16")),
}


# ---------------------------------------------------------------------------------------------------------------------------
# first_conv_kernel: the audio-input conv (fp32 audio in, direct conv on the vector pipe)
# ---------------------------------------------------------------------------------------------------------------------------
FirstCase = collections.namedtuple("FirstCase", "stride cin N k Tout same")
FIRST_B = 2


def first_cases():
    """Every (stride, channels) x {K = 15, K = 9: the run-time instantiation} x N in {24, 56: two weight passes, the second
    partial} x Tout in {5: a lone partial quad, 1027: two workgroups per row and a 3-element tail} x {same padding: both edges
    clamp, valid}; bf16 / fp32 output is the test's own loop."""
    out = []
    for stride in (1, 2):
        for cin in (1, 2):
            for k in (15, 9):
                for N in (24, 56):
                    for Tout in (5, 1027):
                        for same in (1, 0):
                            out.append(FirstCase(stride, cin, N, k, Tout, same))
    return out


def first_geometry(fc):
    """-> Tin, shift"""
    if fc.same:
        return fc.stride * fc.Tout, 7
    return (fc.Tout - 1) * fc.stride + fc.k, 0


def first_inputs(fc, grid=False):
    Tin, _ = first_geometry(fc)
    rng = np.random.default_rng(_seed(*fc, int(grid), 77))
    if grid:
        x = rng.integers(-255, 256, (FIRST_B, fc.cin, Tin)) / 256.0
        w = rng.integers(-255, 256, (fc.k, fc.cin, fc.N)) / 1024.0
        bias = rng.uniform(-0.1, 0.1, fc.N).astype(np.float32).astype(np.float64)
    else:
        x = rng.uniform(-1, 1, (FIRST_B, fc.cin, Tin)).astype(np.float32).astype(np.float64)
        w = (rng.uniform(-1, 1, (fc.k, fc.cin, fc.N)) / np.sqrt(fc.k * fc.cin)).astype(np.float32).astype(np.float64)
        bias = rng.uniform(-0.1, 0.1, fc.N).astype(np.float32).astype(np.float64)
    return x, w, bias


def first_as_case(fc):
    Tin, shift = first_geometry(fc)
    return Case(S2 if fc.stride == 2 else S1, FIRST_B, fc.cin, 0, fc.N, fc.N, fc.k, Tin, fc.Tout, shift)
