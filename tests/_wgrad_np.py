"""Float64 reference of a layer's weight / bias gradient as the plan launches it (wun_op_wgrad_ex, include/wun.h), the launch
shapes tests/test_gpu_wgrad_ops.py runs, and the inputs both it and tests/test_wgrad_ops_host.py build for them.

A SHAPE is a dict of the descriptor's values: B, C0, C1, N, K, x0_pitch, x1_pitch and `parts`, a list of one or two dicts
{loader (0 direct, stride 1 / 1 de-interleaving, stride 2), x0_off, x1_off, Tin, shift, Tq, dz_pitch}; the narrow family's
shapes also carry planes (N = planes * Nper).  Per part the reference takes row[off : off + Tin] of each source, concatenates
the channels, puts `shift` zeros in front and zeros behind as needed, and correlates with the part's dz at the part's stride;
the parts add:
    dW[k][c][n] = sum_p sum_{b, q < Tq} win_p[b][c][S q + k - shift] dz_p[b][n][q],     db[n] = sum_p sum_{b, q} dz_p[b][n][q].
Rows are whole rows ([B][C][pitch]): what lies outside the windows is in the arrays and must not matter."""
import numpy as np
import torch

FILL = 1.0e4                    # magnitude of everything in a row that no window covers (finite: it may be loaded)
LDS, WIN, BF16, NARROW = range(4)        # wun_op_wgrad_desc.family
FAMILY_NAMES = {LDS: "lds", WIN: "win", BF16: "bf16", NARROW: "narrow"}


def pad4(t):
    return (t + 3) // 4 * 4


def bf16_round(a):
    """Round to nearest even bf16, returned as float32 (what a bf16 row holds)."""
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).to(torch.bfloat16).to(torch.float32).numpy()


def stride_of(part):
    return 2 if part["loader"] else 1


def part_window(x0, x1, part):
    """[B][C0 + C1][Tin] float64: the part's window of every row, channels of the two sources concatenated."""
    w = x0[:, :, part["x0_off"]:part["x0_off"] + part["Tin"]]
    assert w.shape[2] == part["Tin"]
    if x1 is not None:
        w1 = x1[:, :, part["x1_off"]:part["x1_off"] + part["Tin"]]
        assert w1.shape[2] == part["Tin"]
        w = np.concatenate([w, w1], axis=1)
    return np.asarray(w, dtype=np.float64)


def reference(x0, x1, dzs, K, parts):
    """x0 [B][C0][x0_pitch], x1 [B][C1][x1_pitch] or None, dzs[p] [B][N][dz_pitch] -> (dW [K][C0 + C1][N], db [N]) in float64."""
    dw = db = None
    for part, dz in zip(parts, dzs):
        win = part_window(x0, x1, part)
        B, C, Tin = win.shape
        S, Tq, shift = stride_of(part), part["Tq"], part["shift"]
        span = (Tq - 1) * S + K
        padded = np.zeros((B, C, max(span, shift + Tin)))
        padded[:, :, shift:shift + Tin] = win
        z = np.asarray(dz[:, :, :Tq], dtype=np.float64)
        g = np.stack([np.einsum("bcq,bnq->cn", padded[:, :, k:k + (Tq - 1) * S + 1:S], z) for k in range(K)])
        dw = g if dw is None else dw + g
        db = z.sum(axis=(0, 2)) if db is None else db + z.sum(axis=(0, 2))
    return dw, db


def reference_loops(x0, x1, dzs, K, parts):
    """The same sums, one product at a time (the smallest shapes only)."""
    C = x0.shape[1] + (0 if x1 is None else x1.shape[1])
    N = dzs[0].shape[1]
    dw, db = np.zeros((K, C, N)), np.zeros(N)
    for part, dz in zip(parts, dzs):
        S = stride_of(part)
        for b in range(x0.shape[0]):
            for q in range(part["Tq"]):
                db += np.asarray(dz[b, :, q], dtype=np.float64)
                for k in range(K):
                    t = S * q + k - part["shift"]
                    if 0 <= t < part["Tin"]:
                        col = [float(x0[b, c, part["x0_off"] + t]) for c in range(x0.shape[1])]
                        if x1 is not None:
                            col += [float(x1[b, c, part["x1_off"] + t]) for c in range(x1.shape[1])]
                        dw[k] += np.outer(np.array(col), np.asarray(dz[b, :, q], dtype=np.float64))
    return dw, db


def reference_autograd(x0, x1, dzs, K, parts):
    """torch.autograd of an explicit F.conv1d over the materialised crop + concat + padding of every part."""
    import torch.nn.functional as F
    C = x0.shape[1] + (0 if x1 is None else x1.shape[1])
    N = dzs[0].shape[1]
    w = torch.zeros((K, C, N), dtype=torch.float64, requires_grad=True)
    bias = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    total = 0.0
    for part, dz in zip(parts, dzs):
        S, Tq = stride_of(part), part["Tq"]
        xin = torch.tensor(part_window(x0, x1, part))
        need = (Tq - 1) * S + K - part["shift"]
        xin = F.pad(xin, (part["shift"], max(0, need - part["Tin"])))
        y = F.conv1d(xin, w.permute(2, 1, 0), bias, stride=S)[:, :, :Tq]
        total = total + (y * torch.tensor(np.asarray(dz[:, :, :Tq], dtype=np.float64))).sum()
    total.backward()
    return w.grad.numpy(), bias.grad.numpy()


# ---------------------------------------------------------------------------------------------------------------------------
# shapes
# ---------------------------------------------------------------------------------------------------------------------------
def make_shape(B, C0, C1, N, K, parts, planes=1):
    parts = [dict(p) for p in parts]
    for p in parts:
        p.setdefault("x1_off", 0)
        p.setdefault("shift", 0)
        p["dz_pitch"] = pad4(p["Tq"]) + 4
    return {"B": B, "C0": C0, "C1": C1, "N": N, "K": K, "planes": planes, "parts": parts,
            # pitches larger than any window, and different for the two sources
            "x0_pitch": pad4(max(p["x0_off"] + p["Tin"] for p in parts)) + 8,
            "x1_pitch": pad4(max(p["x1_off"] + p["Tin"] for p in parts)) + 12 if C1 else 0}


def up_shape(B, C0, C1, N, K, Tin, x0_off, x1_off, shift=0):
    """An up conv over concat(crop(skip), upsampled): one direct part; valid (shift 0) or 'same' (Tq = Tin)."""
    Tq = Tin if shift else Tin - K + 1
    return make_shape(B, C0, C1, N, K, [dict(loader=0, x0_off=x0_off, x1_off=x1_off, Tin=Tin, shift=shift, Tq=Tq)])


def deep_shape(B, C0, C1, N, K, Tin, Tq, x0_off=0, x1_off=0):
    return make_shape(B, C0, C1, N, K, [dict(loader=0, x0_off=x0_off, x1_off=x1_off, Tin=Tin, Tq=Tq)])


T_DOWN = 257            # row length of the down level's input


def down_shape(form, cs=9):
    """(B, Cin, N, K) = (2, 24, 48, 15) on rows of 257: part 0 = the decimated positions; part 1 = the skip-window positions
    (`direct`: full rate at off = cs) or the odd positions (`dedup`: de-interleaving loader at off = 11); `alone`: part 0 only."""
    parts = [dict(loader=1, x0_off=0, Tin=T_DOWN, Tq=122)]
    if form == "direct":
        parts.append(dict(loader=0, x0_off=cs, Tin=114, Tq=100))
    elif form == "dedup":
        parts.append(dict(loader=1, x0_off=11, Tin=T_DOWN - 11, Tq=116))
    else:
        assert form == "alone"
    return make_shape(2, 24, 0, 48, 15, parts)


def reduce_shape(B):
    """Few tiles, many units: (Cin, N, K) = (24, 16, 5), Tq = 130 = two units of 128 positions per excerpt."""
    return make_shape(B, 24, 0, 16, 5, [dict(loader=0, x0_off=0, Tin=134, Tq=130)])


def head_shape(K, planes, x1_off=0):
    """The output head: 2 audio channels cropped at 37 + 24 feature channels, `planes` sources of Nper = 2 rows."""
    Tq = 1000
    return make_shape(2, 2, 24, 2 * planes, K, [dict(loader=0, x0_off=37, x1_off=x1_off, Tin=Tq + K - 1, Tq=Tq)], planes=planes)


def audio_shape(C, two_parts=True):
    """The audio-input conv: K = 15, N = 24 over rows of 5000: the stride-2 positions, then stride-1 positions at an odd offset."""
    parts = [dict(loader=1, x0_off=0, Tin=5000, Tq=2493)]
    if two_parts:
        parts.append(dict(loader=0, x0_off=1001, Tin=314, Tq=300))
    return make_shape(1, C, 0, 24, 15, parts)


UP_MAIN = (2, 24, 24, 40, 5, 301)
UP_OFFSETS = [(a, b) for a in (0, 1, 2, 3, 5) for b in (0, 2)]
UP_OTHER = [((3, 40, 8, 48, 15, 120), (0, 0)), ((3, 40, 8, 48, 15, 120), (3, 2)),
            ((2, 18, 14, 24, 5, 77), (0, 0)), ((2, 18, 14, 24, 5, 77), (1, 2)),
            ((2, 7, 9, 24, 5, 77), (0, 0)), ((2, 7, 9, 24, 5, 77), (2, 1))]
DEEP = [(16, 48, 48, 48, 5, 13, 9), (16, 24, 0, 48, 15, 23, 9)]
DEEP_OFFSETS = [(0, 0), (3, 1)]


def all_shapes():
    """(id, shape) of every launch shape the GPU tests use (the host test checks the reference on each)."""
    out = []
    for a, b in UP_OFFSETS:
        out.append(("up%s off%d,%d" % (UP_MAIN, a, b), up_shape(*UP_MAIN, a, b)))
    out.append(("up%s same" % (UP_MAIN,), up_shape(*UP_MAIN, 0, 0, shift=2)))
    for dims, (a, b) in UP_OTHER:
        out.append(("up%s off%d,%d" % (dims, a, b), up_shape(*dims, a, b)))
    for dims in DEEP:
        for a, b in DEEP_OFFSETS:
            out.append(("deep%s off%d,%d" % (dims, a, b), deep_shape(*dims, a, b if dims[2] else 0)))
    for cs in (9, 10):
        out.append(("down direct cs%d" % cs, down_shape("direct", cs)))
    out.append(("down dedup", down_shape("dedup")))
    out.append(("down alone", down_shape("alone")))
    for B in (16, 32):
        out.append(("reduce B%d" % B, reduce_shape(B)))
    for K, x1_off in ((1, 0), (3, 3)):
        for planes in (2, 4):
            out.append(("head K%d planes%d" % (K, planes), head_shape(K, planes, x1_off)))
    for C in (1, 2):
        out.append(("audio C%d two parts" % C, audio_shape(C)))
        out.append(("audio C%d part 0" % C, audio_shape(C, False)))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def _fill(rng, shape):
    """Finite values around +-1e4: one of them in a sum misses any tolerance by orders of magnitude."""
    return (FILL * rng.uniform(0.5, 1.5, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def make_rows(rng, B, C, pitch, windows):
    """[B][C][pitch] float32: uniform(-1, 1) inside the union of `windows` [(off, Tin)], the fill everywhere else."""
    rows = _fill(rng, (B, C, pitch))
    for off, Tin in windows:
        assert 0 <= off and off + Tin <= pitch
    lo, hi = min(o for o, _ in windows), max(o + t for o, t in windows)
    covered = np.zeros(pitch, dtype=bool)
    for off, Tin in windows:
        covered[off:off + Tin] = True
    vals = rng.uniform(-1, 1, (B, C, hi - lo)).astype(np.float32)
    rows[:, :, lo:hi] = np.where(covered[lo:hi], vals, rows[:, :, lo:hi])
    return rows


def make_inputs(shape, seed, bf16_x0=False, bf16_x1=False, bf16_dz=False):
    """-> (x0, x1 or None, [dz per part]) float32 arrays; with a bf16 flag the array holds bf16 values (rounded here)."""
    rng = np.random.default_rng(seed)
    parts = shape["parts"]
    x0 = make_rows(rng, shape["B"], shape["C0"], shape["x0_pitch"], [(p["x0_off"], p["Tin"]) for p in parts])
    x1 = None
    if shape["C1"]:
        x1 = make_rows(rng, shape["B"], shape["C1"], shape["x1_pitch"], [(p["x1_off"], p["Tin"]) for p in parts])
    dzs = [make_rows(rng, shape["B"], shape["N"], p["dz_pitch"], [(0, p["Tq"])]) for p in parts]
    if bf16_x0:
        x0 = bf16_round(x0)
    if bf16_x1 and x1 is not None:
        x1 = bf16_round(x1)
    if bf16_dz:
        dzs = [bf16_round(z) for z in dzs]
    return x0, x1, dzs


def refill_outside(shape, x0, x1, dzs, seed):
    """Copies of the inputs with everything OUTSIDE the windows replaced by other values (the windows keep theirs)."""
    rng = np.random.default_rng(seed)
    parts = shape["parts"]

    def redo(rows, windows):
        new = (-0.37 * _fill(rng, rows.shape)).astype(np.float32)
        for off, Tin in windows:
            new[:, :, off:off + Tin] = rows[:, :, off:off + Tin]
        return new

    y0 = redo(x0, [(p["x0_off"], p["Tin"]) for p in parts])
    y1 = None if x1 is None else redo(x1, [(p["x1_off"], p["Tin"]) for p in parts])
    return y0, y1, [redo(z, [(0, p["Tq"])]) for z, p in zip(dzs, parts)]
