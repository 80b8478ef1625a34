"""Float64 numpy oracle of the recursive filter and the BS.1770-4 loudness meter, written from the
definition and independently of the device code:
  sosfilt_serial     the serial direct-form-I recurrence per section (the definition of include/wun.h: wun_sosfilt)
  sosfilt_chunked    a numpy emulation of the device's parallel SCHEDULE (chunks, zero-state pass, carry with the chunk's
                     transition matrix, second pass), with carries optionally dropped (the sensitivity check)
  kweight_sos        the K-weighting design;  loudness: the gated meter
For long inputs sosfilt_fast runs scipy.signal.lfilter per section (compared with the serial loop on a short input by
tests/test_loudness_host.py)."""
import numpy as np


def kweight_sos(sr):
    sr = float(sr)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    hp = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, hp], np.float64)


# the standard's table at 48 kHz (ITU-R BS.1770-4, tables 1 and 2), 14 printed decimals
TABLE_48K = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                      [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])


def _section_serial(c, x, x1=0.0, x2=0.0, y1=0.0, y2=0.0):
    """One section over a 1-D float64 signal from the given history; returns y."""
    b0, b1, b2, _, a1, a2 = (float(v) for v in c)
    y = np.empty_like(x)
    for t in range(x.shape[0]):
        xv = x[t]
        yv = b0 * xv + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
        x2, x1 = x1, xv
        y2, y1 = y1, yv
        y[t] = yv
    return y


def sosfilt_serial(sos, x):
    """x [n, C] (any float type) -> float64 [n, C]: the cascade, serial in time, zero initial state (the channels side by side)."""
    sos = np.asarray(sos, np.float64)
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    return _cascade(sos, x, np.zeros(C), np.zeros(C), np.zeros((2 * sos.shape[0], C)))[0]


def sosfilt_fast(sos, x):
    from scipy.signal import lfilter
    sos = np.asarray(sos, np.float64)
    y = np.asarray(x, np.float64)
    for s in range(sos.shape[0]):
        y = lfilter(sos[s, :3], sos[s, 3:], y, axis=0)
    return y


def step_matrix(sos):
    """T: one zero-input step of the cascade on the state (y_s[t-1], y_s[t-2])_s."""
    sos = np.asarray(sos, np.float64)
    nsec = sos.shape[0]
    D = 2 * nsec
    T = np.zeros((D, D))
    for q in range(D):
        st = np.zeros(D)
        st[q] = 1.0
        in0 = in1 = in2 = 0.0
        for s in range(nsec):
            b0, b1, b2, _, a1, a2 = sos[s]
            p1, p2 = st[2 * s], st[2 * s + 1]
            y = b0 * in0 + b1 * in1 + b2 * in2 - a1 * p1 - a2 * p2
            T[2 * s, q], T[2 * s + 1, q] = y, p1
            in0, in1, in2 = y, p1, p2
    return T


def _cascade(sos, x, x1, x2, state):
    """The cascade over x [T, ...] (time first; the other axes run side by side) from the input history x1, x2 [...] and the
    state [2 nsec, ...]; returns (y, end state).  The same arithmetic as _section_serial, section by section."""
    nsec = sos.shape[0]
    v, h1, h2 = x, x1, x2
    end = np.zeros_like(state)
    for s in range(nsec):
        b0, b1, b2, _, a1, a2 = (float(c) for c in sos[s])
        y1, y2 = state[2 * s].copy(), state[2 * s + 1].copy()
        n1, n2 = y1.copy(), y2.copy()                    # the next section's input history is this one's state
        p1, p2 = h1.copy(), h2.copy()
        out = np.empty_like(v)
        for t in range(v.shape[0]):
            xv = v[t]
            yv = b0 * xv + b1 * p1 + b2 * p2 - a1 * y1 - a2 * y2
            p2, p1 = p1, xv
            y2, y1 = y1, yv
            out[t] = yv
        end[2 * s], end[2 * s + 1] = y1, y2
        v, h1, h2 = out, n1, n2
    return v, end


def sosfilt_chunked(sos, x, chunk, drop_carry=False):
    """The device's schedule in numpy: pass 1 (zero recursive state, true input history) -> end states; carry
    v[k+1] = M v[k] + e[k], M = T^chunk; pass 2 from the true states.  drop_carry: v[k] = 0 for every chunk.  All chunks of
    all channels run side by side; the input is zero-extended to whole chunks and the surplus outputs are dropped (the last
    chunk's end state has no reader)."""
    sos = np.asarray(sos, np.float64)
    x = np.asarray(x, np.float64)
    n, C = x.shape
    chunk = int(chunk)
    D = 2 * sos.shape[0]
    M = np.linalg.matrix_power(step_matrix(sos), chunk)
    nch = -(-n // chunk)
    xp = np.zeros((nch * chunk, C))
    xp[:n] = x
    xt = xp.reshape(nch, chunk, C).transpose(1, 0, 2)                      # [chunk, nch, C]
    prev = np.concatenate([np.zeros((2, C)), xp])                           # prev[t] = x[t - 2]
    x1 = prev[1:1 + nch * chunk:chunk]                                      # x[k chunk - 1], [nch, C]
    x2 = prev[0:nch * chunk:chunk]
    zero = np.zeros((D, nch, C))
    ends = _cascade(sos, xt, x1, x2, zero)[1]
    starts = np.zeros((D, nch, C))
    if not drop_carry:
        v = np.zeros((D, C))
        for k in range(nch):
            starts[:, k] = v
            v = M @ v + ends[:, k]
    y = _cascade(sos, xt, x1, x2, starts)[0]
    return y.transpose(1, 0, 2).reshape(nch * chunk, C)[:n]


def block_geometry(n, sr):
    Nb, step = (4 * int(sr) + 5) // 10, (int(sr) + 5) // 10          # round(0.4 sr), round(0.1 sr), halves up
    nb = (n - Nb) // step + 1 if n >= Nb else 0
    return Nb, step, nb


def loudness(x, sr, filt=sosfilt_fast):
    """(L, kept, nb, peak, l) of x [n, C]: integrated loudness (-inf when no block passes), blocks kept, complete blocks,
    sample peak, momentary values l [nb]."""
    x = np.asarray(x)
    n = x.shape[0]
    y = filt(kweight_sos(sr), x)
    Nb, step, nb = block_geometry(n, sr)
    z = np.array([np.sum(np.mean(y[j * step:j * step + Nb] ** 2, axis=0)) for j in range(nb)], np.float64).reshape(nb)
    with np.errstate(divide="ignore"):
        l = -0.691 + 10.0 * np.log10(z)
        peak = float(np.max(np.abs(x.astype(np.float64)))) if n else 0.0
        absg = l > -70.0
        if not absg.any():
            return -np.inf, 0, nb, peak, l
        gate = -0.691 + 10.0 * np.log10(np.mean(z[absg])) - 10.0
        keep = absg & (l > gate)
        if not keep.any():
            return -np.inf, 0, nb, peak, l
        return float(-0.691 + 10.0 * np.log10(np.mean(z[keep]))), int(keep.sum()), nb, peak, l


def gain(L, peak, target=-23.0, max_gain_db=30.0, peak_limit=None):
    """(g, 1 / g) as float32, by the rule of wun_loudness_gain."""
    g = 1.0
    if np.isfinite(L):
        g = min(10.0 ** ((target - L) / 20.0), 10.0 ** (max_gain_db / 20.0))
        if peak_limit is not None and peak > 0 and g * peak > peak_limit:
            g = peak_limit / peak
    g32 = np.float32(g)
    return g32, np.float32(1.0 / np.float64(g32))


# ---- the filter cases of the tests (tests/test_loudness_host.py, tests/test_gpu_loudness.py) ----
def resonator(radius, w0):
    """One peaking section: poles at radius * exp(+-i w0), zeros at +-1, unit gain at the peak."""
    g = (1.0 - radius * radius) / 2.0
    return np.array([[g, 0.0, -g, 1.0, -2.0 * radius * np.cos(w0), radius * radius]])


def filter_cases():
    k48, k8 = kweight_sos(48000), kweight_sos(8000)
    return {"kweight48k": k48, "kweight8k": k8, "peak0999": resonator(0.999, 2 * np.pi * 0.05),
            "cascade3": np.concatenate([k48[:1], resonator(0.99, 2 * np.pi * 0.11), k8[1:]])}


INPUT_KINDS = ("noise", "impulses", "step")


def filter_input(kind, n, C, chunk):
    if kind == "noise":
        return np.random.RandomState(n * 7 + C).randn(n, C).astype(np.float32)
    x = np.zeros((n, C), np.float32)
    if kind == "impulses":                               # at 0 and at chunk - 1: the input history crosses a chunk
        x[0] = 1.0
        if n > chunk - 1:
            x[chunk - 1, :] = -0.75
    else:                                                # a DC step: the high-pass tail crosses many chunks
        x[:] = 0.5
    return x


def filter_tolerance(serial, emulated):
    """What a device result rounded to float32 may differ from float32(serial) by: one float32 rounding at max |y| (two float64
    values a hair apart can round to neighbouring floats: one ulp, 2^-23 max |y|) plus 4 times the error the chunked schedule
    itself shows against the serial recurrence on this input (the 4 covers the device's FMA arithmetic of the same schedule)."""
    return 2.0 ** -23 * np.max(np.abs(serial)) + 4.0 * np.max(np.abs(emulated - serial))
