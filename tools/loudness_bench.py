"""Times the loudness meter (wun_loudness) and the K-weighting as a filter (wun_sosfilt) on a synthetic 3-minute, 44.1 kHz, stereo
track.  HIP events around each entry after a warm-up, minimum and median of `--rounds` rounds; beside each
time the bytes the entry must move (the meter reads every float twice and writes 4 + 4 + 4 doubles per chunk and channel; the
filter reads twice and writes once) and the rate that makes; also the gain + scale launches, and scipy.signal.sosfilt plus the
numpy gating (tests/_loudness_np.py) on the same track on the host.  The R 128 entries on the same track:
wun_true_peak at the rate's oversampling factor with its share of the roof of reading x once, and wun_loudness_r128 timed in
alternation with wun_loudness (the meter it extends) and with wun_loudness + wun_true_peak called separately; --hour-8k adds
r128 on an hour of 8 kHz mono (36 000 short-term values: what the quadratic rank selection costs).  Prints one JSON line;
--out writes it to a file.

  python tools/loudness_bench.py --rounds 5 --out profiles/loudness_bench.json [--seconds 180]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wave_u_net_amd import loudness  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy / numpy timing")
    ap.add_argument("--hour-8k", action="store_true", help="also time r128 on an hour of 8 kHz mono")
    ap.add_argument("--hbm-gb-per-s", type=float, default=6290.0, help="the measured copy rate the roof is taken from")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: timings on a CPU say nothing"
    dev = torch.device("cuda:0")
    n, C, sr = int(a.seconds * a.sr), a.channels, a.sr
    x = (0.1 * torch.randn((n, C), generator=torch.Generator(device="cpu").manual_seed(0))).to(dev)
    sos = loudness.kweight_sos(sr)
    lib = loudness._lib.load()
    s_f = torch.empty(int(lib.wun_sosfilt_scratch_doubles(n, C, 2)), dtype=torch.float64, device=dev)
    s_m = torch.empty(loudness.scratch_doubles(n, C, sr), dtype=torch.float64, device=dev)
    y = torch.empty_like(x)
    z = x.clone()
    s_p = torch.empty(int(lib.wun_true_peak_scratch_doubles(n, C)), dtype=torch.float64, device=dev)
    s_r = torch.empty(loudness.r128_scratch_doubles(n, C, sr), dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        return out, e0.elapsed_time(e1)

    meter = loudness.integrated(x, sr, scratch=s_m)                                   # warm-up of every entry
    loudness.sosfilt(x, sos, out=y, scratch=s_f)
    g = loudness.gain(meter)
    loudness.scale_(z, g[0:1])
    loudness.true_peak(x, sr, scratch=s_p)
    report = loudness.r128(x, sr, scratch=s_r)
    torch.cuda.synchronize()
    t = {"meter_ms": [], "sosfilt_ms": [], "gain_ms": [], "scale_ms": [], "true_peak_ms": [], "r128_ms": [], "meter_alt_ms": [],
         "meter_plus_true_peak_ms": []}
    for _ in range(a.rounds):
        meter, ms = timed(lambda: loudness.integrated(x, sr, scratch=s_m)); t["meter_ms"].append(ms)
        _, ms = timed(lambda: loudness.sosfilt(x, sos, out=y, scratch=s_f)); t["sosfilt_ms"].append(ms)
        g, ms = timed(lambda: loudness.gain(meter)); t["gain_ms"].append(ms)
        _, ms = timed(lambda: loudness.scale_(z, g[1:2])); t["scale_ms"].append(ms)
        _, ms = timed(lambda: loudness.true_peak(x, sr, scratch=s_p)); t["true_peak_ms"].append(ms)
        for _ in range(3):                                                            # alternating: r128, the meter, the two apart
            report, ms = timed(lambda: loudness.r128(x, sr, scratch=s_r)); t["r128_ms"].append(ms)
            _, ms = timed(lambda: loudness.integrated(x, sr, scratch=s_m)); t["meter_alt_ms"].append(ms)
            _, ms = timed(lambda: (loudness.integrated(x, sr, scratch=s_m), loudness.true_peak(x, sr, scratch=s_p)))
            t["meter_plus_true_peak_ms"].append(ms)
    chunks = -(-n // loudness.chunk())
    audio = 4.0 * n * C
    must = {"meter_ms": 2 * audio + 8.0 * C * chunks * (4 + 4 + 4),                   # two reads; states, starts, pieces + peak
            "sosfilt_ms": 3 * audio + 8.0 * C * chunks * (4 + 4), "scale_ms": 2 * audio,
            "true_peak_ms": audio,                                                    # x once; the partials are 16 B per 8 KB
            "r128_ms": 3 * audio + 8.0 * C * chunks * (4 + 4 + 4 + 3)}                # + the read of the peak kernel, the 3 s pieces
    m = meter.cpu().numpy()
    res = {"tool": "loudness_bench", "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "sr": sr, "C": C, "n": n,
           "rounds": a.rounds, "chunk": loudness.chunk(), "tile": loudness.tile(), "lufs": float(m[0]), "blocks": int(m[2]),
           "kept": int(m[1])}
    for k, v in t.items():
        res[k] = {"min": float(np.min(v)), "median": float(np.median(v))}
        if k in must:
            res[k]["bytes"] = must[k]
            res[k]["gb_per_s_at_min"] = must[k] / (res[k]["min"] * 1e-3) / 1e9
    rp = report.cpu().numpy()
    res["r128"] = dict(zip(loudness.REPORT, (float(v) for v in rp)))
    res["r128"]["oversampling"] = loudness.oversampling(sr)
    res["r128"]["short_term_blocks"] = loudness.short_term_blocks(n, sr)
    res["true_peak_ms"]["roof_ms"] = audio / (a.hbm_gb_per_s * 1e9) * 1e3
    res["true_peak_ms"]["fraction_of_roof_at_min"] = res["true_peak_ms"]["roof_ms"] / res["true_peak_ms"]["min"]
    res["true_peak_ms"]["gflop_per_s_at_min"] = 2.0 * 21 * loudness.oversampling(sr) * n * C / (res["true_peak_ms"]["min"] * 1e-3) / 1e9
    if a.hour_8k:
        nh = 3600 * 8000
        xh = (0.1 * torch.randn((nh, 1), generator=torch.Generator(device="cpu").manual_seed(1))).to(dev)
        s_h = torch.empty(loudness.r128_scratch_doubles(nh, 1, 8000), dtype=torch.float64, device=dev)
        s_hm = torch.empty(loudness.scratch_doubles(nh, 1, 8000), dtype=torch.float64, device=dev)
        s_hp = torch.empty(int(lib.wun_true_peak_scratch_doubles(nh, 1)), dtype=torch.float64, device=dev)
        loudness.r128(xh, 8000, scratch=s_h); loudness.integrated(xh, 8000, scratch=s_hm); loudness.true_peak(xh, 8000, scratch=s_hp)
        torch.cuda.synchronize()
        th = {"r128_ms": [], "meter_ms": [], "true_peak_ms": []}
        for _ in range(a.rounds):
            th["r128_ms"].append(timed(lambda: loudness.r128(xh, 8000, scratch=s_h))[1])
            th["meter_ms"].append(timed(lambda: loudness.integrated(xh, 8000, scratch=s_hm))[1])
            th["true_peak_ms"].append(timed(lambda: loudness.true_peak(xh, 8000, scratch=s_hp))[1])
        res["hour_8k_mono"] = {"n": nh, "short_term_blocks": loudness.short_term_blocks(nh, 8000),
                               "oversampling": loudness.oversampling(8000)}
        for k, v in th.items():
            res["hour_8k_mono"][k] = {"min": float(np.min(v)), "median": float(np.median(v))}
    if not a.no_host:
        from scipy.signal import sosfilt
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _loudness_np as ora
        xh = x.cpu().numpy()
        t0 = time.perf_counter(); sosfilt(sos, xh.astype(np.float64), axis=0); t1 = time.perf_counter()
        L = ora.loudness(xh, sr)[0]; t2 = time.perf_counter()
        res["host_s"] = {"scipy_sosfilt": t1 - t0, "numpy_meter": t2 - t1, "lufs": float(L), "cpus": len(os.sched_getaffinity(0))}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
