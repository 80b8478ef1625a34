"""Times the three steps of BSS Eval scoring on a synthetic 3-minute, 44.1 kHz, stereo, two-source track:
correlations (wun_bss_correlations), the filter solve (torch.linalg, host and device), window energies
(wun_bss_window_energies).  HIP events around each step, the steps interleaved over `--rounds` rounds, min and median reported;
the achieved float64 FLOP/s of the correlation kernel is 2 * A * 2A * L * n over its time.  `--oracle` also times the numpy
oracle (tests/_bsseval_np.py) on the same track with the host's usable cores.  Prints one JSON line; --out writes it to a file.

  python tools/bsseval_bench.py --rounds 5 --out profiles/bsseval_bench.json [--oracle] [--seconds 180]
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
from wave_u_net_amd import bsseval  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--sources", type=int, default=2)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--filters-len", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--device-solve", action="store_true", help="also time torch.linalg on the GPU")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU: timings on a CPU say nothing"
    dev = torch.device("cuda:0")
    S, C, L, n = a.sources, a.channels, a.filters_len, int(a.seconds * a.sr)
    A = S * C
    g = torch.Generator(device="cpu").manual_seed(0)
    refs = (0.3 * torch.randn((S, n, C), generator=g)).to(dev)
    ests = (refs + 0.1 * refs.flip(0) + 0.05 * torch.randn((S, n, C), generator=g).to(dev)).contiguous()
    starts, lengths = bsseval.window_table(n, a.sr, a.sr)
    scratch = torch.empty(bsseval.scratch_doubles(S, n, C, L, len(starts), max(lengths)), dtype=torch.float64, device=dev)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); e1.synchronize()
        return out, e0.elapsed_time(e1)

    def host_timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return out, 1e3 * (time.perf_counter() - t0)

    R, D = bsseval.correlations(refs, ests, L, scratch)                              # warm-up of every step
    c_all, c_own = bsseval.solve_filters(R, D, S, C)
    bsseval.window_energies(refs, ests, starts, lengths, c_all, c_own, scratch=scratch)
    bsseval.window_energies(refs, ests, starts, lengths, scratch=scratch)
    if a.device_solve:
        bsseval.solve_filters(R, D, S, C, solve_device="device")
    t = {"correlations_ms": [], "solve_host_ms": [], "solve_device_ms": [], "energies_ms": [], "energies_sdr_only_ms": []}
    for _ in range(a.rounds):
        (R, D), ms = timed(lambda: bsseval.correlations(refs, ests, L, scratch)); t["correlations_ms"].append(ms)
        (c_all, c_own), ms = host_timed(lambda: bsseval.solve_filters(R, D, S, C)); t["solve_host_ms"].append(ms)
        if a.device_solve:
            _, ms = host_timed(lambda: bsseval.solve_filters(R, D, S, C, solve_device="device")); t["solve_device_ms"].append(ms)
        _, ms = timed(lambda: bsseval.window_energies(refs, ests, starts, lengths, c_all, c_own, scratch=scratch))
        t["energies_ms"].append(ms)
        _, ms = timed(lambda: bsseval.window_energies(refs, ests, starts, lengths, scratch=scratch))
        t["energies_sdr_only_ms"].append(ms)
    res = {"tool": "bsseval_bench", "device": torch.cuda.get_device_name(0), "seconds": a.seconds, "sr": a.sr, "S": S, "C": C,
           "L": L, "n": n, "windows": len(starts), "rounds": a.rounds}
    for k, v in t.items():
        if v:
            res[k] = {"min": float(np.min(v)), "median": float(np.median(v))}
    corr_flop = 2.0 * A * 2 * A * L * n
    res["correlation_flop"] = corr_flop
    res["correlation_f64_tflops_at_min"] = corr_flop / (res["correlations_ms"]["min"] * 1e-3) / 1e12
    proj_flop = 2.0 * S * (n + len(starts) * (L - 1)) * (A * L * C + C * L * C)
    res["projection_flop"] = proj_flop
    res["projection_f64_tflops_at_min"] = proj_flop / (res["energies_ms"]["min"] * 1e-3) / 1e12
    if a.oracle:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _bsseval_np as ora
        r, e = refs.cpu().numpy(), ests.cpu().numpy()
        t0 = time.perf_counter(); Ro, Do = ora.correlations(r, e, L); t1 = time.perf_counter()
        ca, co = ora.filters(Ro, Do, S, C); t2 = time.perf_counter()
        ora.window_energies(r, e, starts, lengths, ca, co); t3 = time.perf_counter()
        res["oracle_s"] = {"correlations": t1 - t0, "solve": t2 - t1, "energies": t3 - t2, "cpus": len(os.sched_getaffinity(0)),
                           "omp_num_threads": os.environ.get("OMP_NUM_THREADS")}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
