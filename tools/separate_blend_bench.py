#!/usr/bin/env python3
"""What the blend kernels cost beside the forward passes of a blended separation: a synthetic 3-minute
stereo two-source track at the model's rate, default hop, evaluate.separate_track(overlap=0.25, shifts=2).

  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o blend -- python tools/separate_blend_bench.py run
      the profiled process: ONE blended separation (and nothing else on the GPU but the upload and the download)
  python tools/separate_blend_bench.py report DIR [--out profiles/separate_blend_bench.json]
      reads DIR's *kernel_stats.csv: the summed time of blend_windows_kernel and blend_finish_kernel, the bytes they move (counted
      from the window table, below) against the achievable HBM rate, and their time beside every other kernel of the run (the
      forward passes and the two resampling kernels).  One JSON line on stdout, and the same in --out.

Bytes: per call of wun_blend_windows a frame with c > 0 covering windows in that call is read c times from `outputs` and its
accumulator is read and written ceil(c / 4) times (4 covering rows per launch), S C floats each, plus one den element each way per
launch; wun_blend_finish reads and writes preds once and reads den once per source.
"""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SECONDS, OVERLAP, SHIFTS, BATCH_HOPS, CONFIG = 180, 0.25, 2, 16, "baseline_stereo"
HBM_ACHIEVABLE_TBS = 6.3
COVER = 4                                # WUN_BLEND_COVER: covering rows one launch takes per run


def _geometry():
    import numpy as np
    import wave_u_net_amd as wun
    from wave_u_net_amd import blend
    from wave_u_net_amd.evaluate import blend_options, hop_geometry
    cfg = wun.get_config(CONFIG)
    sep = wun.UnetAudioSeparator(cfg)
    n = SECONDS * int(cfg["expected_sr"])
    tin, tout = hop_geometry(cfg, sep, n)
    _, offsets = blend_options(OVERLAP, SHIFTS, None, cfg["expected_sr"])
    v = min(int(round(OVERLAP * tout)), tout - 1)
    table = blend.window_table(tout, n, v, offsets)
    S, C = len(cfg["source_names"]), 1 if cfg["mono_downmix"] else 2
    batch = min(BATCH_HOPS, table.shape[0])
    rows, rmw = 0, 0                                                             # frames read from outputs / accumulator round trips
    for k in range(0, table.shape[0], batch):
        pos = table[k:k + batch, 0]
        lo, hi = int(max(pos.min(), 0)), int(min(pos.max() + tout, n))
        c = np.zeros(hi - lo + 1, np.int64)
        for p in pos.tolist():
            a, b = max(p, lo), min(p + tout, hi)
            if a < b:
                c[a - lo] += 1
                c[b - lo] -= 1
        c = np.cumsum(c)[:-1]
        rows += int(c.sum())
        rmw += int((-(-c // COVER)).sum())
    blend_bytes = 4 * (S * C * (rows + 2 * rmw) + 2 * rmw)
    finish_bytes = 4 * (2 * S * C * n + S * n)
    return cfg, {"frames": n, "input_frames": tin, "output_frames": tout, "overlap_frames": v, "shift_offsets": offsets,
                 "windows": int(table.shape[0]), "plain_hops": -(-n // tout), "batch_hops": batch, "sources": S, "channels": C,
                 "blend_windows_MB": round(blend_bytes / 1e6, 1), "blend_finish_MB": round(finish_bytes / 1e6, 1)}


def run():
    import numpy as np
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.evaluate import separate_track
    cfg = wun.get_config(CONFIG)
    sep = wun.UnetAudioSeparator(cfg, device="cuda:0")
    C = 1 if cfg["mono_downmix"] else 2
    audio = np.random.default_rng(0).uniform(-0.5, 0.5, (SECONDS * int(cfg["expected_sr"]), C)).astype(np.float32)
    est = separate_track(cfg, sep, audio, cfg["expected_sr"], batch_hops=BATCH_HOPS, overlap=OVERLAP, shifts=SHIFTS)
    torch.cuda.synchronize()
    assert all(np.isfinite(v).all() for v in est.values())
    print("separated %d frames into %s" % (audio.shape[0], ", ".join(est)))


def report(folder, out):
    files = sorted(glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_stats.csv under %s" % folder)
    ns = {}
    calls = {}
    with open(files[-1]) as f:
        for row in csv.DictReader(f):
            ns[row["Name"]] = ns.get(row["Name"], 0.0) + float(row["TotalDurationNs"])
            calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    pick = lambda key: sum(v for k, v in ns.items() if key in k)
    count = lambda key: sum(v for k, v in calls.items() if key in k)
    cfg, geo = _geometry()
    t_blend, t_finish = pick("blend_windows_kernel"), pick("blend_finish_kernel")
    if t_blend == 0 or t_finish == 0:
        raise SystemExit("the trace holds no blend kernels: %s" % files[-1])
    total = sum(ns.values())
    res = dict(geo, tool="separate_blend_bench", config=CONFIG, seconds_of_audio=SECONDS, overlap=OVERLAP, shifts=SHIFTS,
               source="rocprofv3 --kernel-trace --stats, one separate_track call",
               blend_windows_ms=round(t_blend / 1e6, 3), blend_windows_launches=count("blend_windows_kernel"),
               blend_finish_ms=round(t_finish / 1e6, 3), blend_ms=round((t_blend + t_finish) / 1e6, 3),
               other_kernels_ms=round((total - t_blend - t_finish) / 1e6, 3),
               blend_share_of_kernel_time=round((t_blend + t_finish) / total, 5),
               blend_windows_TBs=round(geo["blend_windows_MB"] * 1e6 / (t_blend * 1e-9) / 1e12, 3),
               blend_finish_TBs=round(geo["blend_finish_MB"] * 1e6 / (t_finish * 1e-9) / 1e12, 3),
               hbm_achievable_TBs=HBM_ACHIEVABLE_TBS)
    line = json.dumps(res)
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["run", "report"])
    ap.add_argument("folder", nargs="?")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "run":
        run()
    else:
        if not args.folder:
            raise SystemExit("report needs the folder rocprofv3 wrote")
        report(args.folder, args.out)


if __name__ == "__main__":
    main()
