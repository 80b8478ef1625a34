#!/usr/bin/env python3
"""What a training batch costs to PRODUCE beside the step that consumes it, on synthetic tracks resident in HBM.

Arms (the same snippet stream, seed and residency):
  torch        datasets.DeviceSnippetSource: two pageable host-to-device copies, an int64 index tensor [B, Tin], one advanced-indexing
               gather per source, a broadcast multiply, S - 1 adds, a strided crop, two .contiguous() copies
  fused        datasets.FusedSnippetSource: one wun_gather_snippets launch, the descriptor table in its arguments
  fused_aug    the same with augment = {"remix": 1, "channel_swap": .5, "polarity": .5} (channel_swap on stereo shapes only)
  fused_speed  the same with augment = {"speed": 1} and the default rates: every source resampled inside the one launch
               (wun_gather_snippets_speed)
  fused_pitch / fused_stretch   the same with augment = {"pitch_shift": 1} / {"time_stretch": 1} and the default ratios and
               resolution (n_fft 2048, hop 512): every source of every row is one job of the phase vocoder (wun_time_stretch,
               DESIGN.md 5.24: four launches per 64 jobs) into a slot behind its plane, then the one gather, which resamples
               the slots for fused_pitch.  kernel_ms is both entries called directly on one batch; `vocoder_split_ms` splits
               one such call by kernel (the library's event brackets, wun_profile_begin / wun_profile_end).
  composed     the same batch without the fused resampling: B x S wun_resample launches of the spans into temporary planes, then
               one wun_gather_snippets over them, the C entries called directly (device and kernel columns only).  As a
               producer (device column) it draws its table and rates from fused_speed's stream and allocates its outputs per
               call like the other producers; the temporary planes are allocated once.  composed_direct is the same launches
               on ONE table with preallocated outputs and nothing drawn (device column; it is also what the kernel column
               times).  The output is compared with fused_speed's bit for bit before anything is timed.
  d2d_copy     one device-to-device copy of as many bytes as the fused kernel has to move (read + written), for the copy-rate fraction
  fixed        (step loop only) no producer: Trainer.step() on one resident batch, what bench.py times

Shapes: m1_context (BASELINE.json configs[1]: S = 2, C = 1, B = 16, 147 443 -> 16 389 frames) and full_multi_instrument (S = 4, C = 2).

Per arm and shape, the arms interleaved in ONE process (order rotated each round), median (min .. max) over the rounds:
  device_ms_per_call   HIP events on the stream around ONE call
  wall_ms_per_call     host wall-clock of 100 calls enqueued back to back and synchronised once, / 100
  loop_ms_per_iter     host wall-clock of 50 iterations of `producer(); Trainer.step()`, synchronised once, / 50
  kernel_ms            HIP events around 50 launches enqueued back to back, / 50: wun_gather_snippets called directly on one
                       table and preallocated outputs (fused, fused_aug, fused_speed; composed: 50 times its B x S + 1 launches), and
                       50 d2d copies -- one call of a producer is too short
                       for its bracket to show the kernel (the bracket of device_ms_per_call also holds the host's work between
                       the two records: drawing the descriptors, allocating the outputs)
and `copy_rate_fraction` = (d2d_copy median kernel_ms) / (fused median kernel_ms): the fused kernel's achieved bytes per second
against a plain copy of the same byte count.  For the speed arms: `speed_over_plain_kernel` (median kernel_ms of fused_speed / fused),
`speed_gfma_per_s` (the taps of the batch, sum over rows and sources of Tin C K, over the median kernel_ms) and
`fused_speed_below_composed` (median of fused_speed below the minimum of composed, kernel and device; and the device bracket
against composed_direct, which draws nothing).

  python tools/producer_bench.py [--rounds 9] [--loop-rounds 3] [--shapes m1_context,full_multi_instrument] [--out profiles/producer_bench.json]
One JSON line on stdout, and the same in --out.  bench.py does not run this code.  m1_context steps run the pinned tilings of
profiles/round6_tune_table.txt; full_multi_instrument has no committed table and runs the heuristic tilings (no autotuning here).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SR, TRACKS, SECONDS = 22050, 12, 60
PINNED = {"m1_context": os.path.join(ROOT, "profiles", "round6_tune_table.txt")}


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--loop-rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--shapes", default="m1_context,full_multi_instrument")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd import _lib, datasets, resample, vocoder
    from wave_u_net_amd.training import Trainer

    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    result = {"tool": "producer_bench", "device": torch.cuda.get_device_name(dev), "rounds": args.rounds,
              "loop_rounds": args.loop_rounds, "calls": args.calls, "iterations": args.iterations, "shapes": {}}

    for name in [s for s in args.shapes.split(",") if s]:
        cfg = wun.get_config(name)
        tr = Trainer(cfg, batch_size=args.batch)
        S, C, B = len(cfg["source_names"]), 1 if cfg["mono_downmix"] else 2, tr.batch
        rng = np.random.default_rng(7)
        tracks = [datasets.make_track({k: rng.uniform(-0.3, 0.3, (SECONDS * SR, C)).astype(np.float32)
                                       for k in cfg["source_names"]}, cfg) for _ in range(TRACKS)]
        augment = {"remix": 1, "polarity": .5}
        if C == 2:
            augment["channel_swap"] = .5
        producers = {
            "torch": datasets.DeviceSnippetSource(cfg, tracks, tr.t_in, tr.t_out, B, dev, seed=1),
            "fused": datasets.FusedSnippetSource(cfg, tracks, tr.t_in, tr.t_out, B, dev, seed=1),
            "fused_aug": datasets.FusedSnippetSource(cfg, tracks, tr.t_in, tr.t_out, B, dev, seed=1, augment=augment),
            "fused_speed": datasets.FusedSnippetSource(cfg, tracks, tr.t_in, tr.t_out, B, dev, seed=1, augment={"speed": 1}),
            "fused_pitch": datasets.FusedSnippetSource(cfg, tracks, tr.t_in, tr.t_out, B, dev, seed=1, augment={"pitch_shift": 1}),
            "fused_stretch": datasets.FusedSnippetSource(cfg, tracks, tr.t_in, tr.t_out, B, dev, seed=1, augment={"time_stretch": 1}),
        }
        del tracks
        # what the fused kernel moves (mix_mode 1): every source window read, the mix and the cropped targets written
        kernel_bytes = 4 * B * C * (S * tr.t_in + tr.t_in + S * tr.t_out)
        a = torch.empty(kernel_bytes // 8, dtype=torch.float32, device=dev)
        b = torch.empty_like(a)
        # composed: the spans of fused_speed's next batch resampled one by one into temporary planes, then the plain gather
        sp = producers["fused_speed"]
        sp_table, sp_rates = sp.descriptors().copy(), sp.rates().copy()
        assert sp_rates.all()                                       # every source of every row is resampled
        tmp = [torch.zeros((B * tr.t_in, C), dtype=torch.float32, device=dev) for _ in range(S)]
        tmp_planes = (_lib.C.c_void_p * S)(*[t.data_ptr() for t in tmp])
        tmp_table = sp_table.copy()
        tmp_table["start"] = (np.arange(B, dtype=np.int64) * tr.t_in)[:, None]
        c_outs = (torch.empty((B, tr.t_in, C), dtype=torch.float32, device=dev),
                  torch.empty((S, B, tr.t_out, C), dtype=torch.float32, device=dev))
        spans = []
        for bi in range(B):
            for si, k in enumerate(sp.names):
                up, down = sp.speed_rates[sp_rates[bi, si] - 1]
                spans.append((sp.data[k].data_ptr() + int(sp_table["start"][bi, si]) * C * 4,
                              datasets.speed_source_frames(tr.t_in, up, down), tmp[si].data_ptr(), bi * tr.t_in,
                              sp._tables[sp_rates[bi, si] - 1].data_ptr(), up, down))
        speed_taps = sum(tr.t_in * C * resample.design(*sp.speed_rates[r - 1]).shape[1] for r in sp_rates.ravel())

        def composed():
            st = torch.cuda.current_stream(dev).cuda_stream
            for x, n_src, y, y_off, tab, up, down in spans:
                _lib.check(lib.wun_resample(x, n_src, C, y, y_off, tr.t_in, C, tab, up, down, st))
            _lib.check(lib.wun_gather_snippets(tmp_planes, None, B * tr.t_in, C, S, B, tr.t_in, tr.t_out, tmp_table.ctypes.data, 1,
                                               c_outs[0].data_ptr(), c_outs[1].data_ptr(), st))

        # ... and as a producer: the stream fused_speed consumes, drawn per call (the planes are the padded tracks one behind the other)
        pad = (tr.t_in - tr.t_out) // 2
        draw = datasets.speed_descriptors(cfg, [SECONDS * SR + 2 * pad] * TRACKS, tr.t_in, tr.t_out, np.random.default_rng(1),
                                          {"speed": 1}, np.random.default_rng([1, 1]))

        def composed_producer():
            rows = [next(draw) for _ in range(B)]
            table, rates = np.stack([r[0] for r in rows]), np.stack([r[2] for r in rows])
            mix_o = torch.empty((B, tr.t_in, C), dtype=torch.float32, device=dev)
            tgt_o = torch.empty((S, B, tr.t_out, C), dtype=torch.float32, device=dev)
            st = torch.cuda.current_stream(dev).cuda_stream
            for bi in range(B):
                for si, k in enumerate(sp.names):
                    up, down = sp.speed_rates[rates[bi, si] - 1]
                    _lib.check(lib.wun_resample(sp.data[k].data_ptr() + int(table["start"][bi, si]) * C * 4,
                                                datasets.speed_source_frames(tr.t_in, up, down), C, tmp[si].data_ptr(), bi * tr.t_in,
                                                tr.t_in, C, sp._tables[rates[bi, si] - 1].data_ptr(), up, down, st))
            table["start"] = tmp_table["start"]
            _lib.check(lib.wun_gather_snippets(tmp_planes, None, B * tr.t_in, C, S, B, tr.t_in, tr.t_out, table.ctypes.data, 1,
                                               mix_o.data_ptr(), tgt_o.data_ptr(), st))
            return mix_o, tgt_o
        arms = dict(producers, composed=composed_producer, composed_direct=composed, d2d_copy=lambda: b.copy_(a))
        names = list(arms)

        with torch.cuda.device(dev):
            mix, targets = producers["fused"]()
            ttx = producers["torch"]()
            assert torch.equal(mix, ttx[0]) and torch.equal(targets, ttx[1])      # the arms produce the same batches
            composed()
            cmix, ctargets = composed_producer()                                 # (draws the same first batch)
            smix, stargets = sp()                                                # (the batch sp_table / sp_rates describe)
            assert torch.equal(smix, c_outs[0]) and torch.equal(stargets, c_outs[1])
            assert torch.equal(smix, cmix) and torch.equal(stargets, ctargets)
            del smix, stargets, cmix, ctargets
            pinned = PINNED.get(name) if B == 16 else None
            if pinned and os.path.exists(pinned) and "WUN_NO_TUNE" not in os.environ:
                tr.tune(mix, targets, pinned_table=open(pinned).read())
            for k in names:
                arms[k]()
            tr.step(mix, targets)
            torch.cuda.synchronize()

            dev_ms = {k: [] for k in names}
            for r in range(args.rounds):
                for k in names[r % len(names):] + names[:r % len(names)]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    arms[k]()
                    e1.record()
                    e1.synchronize()
                    dev_ms[k].append(e0.elapsed_time(e1))

            # the kernel alone: one table, preallocated outputs, 50 launches per bracket
            lib_src = {"fused": producers["fused"], "fused_aug": producers["fused_aug"]}
            tables = {k: p.descriptors().copy() for k, p in lib_src.items()}
            outs = (torch.empty_like(mix), torch.empty_like(targets))
            stream = torch.cuda.current_stream(dev).cuda_stream

            def launch(k):
                p = lib_src[k]
                _lib.check(lib.wun_gather_snippets(p._planes, p.data["mix"].data_ptr(), p.plane_frames, C, S, B, tr.t_in, tr.t_out,
                                                   tables[k].ctypes.data, 1, outs[0].data_ptr(), outs[1].data_ptr(), stream))

            def launch_speed():
                _lib.check(lib.wun_gather_snippets_speed(sp._planes, None, sp.plane_frames, C, S, B, tr.t_in, tr.t_out,
                                                         sp_table.ctypes.data, sp_rates.ctypes.data, _lib.C.addressof(sp._bank), 1,
                                                         outs[0].data_ptr(), outs[1].data_ptr(), stream))
            # the vocoder arms: wun_time_stretch on the job table of one batch, then the gather on its descriptors
            voc = {}
            for k in ("fused_pitch", "fused_stretch"):
                p = producers[k]
                vt, vr, vj = p.descriptors().copy(), p.rates().copy(), p.jobs().copy()
                assert (vj[:, :, 1] > 0).all()                          # every source of every row is a job
                voc[k] = (p, vt, vr, p.job_table(vj, vr))

            def launch_vocoder(k):
                p, vt, vr, jt = voc[k]
                vocoder.run(jt, C, p.vocoder_fft[0], p.vocoder_fft[1], p._scratch, dev)
                _lib.check(lib.wun_gather_snippets_speed(p._planes, None, p.gather_frames, C, S, B, tr.t_in, tr.t_out,
                                                         vt.ctypes.data, vr.ctypes.data,
                                                         _lib.C.addressof(p._bank) if p._bank is not None else None, 1,
                                                         outs[0].data_ptr(), outs[1].data_ptr(), stream))
            kernels = {"fused": lambda: launch("fused"), "fused_aug": lambda: launch("fused_aug"), "fused_speed": launch_speed,
                       "fused_pitch": lambda: launch_vocoder("fused_pitch"), "fused_stretch": lambda: launch_vocoder("fused_stretch"),
                       "composed": composed, "d2d_copy": arms["d2d_copy"]}
            knames, reps = list(kernels), 50
            kernel_ms = {k: [] for k in knames}
            for r in range(args.rounds):
                for k in knames[r % len(knames):] + knames[:r % len(knames)]:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(reps):
                        kernels[k]()
                    e1.record()
                    e1.synchronize()
                    kernel_ms[k].append(e0.elapsed_time(e1) / reps)

            # one call of each vocoder arm split by kernel (ms per call; the brackets' overhead, once per launch, beside it)
            split = {}
            for k in voc:
                launch_vocoder(k)
                torch.cuda.synchronize()
                lib.wun_profile_begin()
                for _ in range(5):
                    launch_vocoder(k)
                torch.cuda.synchronize()
                buf = _lib.C.create_string_buffer(1 << 20)
                _lib.check(lib.wun_profile_end(buf, len(buf)))
                prof = json.loads(buf.value.decode())
                split[k] = {"bracket_overhead_ms": prof.get("bracket_overhead_ms"), "jobs": int(len(voc[k][3])),
                            "kernels": {e["name"]: {"launches_per_call": e["launches"] / 5.0, "ms_per_call": e["ms"] / 5.0}
                                        for e in prof["kernels"]}}

            wall_ms = {k: [] for k in producers}
            pnames = list(producers)
            for r in range(args.rounds):
                for k in pnames[r % len(pnames):] + pnames[:r % len(pnames)]:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        producers[k]()
                    torch.cuda.synchronize()
                    wall_ms[k].append((time.perf_counter() - t0) * 1e3 / args.calls)

            loops = dict(producers, fixed=lambda: (mix, targets))
            lnames = list(loops)
            loop_ms = {k: [] for k in lnames}
            for _ in range(5):                                   # settle the step
                tr.step(mix, targets)
            for r in range(args.loop_rounds):
                for k in lnames[r % len(lnames):] + lnames[:r % len(lnames)]:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iterations):
                        tr.step(*loops[k]())
                    torch.cuda.synchronize()
                    loop_ms[k].append((time.perf_counter() - t0) * 1e3 / args.iterations)

        fused_dev = statistics.median(dev_ms["fused"])
        fused_med, copy_med = statistics.median(kernel_ms["fused"]), statistics.median(kernel_ms["d2d_copy"])
        speed_med = statistics.median(kernel_ms["fused_speed"])
        result["shapes"][name] = {
            "sources": S, "channels": C, "batch": B, "input_frames": tr.t_in, "output_frames": tr.t_out,
            "resident_frames": int(producers["fused"].plane_frames), "kernel_bytes": kernel_bytes,
            "tilings": getattr(tr, "tune_source", None) or "heuristic",
            "device_ms_per_call": {k: stats(v) for k, v in dev_ms.items()},
            "kernel_ms": {k: stats(v) for k, v in kernel_ms.items()},
            "wall_ms_per_call": {k: stats(v) for k, v in wall_ms.items()},
            "loop_ms_per_iter": {k: stats(v) for k, v in loop_ms.items()},
            "fused_gb_per_s": kernel_bytes / (fused_med * 1e-3) / 1e9,
            "d2d_copy_gb_per_s": kernel_bytes / (copy_med * 1e-3) / 1e9,
            "copy_rate_fraction": copy_med / fused_med,
            "speed_over_plain_kernel": speed_med / fused_med,
            "vocoder_fft": list(voc["fused_pitch"][0].vocoder_fft), "vocoder_split_ms": split,
            "vocoder_over_plain_kernel": {k: statistics.median(kernel_ms[k]) / fused_med for k in voc},
            "speed_taps": int(speed_taps), "speed_gfma_per_s": speed_taps / (speed_med * 1e-3) / 1e9,
            "fused_speed_below_composed": {"kernel": speed_med < min(kernel_ms["composed"]),
                                           "device": statistics.median(dev_ms["fused_speed"]) < min(dev_ms["composed"]),
                                           "device_against_composed_direct":
                                               statistics.median(dev_ms["fused_speed"]) < min(dev_ms["composed_direct"])},
            "fused_not_slower": {"device": fused_dev <= statistics.median(dev_ms["torch"]),
                                 "wall": statistics.median(wall_ms["fused"]) <= statistics.median(wall_ms["torch"])},
        }
        del producers, arms, loops, kernels, lib_src, outs, voc, tr, a, b, mix, targets, ttx, sp, tmp, c_outs, spans, draw
        torch.cuda.empty_cache()

    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, sort_keys=True, indent=1) + "\n")


if __name__ == "__main__":
    main()
