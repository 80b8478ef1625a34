#!/usr/bin/env python3
"""What Griffin-Lim phase reconstruction costs, on a synthetic 3-minute mono track at 22 050 Hz, 32 iterations
from a random initial spectrum, centred framing, at 2048 / 512 and at 4096 / 1024.

Arms (HIP events on the launch stream around one call of 32 iterations, buffers resident in HBM, scratch allocated once):
  gl_<n_fft>         wun_griffin_lim: per iteration and block of 256 frames one gl_frame_kernel launch (samples -> FFT -> projection
                     -> inverse FFT -> windowed frame inside a workgroup's LDS) and one istft_ola_kernel launch
  gl_fast_<n_fft>    the same with momentum 0.99: the frame kernel also reads and rewrites c_{i-1}
  composed_<n_fft>   the same iteration from the entries that existed before: wun_stft_complex_fft, the projection in torch
                     (eager elementwise kernels on Re, Im and mag), wun_istft_fft -- the spectrum goes through HBM twice

  python tools/griffin_lim_bench.py [--rounds 7] [--iterations 32] [--arms gl,composed] [--out profiles/griffin_lim_bench.json]
      the arms interleaved in ONE process for `rounds` rounds (order rotated each round); per arm the median, the minimum and
      the maximum over the rounds, and the bytes each arm has to move per iteration, computed from the shapes (`bytes_per_iteration`:
      unique floats in and out of every launch; the composed arm's torch projection counted as ONE fused pass, which eager torch
      does not reach).  One JSON line on stdout, and the same in --out.  There is no target.  bench.py does not run this code.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SECONDS, SR = 180, 22050
RESOLUTIONS = [(2048, 512), (4096, 1024)]


def bytes_per_iteration(T, n_fft, hop, F):
    K = n_fft // 2 + 1
    frames, spec, audio = 4 * F * n_fft, 4 * F * K, 4 * T
    gl = {"frame_kernel": audio + spec + frames, "overlap_add": frames + audio}
    fast = {"frame_kernel": audio + spec + frames + 4 * spec, "overlap_add": frames + audio}
    composed = {"stft": audio + 2 * spec, "projection_fused": 3 * spec + 2 * spec, "inverse_frames": 2 * spec + frames,
                "overlap_add": frames + audio}
    return {"gl": dict(gl, total=sum(gl.values())), "gl_fast": dict(fast, total=sum(fast.values())),
            "composed": dict(composed, total=sum(composed.values()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--seconds", type=int, default=SECONDS)
    ap.add_argument("--arms", default="gl,gl_fast,composed")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    from wave_u_net_amd import _lib, spectral

    assert torch.cuda.is_available(), "this benchmark needs an MI355X"
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    T = args.seconds * SR
    kinds = [a for a in args.arms.split(",") if a]
    stream = lambda: C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731

    arms, info = {}, {}
    for n_fft, hop in RESOLUTIONS:
        lead, F = n_fft - hop, spectral.centered_frames(T, n_fft, hop, "fft")
        K = n_fft // 2 + 1
        g = torch.Generator(device=dev).manual_seed(n_fft)
        mag = torch.rand((1, F, K), generator=g, device=dev) * 10.0
        re0 = torch.rand((1, F, K), generator=g, device=dev)
        im0 = (torch.rand((1, F, K), generator=g, device=dev) * 2.0 - 1.0) * 3.141592653589793
        y = torch.empty((1, T), device=dev)
        table = spectral._fft_table(n_fft, dev)
        scratch = torch.empty(int(lib.wun_griffin_lim_scratch_floats(1, 1, T, 1, n_fft, hop, lead, F, 1)), device=dev)
        iscratch = torch.empty(int(lib.wun_istft_fft_scratch_floats(1, 1, T, 1, n_fft, hop, lead, F)), device=dev)
        re, im = torch.empty_like(re0), torch.empty_like(im0)
        info["%d/%d" % (n_fft, hop)] = {"frames": F, "samples": T, "bytes_per_iteration": bytes_per_iteration(T, n_fft, hop, F)}

        def gl(momentum, n_fft=n_fft, hop=hop, lead=lead, F=F, mag=mag, re0=re0, im0=im0, y=y, scratch=scratch):
            spectral.griffin_lim_call(mag, re0, im0, None, T, n_fft, hop, lead, args.iterations, momentum, y=y, scratch=scratch)

        def composed(n_fft=n_fft, hop=hop, lead=lead, F=F, mag=mag, re0=re0, im0=im0, y=y, re=re, im=im, table=table,
                     iscratch=iscratch):
            cr, ci = re0, im0
            for i in range(args.iterations):
                if i:
                    _lib.check(lib.wun_stft_complex_fft(y.data_ptr(), 1, 1, T, 1, n_fft, hop, lead, F, table.data_ptr(),
                                                        re.data_ptr(), im.data_ptr(), stream()))
                    cr, ci = re, im
                # the projection as a user of torch would write it (unit(0) = 1 through the clamp's where)
                a = torch.sqrt(cr * cr + ci * ci)
                zero = a == 0
                s = mag / torch.where(zero, torch.ones_like(a), a)
                sr, si = torch.where(zero, mag, cr * s), ci * s
                _lib.check(lib.wun_istft_fft(sr.data_ptr(), si.data_ptr(), 1, 1, T, 1, n_fft, hop, lead, F, table.data_ptr(),
                                             y.data_ptr(), iscratch.data_ptr(), stream()))

        if "gl" in kinds:
            arms["gl_%d" % n_fft] = lambda gl=gl: gl(0.0)
        if "gl_fast" in kinds:
            arms["gl_fast_%d" % n_fft] = lambda gl=gl: gl(0.99)
        if "composed" in kinds:
            arms["composed_%d" % n_fft] = composed

    names = list(arms)
    with torch.cuda.device(dev):
        for a in names:                                  # warm-up: every shape the timed window uses
            arms[a]()
        torch.cuda.synchronize()
        ms = {a: [] for a in names}
        for r in range(args.rounds):
            for a in names[r % len(names):] + names[:r % len(names)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                arms[a]()
                e1.record()
                e1.synchronize()
                ms[a].append(e0.elapsed_time(e1))
    result = {"tool": "griffin_lim_bench", "device": torch.cuda.get_device_name(dev), "seconds": args.seconds, "sample_rate": SR,
              "iterations": args.iterations, "rounds": args.rounds, "shapes": info,
              "ms_per_call": {a: {"median": statistics.median(v), "min": min(v), "max": max(v)} for a, v in ms.items()},
              "ms_per_iteration_median": {a: statistics.median(v) / args.iterations for a, v in ms.items()}}
    line = json.dumps(result, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, sort_keys=True, indent=1) + "\n")


if __name__ == "__main__":
    main()
