#!/usr/bin/env python3
"""What a backward pass for a subset of the variables costs, on the benchmarked plan: configs[1], M1 with
context, B = 16, 147443 -> 16389 samples, the pinned tuning table imported as bench.py does.

Each arm is one forward pass (training = 1) + one backward call:
  full_dmix     wun_backward with d_mix                   (the full pass an autograd caller with a mix that requires grad runs)
  full          wun_backward without d_mix
  input_only    wun_backward_select, nothing selected, d_mix
  decoder       wun_backward_select: interp_*, up convs, output layer
  head          wun_backward_select: the output layer only
  loss_full     wun_loss_backward
  loss_null     wun_loss_backward_select with select = NULL (must cost what loss_full costs)

  python tools/backward_select_cost.py [--rounds 7] [--iters 20]
      HIP events on the launch stream around `iters` back-to-back iterations of one arm; the arms interleaved for `rounds`
      rounds; per arm the minimum over the rounds of (time / iters).  One JSON line on stdout.
  python tools/backward_select_cost.py --trace --iters 10
      runs every arm `iters` times with a marker kernel (a torch cumsum) between the arms, for
      rocprofv3 --kernel-trace --stats -d DIR -o run -- python tools/backward_select_cost.py --trace --iters 10
  python tools/backward_select_cost.py --count DIR/.../run_kernel_trace.csv --iters 10
      kernel launches per iteration of each arm from that trace (host dispatch order, split at the markers).
"""
import argparse
import ctypes as C
import csv
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ARMS = ["full_dmix", "full", "input_only", "decoder", "head", "loss_full", "loss_null"]
MARKER = "scan"      # substring of the marker kernel's name (torch.cumsum)


def setup():
    import torch
    import wave_u_net_amd as wun
    from wave_u_net_amd.training import Trainer, synthetic_source
    cfg = wun.get_config("m1_context")
    tr = Trainer(cfg, batch_size=16)
    mix, targets = synthetic_source(cfg, 16, tr.t_in, tr.t_out, tr.device, seed=1337)()
    table = os.path.join(ROOT, "profiles", "round6_tune_table.txt")
    tr.tune(mix, targets, pinned_table=open(table).read())
    sep = tr.sep
    names = [n for n, _, _ in sep._active.tensors]
    L = cfg["num_layers"]
    decoder = [n for n in names if n.startswith("separator/interp_")]
    nconv = sum(1 for n in names if n.endswith("/kernel"))
    conv = ["separator/conv1d" if c == 0 else "separator/conv1d_%d" % c for c in range(nconv)]
    head = [c + kb for c in conv[2 * L + 1:] for kb in ("/kernel", "/bias")]
    decoder += [c + kb for c in conv[L + 1:2 * L + 1] for kb in ("/kernel", "/bias")] + head
    masks = {"input_only": sep.select_mask([]), "decoder": sep.select_mask(decoder), "head": sep.select_mask(head)}
    tg = targets.to(torch.float32).contiguous()
    sep.get_output(mix, True)
    dout = (2.0 / tg.numel()) * (sep._outs[sep._last_key] - tg)
    dmix = torch.empty(tuple(mix.shape), device=mix.device)
    loss = torch.empty((), device=mix.device)
    lib = sep._lib
    plan = sep._active.handle

    def step(arm):
        sep.get_output(mix, True)
        ws, outs = sep._ws[sep._last_key].data_ptr(), sep._outs[sep._last_key].data_ptr()
        pr, g, st = sep.params.data_ptr(), sep.grads.data_ptr(), sep._stream()
        if arm in ("full_dmix", "full"):
            rc = lib.wun_backward(plan, pr, None, ws, outs, dout.data_ptr(), g, dmix.data_ptr() if arm == "full_dmix" else None, st)
        elif arm in masks:
            m = masks[arm]
            rc = lib.wun_backward_select(plan, pr, None, ws, outs, dout.data_ptr(), g if m.any() else None,
                                         dmix.data_ptr() if arm == "input_only" else None, st, None, None, 0,
                                         m.ctypes.data_as(C.POINTER(C.c_uint8)), int(m.size))
        elif arm == "loss_full":
            rc = lib.wun_loss_backward(plan, pr, None, ws, outs, tg.data_ptr(), g, loss.data_ptr(), st)
        else:
            rc = lib.wun_loss_backward_select(plan, pr, None, ws, outs, tg.data_ptr(), g, loss.data_ptr(), st, None, None, 0,
                                              None, 0)
        if rc:
            raise RuntimeError("%s: rc %d: %s" % (arm, rc, lib.wun_last_error().decode()))
    return torch, step


def timed(rounds, iters):
    torch, step = setup()
    for arm in ARMS:                                              # warm-up
        for _ in range(3):
            step(arm)
    torch.cuda.synchronize()
    best = {a: float("inf") for a in ARMS}
    allr = {a: [] for a in ARMS}
    for r in range(rounds):
        order = ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]      # rotate the order each round
        for arm in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                step(arm)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / iters
            allr[arm].append(round(ms, 4))
            best[arm] = min(best[arm], ms)
    print(json.dumps({"what": "forward + backward, ms per iteration (min over rounds)", "rounds": rounds, "iters": iters,
                      "min_ms": {a: round(best[a], 4) for a in ARMS}, "rounds_ms": allr}))


def trace(iters):
    torch, step = setup()
    x = torch.ones(64, device="cuda")
    torch.cuda.synchronize()
    for arm in ARMS:
        torch.cumsum(x, 0)
        for _ in range(iters):
            step(arm)
        torch.cumsum(x, 0)
    torch.cuda.synchronize()


def count(path, iters):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    key = "Dispatch_Id" if "Dispatch_Id" in rows[0] else "Correlation_Id"
    rows.sort(key=lambda r: int(r[key]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, n in enumerate(names) if MARKER in n.lower()]
    if len(marks) != 2 * len(ARMS):
        raise SystemExit("expected %d marker kernels, found %d" % (2 * len(ARMS), len(marks)))
    out = {}
    for k, arm in enumerate(ARMS):
        seg = names[marks[2 * k] + 1:marks[2 * k + 1]]
        fams = {}
        for n in seg:
            fam = n.split("<")[0].split("(")[0].strip()
            fams[fam] = fams.get(fam, 0) + 1
        out[arm] = {"kernels_per_iter": len(seg) / iters,
                    "families_per_iter": {f: c / iters for f, c in sorted(fams.items(), key=lambda t: -t[1])}}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--count", metavar="KERNEL_TRACE_CSV")
    a = ap.parse_args()
    if a.count:
        count(a.count, a.iters)
    elif a.trace:
        trace(a.iters)
    else:
        timed(a.rounds, a.iters)


if __name__ == "__main__":
    main()
