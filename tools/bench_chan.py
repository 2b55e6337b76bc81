#!/usr/bin/env python
"""Dev tool (GPU box): the FNO at in_chan = out_chan = N -- the fused training step (FnoTrainEngine, B = 256, 64 x 64, modes 12,
width 20, L = 4) and the 200-step rollout of 64 cases (FnoRollout, 66 x 65) -- for N in 2, 3, 4, 8 on one build, with the per-kernel
split of the step (cfd_prof).  N = 2 runs the pair kernels and the one-pass training head, N > 2 the head's channel route.

    python tools/bench_chan.py [--chans 2 3 4 8] [--batch 256] [--hidden 20] [--window 1.0] [--json profiles/chan_step.json]
    python tools/bench_chan.py --chans 4 --trace-steps 5      (a few plain steps and nothing else: the program of a kernel trace)

Timing: device events around a window of at least --window seconds of back-to-back steps after a warm-up; one JSON line per leg."""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cfdbench_amd import _lib  # noqa: E402
from cfdbench_amd.engine import FnoTrainEngine  # noqa: E402
from cfdbench_amd.models.fno.fno2d import Fno2d  # noqa: E402
from cfdbench_amd.models.loss import loss_name_to_fn  # noqa: E402
from cfdbench_amd.rollout import FnoRollout  # noqa: E402


def read_prof(api):
    buf = ctypes.create_string_buffer(1 << 16)
    api.call("cfd_prof_end", buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        rows.append(dict(kernel=f[0], launches=int(f[1]), ms=float(f[2])))
    return sorted(rows, key=lambda r: -r["ms"])


def timed_window(fn, warmup, window_s):
    """Seconds per call from device events: `warmup` calls, a probe of 3 calls to size the window, then >= window_s of calls."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    per = a.elapsed_time(b) / 3e3
    n = max(3, int(window_s / max(per, 1e-6)) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n, n


def make_model(N, C, L, p, dev):
    torch.manual_seed(0)
    return Fno2d(N, N, p, loss_name_to_fn("nmse"), L, 12, 12, C).to(dev)


def step_inputs(N, B, H, W, p, dev):
    g = torch.Generator(device="cpu").manual_seed(1234)
    inputs = torch.randn(B, N, H, W, generator=g)
    label = inputs + 0.1 * torch.randn(B, N, H, W, generator=g)
    return inputs.to(dev), label.to(dev), torch.randn(B, p, generator=g).to(dev), torch.ones(B, 1, H, W, device=dev)


def step_leg(api, args, N, dev):
    B, H, W, p, C, L = args.batch, 64, 64, 5, args.hidden, args.layers
    inputs, label, cp, mask = step_inputs(N, B, H, W, p, dev)
    eng = FnoTrainEngine(make_model(N, C, L, p, dev), lr=1e-3, loss_name="nmse")
    step = lambda: eng.train_step(inputs, label, cp, mask)  # noqa: E731
    sec, n = timed_window(step, args.warmup, args.window)
    api.call("cfd_prof_begin")
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    rows = read_prof(api)
    kernels = [dict(kernel=r["kernel"], launches=r["launches"] // 3, us_per_step=round(r["ms"] / 3 * 1e3, 2)) for r in rows]
    return dict(leg="fused_step", chans=N, batch=B, hidden=C, layers=L, grid=f"{H}x{W}", ms_per_step=round(sec * 1e3, 4), steps_timed=n,
                kernels=kernels)


def rollout_leg(args, N, dev):
    B, H, W, p, steps = args.rollout_batch, 66, 65, 5, args.rollout_steps
    g = torch.Generator(device="cpu").manual_seed(99)
    x0 = torch.randn(B, N, H, W, generator=g).to(dev)
    cp = torch.randn(B, p, generator=g).to(dev)
    mask = torch.ones(B, 1, H, W, device=dev)
    mask[:, :, 0, :] = 0
    mask[:, :, -1, :] = 0
    mask[:, :, :, 0] = 0
    ro = FnoRollout(make_model(N, args.hidden, args.layers, p, dev).eval())
    run = lambda: ro.generate_frames(x0, cp, mask, steps)  # noqa: E731
    sec, n = timed_window(run, 1, args.window)  # (the warm-up call builds and captures the graph)
    return dict(leg="rollout", chans=N, cases=B, steps=steps, hidden=args.hidden, layers=args.layers, grid=f"{H}x{W}",
                ms_per_step=round(sec / steps * 1e3, 4), frames_per_s=round(B * steps / sec, 1), rollouts_timed=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chans", nargs="*", type=int, default=[2, 3, 4, 8])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back calls per timed leg (at least)")
    ap.add_argument("--rollout-batch", type=int, default=64)
    ap.add_argument("--rollout-steps", type=int, default=200)
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--trace-steps", type=int, default=0, help="run this many plain training steps per channel count and exit")
    ap.add_argument("--json", default="profiles/chan_step.json")
    args = ap.parse_args()
    api = _lib.api()
    dev = torch.device("cuda", 0)
    if args.trace_steps:
        for N in args.chans:
            inputs, label, cp, mask = step_inputs(N, args.batch, 64, 64, 5, dev)
            eng = FnoTrainEngine(make_model(N, args.hidden, args.layers, 5, dev), lr=1e-3, loss_name="nmse")
            for _ in range(args.trace_steps):
                eng.train_step(inputs, label, cp, mask)
            torch.cuda.synchronize()
        return
    out = []
    for N in args.chans:
        out.append(step_leg(api, args, N, dev))
        print(json.dumps(out[-1]), flush=True)
        if not args.no_rollout:
            out.append(rollout_leg(args, N, dev))
            print(json.dumps(out[-1]), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
