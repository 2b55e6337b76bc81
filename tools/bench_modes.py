#!/usr/bin/env python
"""Dev tool (GPU box): the FNO at given Fourier mode counts -- the fused training step (FnoTrainEngine) and a whole-horizon rollout
(FnoRollout) -- with the per-kernel split of one step and each transform's share of its paper bound.

    python tools/bench_modes.py [--modes 16,16 24,24 32,33] [--hidden 20 32] [--batch 256] [--steps 20] [--warmup 5] [--grid 64,64]
                                [--rollout 16,16] [--rollout-hidden 32] [--rollout-batch 64] [--rollout-steps 200] [--rollout-grid 66,65]
                                [--json FILE]

--grid H,W (the step; also --height / --width) and --rollout-grid H,W reach the grids up to 128 x 128, e.g. the large-grid table of LABNOTES:
    python tools/bench_modes.py --grid 128,128 --batch 64 --modes 12,12 32,33 --rollout 12,12 --rollout-hidden 20 --rollout-grid 128,128

Prints one JSON line per measurement.  The paper bound of a transform launch is the larger of its FLOP at 155 TF (fp32 matrix / vector
pipe) and its algorithmic bytes at 8 TB/s, both as declared at the launch site (CFD_PROF_W: F = 4 H W m2 + 16 H m1 m2 per image and
direction; bytes = 4 H W + 16 m1 m2 forward, plus 4 H W per addend / aprev read on the inverse).
"""
from __future__ import annotations

import argparse
import ctypes
import gc
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cfdbench_amd import _lib  # noqa: E402
from cfdbench_amd.engine import FnoTrainEngine  # noqa: E402
from cfdbench_amd.models.fno.fno2d import Fno2d  # noqa: E402
from cfdbench_amd.models.loss import loss_name_to_fn  # noqa: E402
from cfdbench_amd.rollout import FnoRollout  # noqa: E402

PEAK_FLOPS, PEAK_BYTES = 155e12, 8e12
TRANSFORMS = ("k_dft_many", "k_dft_many_act", "k_idft_many", "k_idft_many_add", "k_idft_many_add_dgelu")


def modes_list(s):
    return [tuple(int(v) for v in m.split(",")) for m in s]


def read_prof(api):
    buf = ctypes.create_string_buffer(1 << 16)
    api.call("cfd_prof_end", buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        rows.append(dict(kernel=f[0], launches=int(f[1]), ms=float(f[2]), bytes=float(f[3]), flops=float(f[4])))
    return sorted(rows, key=lambda r: -r["ms"])


def timed(fn, steps, warmup):
    gc.collect()
    torch.cuda.synchronize()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def make_model(C, L, m1, m2, p, dev):
    torch.manual_seed(0)
    return Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, m1, m2, C).to(dev)


def step_leg(api, args, C, m1, m2, dev):
    B, H, W, p = args.batch, args.height, args.width, 5
    g = torch.Generator(device="cpu").manual_seed(1234)
    inputs = torch.randn(B, 2, H, W, generator=g).to(dev)
    label = (inputs.cpu() + 0.1 * torch.randn(B, 2, H, W, generator=g)).to(dev)
    cp = torch.randn(B, p, generator=g).to(dev)
    mask = torch.ones(B, 1, H, W, device=dev)
    eng = FnoTrainEngine(make_model(C, args.layers, m1, m2, p, dev), lr=1e-3, loss_name="nmse")
    step = lambda: eng.train_step(inputs, label, cp, mask)  # noqa: E731
    ms = timed(step, args.steps, args.warmup) * 1e3
    api.call("cfd_prof_begin")
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    rows = read_prof(api)
    tot = sum(r["ms"] for r in rows)
    kernels = []
    for r in rows:
        k = dict(kernel=r["kernel"], launches=r["launches"], us_per_step=round(r["ms"] / 3 * 1e3, 2), share=round(r["ms"] / tot, 4))
        if r["kernel"] in TRANSFORMS:
            bound_us = max(r["flops"] / PEAK_FLOPS, r["bytes"] / PEAK_BYTES) * 1e6 / r["launches"]
            k.update(us_per_launch=round(r["ms"] / r["launches"] * 1e3, 2), bound_us_per_launch=round(bound_us, 2),
                     bound_fraction=round(bound_us / (r["ms"] / r["launches"] * 1e3), 3))
        kernels.append(k)
    return dict(leg="fused_step", batch=B, hidden=C, layers=args.layers, grid=f"{H}x{W}", modes=[m1, m2], ms_per_step=round(ms, 4),
                kernels=kernels)


def rollout_leg(args, C, m1, m2, dev):
    B, (H, W), p, steps = args.rollout_batch, (int(v) for v in args.rollout_grid.split(",")), 5, args.rollout_steps
    g = torch.Generator(device="cpu").manual_seed(99)
    x0 = torch.randn(B, 2, H, W, generator=g).to(dev)
    cp = torch.randn(B, p, generator=g).to(dev)
    mask = torch.ones(B, 1, H, W, device=dev)
    mask[:, :, 0, :] = 0
    mask[:, :, -1, :] = 0
    mask[:, :, :, 0] = 0
    model = make_model(C, args.layers, m1, m2, p, dev).eval()
    ro = FnoRollout(model)
    ro.generate_frames(x0, cp, mask, steps)  # builds and captures the graph
    reps = 3
    dt = timed(lambda: ro.generate_frames(x0, cp, mask, steps), reps, 0)
    return dict(leg="rollout", cases=B, steps=steps, hidden=C, layers=args.layers, grid=f"{H}x{W}", modes=[m1, m2],
                ms_per_step=round(dt / steps * 1e3, 4), frames_per_s=round(B * steps / dt, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", nargs="*", default=["16,16", "24,24", "32,33"])
    ap.add_argument("--hidden", nargs="*", type=int, default=[20, 32])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--grid", default="", help="H,W of the step leg (overrides --height / --width)")
    ap.add_argument("--rollout-grid", default="66,65", help="H,W of the rollout leg")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollout", nargs="*", default=["16,16"])
    ap.add_argument("--rollout-hidden", type=int, default=32)
    ap.add_argument("--rollout-batch", type=int, default=64)
    ap.add_argument("--rollout-steps", type=int, default=200)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if args.grid:
        args.height, args.width = (int(v) for v in args.grid.split(","))
    api = _lib.api()
    dev = torch.device("cuda", 0)
    out = []
    for C in args.hidden:
        for m1, m2 in modes_list(args.modes):
            out.append(step_leg(api, args, C, m1, m2, dev))
            print(json.dumps(out[-1]), flush=True)
    for m1, m2 in modes_list(args.rollout):
        out.append(rollout_leg(args, args.rollout_hidden, m1, m2, dev))
        print(json.dumps(out[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
