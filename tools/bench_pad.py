#!/usr/bin/env python
"""Dev tool (GPU box): what domain padding costs.  Times the fused training step (FnoTrainEngine, B = 256, modes 12, width 20, L = 4) and
the rollout step of 64 cases (FnoRollout) of Fno2d(padding=8) at 64 x 64 against its yardstick, the UNPADDED model on a 72 x 72 grid: the
same transform grid and the same block work, a larger head and no copies (pad = 0 is the code path of every earlier build).  The unpadded
64 x 64 model is timed too, for scale.  The legs alternate (--rounds times) so that drift of the machine shows as spread instead of as a
difference; the per-kernel split of the padded step (cfd_prof) gives the three pad.hip kernels' times and achieved bandwidth.

    python tools/bench_pad.py [--batch 256] [--hidden 20] [--window 1.0] [--rounds 3] [--json profiles/pad_step.json]

Timing: device events around a window of at least --window seconds of back-to-back steps after a warm-up (tools/bench_chan.py's
timed_window); each leg's figure is the median over the rounds.  Step inputs rotate over 8 batches and a B = 256 step streams about 1 GB of
workspace in between, so no step finds its inputs in the 256 MB Infinity Cache."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cfdbench_amd import _lib  # noqa: E402
from cfdbench_amd.engine import FnoTrainEngine  # noqa: E402
from cfdbench_amd.models.fno.fno2d import Fno2d  # noqa: E402
from cfdbench_amd.models.loss import loss_name_to_fn  # noqa: E402
from cfdbench_amd.rollout import FnoRollout  # noqa: E402
from tools.bench_chan import timed_window  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3  # the streaming rate the project's copy-class kernels reach, not the 8 TB/s data-sheet peak
LEGS = [("pad8_64x64", 64, 8), ("plain_72x72", 72, 0), ("plain_64x64", 64, 0)]
PAD_KERNELS = ("k_stem_pad", "k_pad_crop", "k_pad_embed")


def read_prof(api):
    """cfd_prof_end's lines with the algorithmic bytes of each kernel (name count total_ms total_bytes total_flops)."""
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)
    api.call("cfd_prof_end", buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        rows.append(dict(kernel=f[0], launches=int(f[1]), ms=float(f[2]), bytes=float(f[3])))
    return sorted(rows, key=lambda r: -r["ms"])


def make_model(C, L, p, pad, dev):
    torch.manual_seed(0)
    return Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C, padding=pad or None).to(dev)


def batches(B, n, p, dev, slots=8):
    g = torch.Generator(device="cpu").manual_seed(1234)
    out = []
    for _ in range(slots):
        x = torch.randn(B, 2, n, n, generator=g)
        out.append((x.to(dev), (x + 0.1 * torch.randn(B, 2, n, n, generator=g)).to(dev), torch.randn(B, p, generator=g).to(dev),
                    torch.ones(B, 1, n, n, device=dev)))
    return out


def step_fn(args, n, pad, dev):
    eng = FnoTrainEngine(make_model(args.hidden, args.layers, 5, pad, dev), lr=1e-3, loss_name="nmse")
    data, k = batches(args.batch, n, 5, dev), [0]

    def step():
        inputs, label, cp, mask = data[k[0] % len(data)]
        k[0] += 1
        eng.train_step(inputs, label, cp, mask)
    return step


def rollout_fn(args, n, pad, dev):
    g = torch.Generator(device="cpu").manual_seed(99)
    x0 = torch.randn(args.rollout_batch, 2, n, n, generator=g).to(dev)
    cp = torch.randn(args.rollout_batch, 5, generator=g).to(dev)
    mask = torch.ones(args.rollout_batch, 1, n, n, device=dev)
    ro = FnoRollout(make_model(args.hidden, args.layers, 5, pad, dev).eval())
    return lambda: ro.generate_frames(x0, cp, mask, args.rollout_steps)


def kernel_split(api, step, reps=3):
    api.call("cfd_prof_begin")
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    out = []
    for r in read_prof(api):
        row = dict(kernel=r["kernel"], launches=r["launches"] // reps, us_per_step=round(r["ms"] / reps * 1e3, 2))
        if r["kernel"] in PAD_KERNELS:
            tbs = r["bytes"] / (r["ms"] * 1e-3) / 1e12
            row.update(mb_per_launch=round(r["bytes"] / r["launches"] / 1e6, 2), tb_per_s=round(tbs, 3),
                       share_of_achievable_hbm=round(tbs / HBM_ACHIEVABLE_TBS, 3))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hidden", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back calls per timed leg and round (at least)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rollout-batch", type=int, default=64)
    ap.add_argument("--rollout-steps", type=int, default=50)
    ap.add_argument("--json", default="profiles/pad_step.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_pad.py measures on the GPU: no device found")
    api, dev = _lib.api(), torch.device("cuda", 0)
    steps = {name: step_fn(args, n, pad, dev) for name, n, pad in LEGS}
    rolls = {name: rollout_fn(args, n, pad, dev) for name, n, pad in LEGS}
    t_step, t_roll = {k: [] for k in steps}, {k: [] for k in rolls}
    for r in range(args.rounds):  # alternate the legs: pad, 72, 64, pad, 72, 64, ...
        for name in steps:
            t_step[name].append(timed_window(steps[name], args.warmup if r == 0 else 2, args.window)[0])
        for name in rolls:
            t_roll[name].append(timed_window(rolls[name], 1, args.window)[0] / args.rollout_steps)
    out = []
    for name, n, pad in LEGS:
        ms = [t * 1e3 for t in t_step[name]]
        out.append(dict(leg="fused_step", model=name, grid=f"{n}x{n}", padding=pad, batch=args.batch, hidden=args.hidden, layers=args.layers,
                        ms_per_step=round(statistics.median(ms), 4), rounds_ms=[round(v, 4) for v in ms],
                        kernels=kernel_split(api, steps[name])))
        print(json.dumps(out[-1]), flush=True)
        ms = [t * 1e3 for t in t_roll[name]]
        out.append(dict(leg="rollout_step", model=name, grid=f"{n}x{n}", padding=pad, cases=args.rollout_batch, steps=args.rollout_steps,
                        hidden=args.hidden, layers=args.layers, ms_per_step=round(statistics.median(ms), 4), rounds_ms=[round(v, 4) for v in ms]))
        print(json.dumps(out[-1]), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
