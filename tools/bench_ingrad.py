#!/usr/bin/env python
"""Dev tool (GPU box): what the FNO's input gradients cost.  At B = 256, 64 x 64, width 20, L = 4 (the benchmark's model) it times
  * the eager autograd step model(**batch) -> loss["nmse"].backward() -> Adam.step() without and with inputs / case_params requiring a
    gradient -- the difference is k_ingrad plus what leaving the lifting layer's fused sums (stemg) costs: g_0 stored, k_chan_wgrad_stem
    and its reduction launched;
  * k_ingrad next to k_chan_wgrad_stem in the per-kernel split (cfd_prof) of the second leg: both read the same g_0;
  * the unrolled step (cfdbench_amd.unroll.unrolled_loss -> backward -> Adam.step) at K = 1, 2 and 4.

    python tools/bench_ingrad.py [--batch 256] [--hidden 20] [--window 1.0] [--rounds 3] [--json profiles/ingrad_step.json]

Timing: device events around a window of at least --window seconds of back-to-back steps after a warm-up (tools/bench_chan.py's
timed_window); each leg's figure is the median over the rounds, the legs alternate so that drift shows as spread.  Step inputs rotate over
8 batches and a B = 256 step streams about 1 GB of workspace in between, so no step finds its inputs in the 256 MB Infinity Cache."""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cfdbench_amd import _lib  # noqa: E402
from cfdbench_amd.models.fno.fno2d import Fno2d  # noqa: E402
from cfdbench_amd.models.loss import loss_name_to_fn  # noqa: E402
from cfdbench_amd.unroll import unrolled_loss  # noqa: E402
from tools.bench_chan import timed_window  # noqa: E402
from tools.bench_pad import read_prof  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3  # the streaming rate the project's copy-class kernels reach
KERNELS = ("k_ingrad", "k_ingrad_cp", "k_chan_wgrad_stem", "k_wgrad_reduce")


def make_model(C, L, p, dev):
    torch.manual_seed(0)
    return Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C).to(dev)


def batches(B, n, p, K, dev, slots=8):
    g = torch.Generator(device="cpu").manual_seed(1234)
    out = []
    for _ in range(slots):
        x = torch.randn(B, 2, n, n, generator=g)
        labels = [(x + 0.1 * (k + 1) * torch.randn(B, 2, n, n, generator=g)).to(dev) for k in range(K)]
        out.append((x.to(dev), labels, torch.randn(B, p, generator=g).to(dev), torch.ones(B, 1, n, n, device=dev)))
    return out


def autograd_step(args, dev, input_grads):
    model = make_model(args.hidden, args.layers, 5, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    data, k = batches(args.batch, args.grid, 5, 1, dev), [0]

    def step():
        x, labels, cp, mask = data[k[0] % len(data)]
        k[0] += 1
        if input_grads:
            x, cp = x.detach().requires_grad_(True), cp.detach().requires_grad_(True)
        opt.zero_grad()
        model(inputs=x, case_params=cp, mask=mask, label=labels[0])["loss"]["nmse"].backward()
        opt.step()
    return step


def unrolled_step(args, dev, K):
    model = make_model(args.hidden, args.layers, 5, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    data, k = batches(args.batch, args.grid, 5, K, dev), [0]

    def step():
        x, labels, cp, mask = data[k[0] % len(data)]
        k[0] += 1
        opt.zero_grad()
        unrolled_loss(model, x, labels, cp, mask)[0].backward()
        opt.step()
    return step


def kernel_split(api, step, reps=3):
    api.call("cfd_prof_begin")
    for _ in range(reps):
        step()
    torch.cuda.synchronize()
    out = []
    for r in read_prof(api):
        row = dict(kernel=r["kernel"], launches=r["launches"] // reps, us_per_step=round(r["ms"] / reps * 1e3, 2))
        if r["kernel"] in KERNELS and r["bytes"] > 0:
            tbs = r["bytes"] / (r["ms"] * 1e-3) / 1e12
            row.update(mb_per_launch=round(r["bytes"] / r["launches"] / 1e6, 2), tb_per_s=round(tbs, 3),
                       share_of_achievable_hbm=round(tbs / HBM_ACHIEVABLE_TBS, 3))
        out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back calls per timed leg and round (at least)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="profiles/ingrad_step.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_ingrad.py measures on the GPU: no device found")
    api, dev = _lib.api(), torch.device("cuda", 0)
    legs = {"autograd_step": autograd_step(args, dev, False), "autograd_step_input_grads": autograd_step(args, dev, True)}
    legs.update({f"unrolled_step_K{K}": unrolled_step(args, dev, K) for K in (1, 2, 4)})
    times = {k: [] for k in legs}
    for r in range(args.rounds):
        for name, fn in legs.items():
            times[name].append(timed_window(fn, args.warmup if r == 0 else 2, args.window)[0])
    out = []
    for name in legs:
        ms = [t * 1e3 for t in times[name]]
        row = dict(leg=name, grid=f"{args.grid}x{args.grid}", batch=args.batch, hidden=args.hidden, layers=args.layers,
                   ms_per_step=round(statistics.median(ms), 4), rounds_ms=[round(v, 4) for v in ms])
        if name.startswith("autograd_step"):
            row["kernels"] = kernel_split(api, legs[name])
        out.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
