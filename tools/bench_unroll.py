#!/usr/bin/env python
"""Dev tool (GPU box): what an optimiser step on a K-step rollout window costs (B = 256, 64 x 64, width 20, L = 4, one GPU) at K = 1, 2, 4,
three ways in one session:

  (a) eager      cfdbench_amd.unroll.unrolled_loss -> backward -> torch.optim.Adam.step (tools/bench_ingrad.py's unrolled step)
  (b) window     FnoTrainEngine.train_window: the full gradient through the fed-back frames
  (c) detached   FnoTrainEngine.train_window(detach=True): K plain micro-batches along the model's own rollout

    python tools/bench_unroll.py [--rounds 3] [--window 1.0] [--json profiles/unroll_step.json]

The nine legs are alternated --rounds times; each timing is device events around >= --window seconds of back-to-back steps after a warm-up
(tools/bench_chan.py's timed_window); medians, and per leg the spread (max - min) / median of its rounds.  The expectation recorded with
the result: (b) is not slower than (a) at any K by more than (a)'s own run-to-run spread.  The per-kernel split (cfd_prof's device-event
pairs, three steps of their own after the timed windows) of (a) and (b) at K = 2 is written next to the times."""
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
from tools.bench_chan import timed_window  # noqa: E402
from tools.bench_ingrad import batches, kernel_split, make_model, unrolled_step  # noqa: E402

KS = (1, 2, 4)


def window_step(args, dev, K, detach):
    eng = FnoTrainEngine(make_model(args.hidden, args.layers, 5, dev), lr=1e-3, loss_name="nmse")
    data, k = batches(args.batch, args.grid, 5, K, dev), [0]

    def step():
        x, labels, cp, mask = data[k[0] % len(data)]
        k[0] += 1
        eng.train_window(x, labels, cp, mask, detach=detach)
    step.engine = eng
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--grid", type=int, default=64)
    ap.add_argument("--hidden", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back steps per timed leg and round (at least)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="profiles/unroll_step.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_unroll.py measures on the GPU: no device found")
    api, dev = _lib.api(), torch.device("cuda", 0)
    legs = {}
    for K in KS:
        legs[f"eager_K{K}"] = unrolled_step(args, dev, K)
        legs[f"window_K{K}"] = window_step(args, dev, K, False)
        legs[f"detached_K{K}"] = window_step(args, dev, K, True)
    times = {name: [] for name in legs}
    for r in range(args.rounds):  # alternate the legs
        for name, fn in legs.items():
            times[name].append(timed_window(fn, args.warmup if r == 0 else 2, args.window)[0] * 1e3)
    out = dict(config=dict(batch=args.batch, grid=f"{args.grid}x{args.grid}", hidden=args.hidden, layers=args.layers, gpus=1,
                           window_s=args.window, rounds=args.rounds), step_ms={})
    for name, ms in times.items():
        med = statistics.median(ms)
        out["step_ms"][name] = dict(median_ms=round(med, 4), rounds_ms=[round(v, 4) for v in ms], spread=round((max(ms) - min(ms)) / med, 4))
    out["window_vs_eager"] = {}
    for K in KS:
        a, b, c = (out["step_ms"][f"{leg}_K{K}"] for leg in ("eager", "window", "detached"))
        out["window_vs_eager"][f"K{K}"] = dict(
            window_to_eager=round(b["median_ms"] / a["median_ms"], 4), detached_to_eager=round(c["median_ms"] / a["median_ms"], 4),
            eager_spread=a["spread"], window_not_slower=bool(b["median_ms"] <= a["median_ms"] * (1.0 + a["spread"])))
    eng = legs["window_K2"].engine  # what a window holds per step: one training workspace and one prediction buffer (+ two dx buffers)
    out["config"]["bytes"] = dict(workspace_per_step=int(eng.ws.numel()), preds_per_step=int(eng.preds.numel() * 4),
                                  chained_gradient_buffers=2 * int(eng._win["dx"][0].numel() * 4), parameters=int(eng.flat.numel * 4))
    print(json.dumps(out["config"]), flush=True)
    print(json.dumps(out["step_ms"]), flush=True)
    print(json.dumps(out["window_vs_eager"]), flush=True)
    out["kernels_K2"] = {leg: kernel_split(api, legs[f"{leg}_K2"]) for leg in ("eager", "window")}
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
