#!/usr/bin/env python
"""Dev tool (GPU box): what the Sobolev objective costs the fused step (FnoTrainEngine(objective="hs"); B = 256, width 20, L = 4, one
GPU), at 64 x 64 and at 66 x 65.  Writes profiles/sobolev_step.json and prints the table of LABNOTES "Sobolev objective".

    python tools/bench_sobolev.py [--rounds 2] [--window 0.5] [--json profiles/sobolev_step.json]

1. Step time of five legs on the same build: `nmse` with the two-pass head (what an objective's pass is built on), `rel_l2`, and `hs` with
   k = 1, k = 2 and k = 2 grouped.  Child processes of this file, one per grid and round; a child times its legs alternately (device
   events around >= --window seconds of back-to-back steps after a warm-up), twice each.  Per leg: median and spread (min, max) over all
   windows of all rounds -- the spread of repeated runs is the margin a difference has to clear.
2. The Sobolev kernels against their declared counts: the library's own per-kernel profiler (cfd_prof_begin / cfd_prof_end: device events
   around every launch, with the bytes and flops each CFD_PROF_W line declares), as microseconds per launch, the share of the fp32
   matrix peak (157.3 TFLOP/s) and of 8 TB/s.
No threshold is fixed in advance: the numbers are written down.

Every child that uses the GPU runs under a time limit of its own (`timeout -k 10`), one after the other; the first one that fails ends
the tool -- nothing more is started on the GPU -- and what was measured until then is not written."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
from bench_clip import timed_window  # noqa: E402  (the headline step's timer)

B, C, L, P = 256, 20, 4, 5
GRIDS = ("64x64", "66x65")
LEGS = {"nmse_two_pass_head": dict(fused_head=False), "rel_l2": dict(objective="rel_l2"), "hs_k1": dict(objective="hs", hs_k=1),
        "hs_k2": dict(objective="hs", hs_k=2), "hs_k2_grouped": dict(objective="hs", hs_k=2, hs_group=True)}
KERNELS = ("k_hs_fwd", "k_hs_final", "k_hs_bwd")
HBM_BYTES_PER_S, MFMA_FP32_FLOPS = 8e12, 157.3e12


def _setup(H, W):
    sys.path.insert(0, str(REPO))
    import torch
    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_sobolev.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)

    def engine(**kw):
        torch.manual_seed(0)
        return FnoTrainEngine(Fno2d(2, 2, P, loss_name_to_fn("nmse"), L, 12, 12, C).to(dev), lr=1e-3, loss_name="nmse", **kw)

    g = torch.Generator(device="cpu").manual_seed(1234)
    data = []
    for _ in range(8):  # (rotating inputs, as tools/bench_clip.py: nothing stays in the Infinity Cache)
        x = torch.randn(B, 2, H, W, generator=g)
        data.append((x.to(dev), (x + 0.1 * torch.randn(B, 2, H, W, generator=g)).to(dev), torch.randn(B, P, generator=g).to(dev),
                     torch.ones(B, 1, H, W, device=dev)))

    def stepper(eng):
        k = [0]

        def step():
            inputs, label, cp, mask = data[k[0] % len(data)]
            k[0] += 1
            eng.train_step(inputs, label, cp, mask)
        return step
    return torch, engine, stepper


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), windows_ms=[round(v, 4) for v in ms])


def kernel_rows(torch, eng, step, n=5):
    """The Sobolev kernels over n steps of the library's profiler: per launch, microseconds, declared bytes and flops."""
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    eng.api.call("cfd_prof_begin")
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    eng.api.call("cfd_prof_end", buf, len(buf))
    rows, total_us = {}, 0.0
    for line in buf.value.decode().splitlines():
        name, count, ms, nbytes, flops = line.split()
        total_us += float(ms) * 1e3 / n
        if name in KERNELS:
            us, per, fl = float(ms) * 1e3 / int(count), float(nbytes) / int(count), float(flops) / int(count)
            rows[name] = dict(launches_per_step=int(count) / n, us_per_launch=round(us, 2), bytes_per_launch=int(per), flops_per_launch=int(fl),
                              share_of_fp32_mfma_peak=round(fl / (us * 1e-6) / MFMA_FP32_FLOPS, 4),
                              share_of_8_tb_per_s=round(per / (us * 1e-6) / HBM_BYTES_PER_S, 4))
    return dict(kernels=rows, all_kernels_us_per_step=round(total_us, 1))


def child(window, grid):
    H, W = (int(v) for v in grid.split("x"))
    torch, engine, stepper = _setup(H, W)
    engines = {n: engine(**kw) for n, kw in LEGS.items()}
    legs = {n: stepper(e) for n, e in engines.items()}
    ms = {n: [] for n in LEGS}
    for r in range(2):
        for n, fn in legs.items():
            ms[n].append(timed_window(torch, fn, 10 if r == 0 else 2, window) * 1e3)
    prof = {n: kernel_rows(torch, engines[n], legs[n]) for n, kw in LEGS.items() if kw.get("objective") == "hs"}
    print(json.dumps(dict(ms=ms, prof=prof)), flush=True)


def gpu_child(cmd, limit, what):
    """One child that uses the GPU, under its own time limit; a failure ends the tool: nothing more is started on the GPU."""
    r = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, env=dict(os.environ))
    if r.returncode != 0:
        sys.stderr.write(f"{what} failed (exit status {r.returncode}); nothing more is started on the GPU.\n{r.stderr[-2000:]}\n")
        raise SystemExit(2)
    return r


def markdown(out):
    lines = ["| grid | leg | step, median (min .. max) ms | " + " | ".join(f"{k} us (MFMA peak, HBM)" for k in KERNELS) + " |", "|---|---|---|---|---|---|"]
    for grid, g in out["grids"].items():
        for leg, v in g["step_ms"].items():
            rows = g["kernels"].get(leg, {}).get("kernels", {})
            cells = [f"{rows[k]['us_per_launch']} ({rows[k]['share_of_fp32_mfma_peak']:.1%}, {rows[k]['share_of_8_tb_per_s']:.1%})" if k in rows else "-"
                     for k in KERNELS]
            lines.append(f"| {grid} | {leg} | {v['median_ms']:.4f} ({v['min_ms']:.4f} .. {v['max_ms']:.4f}) | " + " | ".join(cells) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back steps per timed window (at least)")
    ap.add_argument("--json", default="profiles/sobolev_step.json")
    ap.add_argument("--child-limit", type=int, default=240, help="seconds a timing child may take")
    ap.add_argument("--child", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.window, args.child)
    me = [sys.executable, str(Path(__file__).resolve())]
    grids = {}
    for grid in GRIDS:
        ms, prof = {n: [] for n in LEGS}, {}
        for _ in range(args.rounds):
            r = gpu_child([*me, "--child", grid, "--window", str(args.window)], args.child_limit, f"timing child {grid}")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            for leg, v in res["ms"].items():
                ms[leg] += v
            prof = res["prof"]  # (the last round's)
        grids[grid] = dict(step_ms={leg: _summary(v) for leg, v in ms.items()}, kernels=prof)
    out = dict(config=dict(batch=B, hidden=C, layers=L, gpus=1, window_s=args.window, rounds=args.rounds, windows_per_leg=2 * args.rounds,
                           hbm_bytes_per_s=HBM_BYTES_PER_S, mfma_fp32_flops=MFMA_FP32_FLOPS,
                           note="kernel times: device events around each launch (the library's profiler), an upper bound for launches of a few us"),
               grids=grids)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(markdown(out), flush=True)


if __name__ == "__main__":
    main()
