#!/usr/bin/env python
"""Dev tool (GPU box): what a training objective costs the fused step (FnoTrainEngine(objective=); B = 256, 64 x 64, width 20, L = 4, one
GPU -- the headline step).  Writes profiles/objective_step.json and prints the table of LABNOTES "Objective step".

    python tools/bench_objective.py [--rounds 2] [--window 0.5] [--json profiles/objective_step.json]

1. Step time of five legs on the same build: `nmse` with the one-pass head (fused_head=True: the deferred step) and with the two-pass head
   (fused_head=False: what an objective's pass is built on), and the three objectives.  Child processes of this file, --rounds of them; a
   child times its legs alternately (device events around >= --window seconds of back-to-back steps after a warm-up), twice each.  Per leg:
   median and spread (min, max) over all windows of all rounds -- the spread of repeated runs is the margin a difference has to clear.
2. The three kernels' times against their byte counts: the library's own per-kernel profiler (cfd_prof_begin / cfd_prof_end: device events
   around every launch, with the bytes each CFD_PROF_W line declares) over a few steps of each objective, as microseconds per launch,
   GB/s and the share of 8 TB/s.  Events around a launch of a few microseconds include the events' own cost: the figure is an upper
   bound of the kernel's time.
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
from bench_clip import _setup, timed_window  # noqa: E402  (the headline step's engines, data and timer)

LEGS = {"nmse_one_pass_head": {}, "nmse_two_pass_head": dict(fused_head=False), "rel_l2": dict(objective="rel_l2"),
        "nmse_sample": dict(objective="nmse_sample"), "nmse_channel": dict(objective="nmse_channel")}
KERNELS = ("k_obj_part", "k_obj_final", "k_obj_bwd")
HBM_BYTES_PER_S = 8e12


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), windows_ms=[round(v, 4) for v in ms])


def kernel_rows(torch, eng, step, n=5):
    """The objective's three kernels over n steps of the library's profiler: per launch, microseconds and declared bytes."""
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
        name, count, ms, nbytes, _flops = line.split()
        total_us += float(ms) * 1e3 / n
        if name in KERNELS:
            us, per = float(ms) * 1e3 / int(count), float(nbytes) / int(count)
            rows[name] = dict(launches_per_step=int(count) / n, us_per_launch=round(us, 2), bytes_per_launch=int(per),
                              gb_per_s=round(per / (us * 1e-6) / 1e9, 1), share_of_8_tb_per_s=round(per / (us * 1e-6) / HBM_BYTES_PER_S, 3))
    return dict(kernels=rows, all_kernels_us_per_step=round(total_us, 1))


def child(window):
    torch, engine, stepper = _setup(REPO)
    engines = {n: engine(**kw) for n, kw in LEGS.items()}
    legs = {n: stepper(e) for n, e in engines.items()}
    ms = {n: [] for n in LEGS}
    for r in range(2):
        for n, fn in legs.items():
            ms[n].append(timed_window(torch, fn, 10 if r == 0 else 2, window) * 1e3)
    prof = {n: kernel_rows(torch, engines[n], legs[n]) for n, kw in LEGS.items() if "objective" in kw}
    print(json.dumps(dict(ms=ms, prof=prof)), flush=True)


def gpu_child(cmd, limit, what):
    """One child that uses the GPU, under its own time limit; a failure ends the tool: nothing more is started on the GPU."""
    r = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, env=dict(os.environ))
    if r.returncode != 0:
        sys.stderr.write(f"{what} failed (exit status {r.returncode}); nothing more is started on the GPU.\n{r.stderr[-2000:]}\n")
        raise SystemExit(2)
    return r


def markdown(out):
    lines = ["| leg | step, median (min .. max) ms | " + " | ".join(f"{k} us (GB/s)" for k in KERNELS) + " |", "|---|---|---|---|---|"]
    for leg, v in out["step_ms"].items():
        rows = out["kernels"].get(leg, {}).get("kernels", {})
        cells = [f"{rows[k]['us_per_launch']} ({rows[k]['gb_per_s']})" if k in rows else "-" for k in KERNELS]
        lines.append(f"| {leg} | {v['median_ms']:.4f} ({v['min_ms']:.4f} .. {v['max_ms']:.4f}) | " + " | ".join(cells) + " |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back steps per timed window (at least)")
    ap.add_argument("--json", default="profiles/objective_step.json")
    ap.add_argument("--child-limit", type=int, default=240, help="seconds a timing child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.window)
    me = [sys.executable, str(Path(__file__).resolve())]
    ms, prof = {n: [] for n in LEGS}, {}
    for _ in range(args.rounds):
        r = gpu_child([*me, "--child", "--window", str(args.window)], args.child_limit, "timing child")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        for leg, v in res["ms"].items():
            ms[leg] += v
        prof = res["prof"]  # (the last round's)
    out = dict(config=dict(batch=256, grid="64x64", hidden=20, layers=4, gpus=1, window_s=args.window, rounds=args.rounds,
                           windows_per_leg=2 * args.rounds, hbm_bytes_per_s=HBM_BYTES_PER_S,
                           note="kernel times: device events around each launch (the library's profiler), an upper bound for launches of a few us"),
               step_ms={leg: _summary(v) for leg, v in ms.items()}, kernels=prof)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(markdown(out), flush=True)


if __name__ == "__main__":
    main()
