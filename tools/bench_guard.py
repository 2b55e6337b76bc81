#!/usr/bin/env python
"""Dev tool (GPU box): what skipping non-finite steps on the device costs the fused training step (FnoTrainEngine(skip_nonfinite=True);
B = 256, 64 x 64, width 20, L = 4, nMSE, one GPU -- the headline step).  Writes profiles/guard_step.json.

    python tools/bench_guard.py --parent-root DIR [--rounds 3] [--window 0.5] [--no-trace] [--json profiles/guard_step.json]

1. Step time against the PARENT commit, in one session.  Child processes of this file, alternately one on this tree and one on DIR (a
   checkout of the parent commit with its library built), --rounds times each.  A child times its legs alternately (device events around
   >= --window seconds of back-to-back steps after a warm-up), twice each: the parent's `unclipped` and `clipped` steps; this tree's
   `unclipped`, `guard` (skip_nonfinite alone: the norm is measured, nothing clipped), `clipped` and `guard_clipped`.  The threshold is
   half the first step's norm, measured by the child.  Per leg: median and spread (min, max) over all windows of all rounds -- the spread
   of repeated runs is the margin a difference has to clear.
2. Launches per step and kernel times: one `rocprofv3 --kernel-trace --stats` run of this file's --trace-child mode (this tree's four
   legs one after the other).  From the dispatch list: launches per step of each leg (a step ends with its k_adam_f dispatch) -- the guard
   alone must cost the one launch clipping costs (k_gradsq), the guard with clipping none more than clipping -- and the mean times of
   k_gradsq and k_adam_f per leg."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO / "tools"))
from bench_clip import _first_norm, _setup, timed_window  # noqa: E402  (the headline step's engines, data and timer)

LEGS = {"unclipped": lambda thr: {}, "guard": lambda thr: dict(skip_nonfinite=True), "clipped": lambda thr: dict(max_grad_norm=thr),
        "guard_clipped": lambda thr: dict(max_grad_norm=thr, skip_nonfinite=True)}


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), windows_ms=[round(v, 4) for v in ms])


def child(root, names, window):
    """--child ROOT: the legs `names` of the tree at ROOT, alternated twice; prints {leg: [ms, ms]}."""
    torch, engine, stepper = _setup(root)
    thr = 0.5 * _first_norm(torch, engine, stepper)
    legs = {n: stepper(engine(**LEGS[n](thr))) for n in names}
    ms = {n: [] for n in names}
    for r in range(2):
        for n, fn in legs.items():
            ms[n].append(timed_window(torch, fn, 10 if r == 0 else 2, window) * 1e3)
    print(json.dumps(ms), flush=True)


def trace_child(n_steps):
    torch, engine, stepper = _setup(REPO)
    thr = 0.5 * _first_norm(torch, engine, stepper)
    for n in LEGS:
        step = stepper(engine(**LEGS[n](thr)))
        for _ in range(n_steps):
            step()
        torch.cuda.synchronize()


def read_trace(trace_dir, n_steps):
    import csv
    files = sorted(Path(trace_dir).rglob("*kernel_trace.csv"))
    if not files:
        raise RuntimeError(f"no kernel_trace.csv under {trace_dir}")
    rows = sorted(csv.DictReader(files[0].open()), key=lambda r: int(r["Start_Timestamp"]))
    steps, cur = [], []
    for r in rows:
        name = r["Kernel_Name"].replace("void ", "")
        cur.append((name, int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
        if name.startswith("k_adam_f<"):
            steps.append(cur)
            cur = []
    steps = steps[-len(LEGS) * n_steps:]  # (in front: the step that measured the threshold)
    if len(steps) != len(LEGS) * n_steps:
        raise RuntimeError(f"{len(steps)} optimiser launches in the trace, expected {len(LEGS) * n_steps}")
    out = {}
    for k, n in enumerate(LEGS):
        leg = steps[k * n_steps + 1:(k + 1) * n_steps]  # (a leg's first step carries the launches in front of it)
        mean_us = lambda key: round(statistics.mean([ns for s in leg for name, ns in s if name.startswith(key)] or [0]) / 1e3, 3)  # noqa: E731
        out[n] = dict(launches_per_step=sorted({len(s) for s in leg}), k_gradsq_us=mean_us("k_gradsq<"), k_adam_f_us=mean_us("k_adam_f<"),
                      k_adam_f=sorted({name.split("(")[0] for s in leg for name, _ in s if name.startswith("k_adam_f<")}))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back steps per timed window (at least)")
    ap.add_argument("--json", default="profiles/guard_step.json")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default="profiles/guard_trace")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--legs", nargs="+", default=list(LEGS), help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-steps", type=int, default=10, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(Path(args.child).resolve(), args.legs, args.window)
    if args.trace_child:
        return trace_child(args.trace_steps)

    me = [sys.executable, str(Path(__file__).resolve())]
    roots = {"this": (REPO, list(LEGS))}
    if args.parent_root:
        roots["parent"] = (Path(args.parent_root).resolve(), ["unclipped", "clipped"])
    ms = {name: {leg: [] for leg in legs} for name, (_, legs) in roots.items()}
    for _ in range(args.rounds):  # alternate: this, parent, this, parent, ...
        for name, (root, legs) in roots.items():
            r = subprocess.run([*me, "--child", str(root), "--legs", *legs, "--window", str(args.window)], capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"child for {name} failed ({r.returncode}): {r.stderr[-2000:]}")
            for leg, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                ms[name][leg] += v
    out = dict(config=dict(batch=256, grid="64x64", hidden=20, layers=4, loss="nmse", gpus=1, window_s=args.window, rounds=args.rounds,
                           windows_per_leg=2 * args.rounds),
               step_ms={name: {leg: _summary(v) for leg, v in legs.items()} for name, legs in ms.items()})
    if "parent" not in roots:
        out["step_ms"]["parent"] = "not measured (no --parent-root)"
    print(json.dumps(out["step_ms"]), flush=True)

    if args.no_trace:
        out["trace"] = "not measured (--no-trace)"
    else:
        tdir = Path(args.trace_dir)
        tdir.mkdir(parents=True, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tdir), "-o", "guard", "--", *me, "--trace-child",
               "--trace-steps", str(args.trace_steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ))
        try:  # (a trace that cannot be read leaves the timings above in the file, and says so)
            if r.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({r.returncode}): {r.stderr[-2000:]}")
            out["trace"] = read_trace(tdir, args.trace_steps)
        except Exception as e:  # noqa: BLE001
            out["trace"] = f"not measured: {e}"
    print(json.dumps(out["trace"]), flush=True)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
