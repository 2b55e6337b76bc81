#!/usr/bin/env python
"""Dev tool (GPU box): what gradient-norm clipping costs the fused training step (FnoTrainEngine(max_grad_norm=); B = 256, 64 x 64, width 20,
L = 4, one GPU).  Writes profiles/clip_step.json.

    python tools/bench_clip.py [--rounds 5] [--window 1.0] [--parent-root DIR] [--no-trace] [--json profiles/clip_step.json]

1. Step time.  Three engines in one process -- no clipping, max_grad_norm = inf (the norm is measured, nothing clipped) and a threshold that
   bites (half the first step's norm) -- timed alternately (--rounds times, device events around >= --window seconds of back-to-back steps
   after a warm-up); median and spread per leg.
2. Launches and kernel times: one `rocprofv3 --kernel-trace --stats` run of this file's --trace-child mode (unclipped steps, then clipped
   ones).  From the dispatch list: launches per step of either leg (a step ends with its k_adam_f dispatch) -- the clipped step must have
   exactly one more -- and the mean times of k_gradsq and k_adam_f in the clipped steps: k_gradsq moves 4 of k_adam_f's 28 bytes per
   element and must not take longer.
3. --parent-root DIR (a checkout of the parent commit with its library built): the unclipped step of this tree and of DIR, each in child
   processes of its own, alternated --rounds times in this one call; both medians and spreads are recorded.  Without it: "not measured"."""
from __future__ import annotations

import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
B, N, C, L, P = 256, 64, 20, 4, 5


def _setup(root):
    sys.path.insert(0, str(root))
    import torch
    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_clip.py measures on the GPU: no device found")
    dev = torch.device("cuda", 0)

    def engine(**kw):
        torch.manual_seed(0)
        return FnoTrainEngine(Fno2d(2, 2, P, loss_name_to_fn("nmse"), L, 12, 12, C).to(dev), lr=1e-3, loss_name="nmse", **kw)

    g = torch.Generator(device="cpu").manual_seed(1234)
    data = []
    for _ in range(8):  # (rotating inputs; a B = 256 step streams ~1 GB of workspace in between: nothing stays in the Infinity Cache)
        x = torch.randn(B, 2, N, N, generator=g)
        data.append((x.to(dev), (x + 0.1 * torch.randn(B, 2, N, N, generator=g)).to(dev), torch.randn(B, P, generator=g).to(dev),
                     torch.ones(B, 1, N, N, device=dev)))

    def stepper(eng):
        k = [0]

        def step():
            inputs, label, cp, mask = data[k[0] % len(data)]
            k[0] += 1
            eng.train_step(inputs, label, cp, mask)
        return step
    return torch, engine, stepper


def timed_window(torch, fn, warmup, window_s):
    """Seconds per call from device events (tools/bench_chan.py's timed_window)."""
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(3):
        fn()
    b.record()
    torch.cuda.synchronize()
    n = max(3, int(window_s / max(a.elapsed_time(b) / 3e3, 1e-6)) + 1)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3 / n


def _first_norm(torch, engine, stepper):
    eng = engine(max_grad_norm=float("inf"))
    stepper(eng)()
    torch.cuda.synchronize()
    return float(eng.grad_norm())


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), rounds_ms=[round(v, 4) for v in ms])


def child_unclipped(root, window):
    """--child ROOT: the unclipped step of the tree at ROOT (this one or the parent's), one window; prints the milliseconds."""
    torch, engine, stepper = _setup(root)
    print(json.dumps(dict(ms=timed_window(torch, stepper(engine()), 10, window) * 1e3)), flush=True)


def trace_child(n_plain, n_clip):
    torch, engine, stepper = _setup(REPO)
    thr = 0.5 * _first_norm(torch, engine, stepper)
    plain, clipped = stepper(engine()), stepper(engine(max_grad_norm=thr))
    torch.cuda.synchronize()
    for _ in range(n_plain):
        plain()
    torch.cuda.synchronize()
    for _ in range(n_clip):
        clipped()
    torch.cuda.synchronize()


def read_trace(trace_dir, n_plain, n_clip):
    """Launches per step of both legs and the two kernels' mean times, from rocprofv3's dispatch list."""
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
    steps = steps[-(n_plain + n_clip):]  # (in front: the step that measured the threshold)
    if len(steps) != n_plain + n_clip:
        raise RuntimeError(f"{len(steps)} optimiser launches in the trace, expected {n_plain + n_clip}")
    plain, clipped = steps[1:n_plain], steps[n_plain + 1:]  # (each leg's first step carries the launches in front of it)
    count = lambda leg: sorted({len(s) for s in leg})  # noqa: E731
    mean_us = lambda leg, key: statistics.mean(ns for s in leg for name, ns in s if name.startswith(key)) / 1e3  # noqa: E731
    return dict(launches_per_step=dict(unclipped=count(plain), clipped=count(clipped)),
                k_gradsq_us=round(mean_us(clipped, "k_gradsq<"), 3), k_adam_f_clipped_us=round(mean_us(clipped, "k_adam_f<"), 3),
                k_adam_f_unclipped_us=round(mean_us(plain, "k_adam_f<"), 3),
                gradsq_launches=sum(1 for s in clipped for name, _ in s if name.startswith("k_gradsq<")), clipped_steps=len(clipped),
                trace_file=files[0].name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of back-to-back steps per timed leg and round (at least)")
    ap.add_argument("--json", default="profiles/clip_step.json")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default="profiles/clip_trace")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--trace-steps", type=int, nargs=2, default=(12, 16), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_unclipped(Path(args.child).resolve(), args.window)
    if args.trace_child:
        return trace_child(*args.trace_steps)

    torch, engine, stepper = _setup(REPO)
    thr = 0.5 * _first_norm(torch, engine, stepper)
    legs = {"unclipped": stepper(engine()), "measure_only_inf": stepper(engine(max_grad_norm=float("inf"))),
            "clipped": stepper(engine(max_grad_norm=thr))}
    t = {k: [] for k in legs}
    for r in range(args.rounds):  # alternate: unclipped, inf, clipped, unclipped, ...
        for name, fn in legs.items():
            t[name].append(timed_window(torch, fn, 10 if r == 0 else 2, args.window) * 1e3)
    out = dict(config=dict(batch=B, grid=f"{N}x{N}", hidden=C, layers=L, gpus=1, max_grad_norm_clipped=thr, window_s=args.window),
               step_ms={k: _summary(v) for k, v in t.items()})
    print(json.dumps(out["step_ms"]), flush=True)
    del legs
    torch.cuda.synchronize()

    me = [sys.executable, str(Path(__file__).resolve())]
    if args.parent_root:
        roots, ms = {"this": REPO, "parent": Path(args.parent_root).resolve()}, {"this": [], "parent": []}
        for _ in range(args.rounds):  # alternate: this, parent, this, parent, ...
            for name, root in roots.items():
                r = subprocess.run([*me, "--child", str(root), "--window", str(args.window)], capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError(f"child for {name} failed ({r.returncode}): {r.stderr[-2000:]}")
                ms[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        out["unclipped_vs_parent"] = {k: _summary(v) for k, v in ms.items()}
    else:
        out["unclipped_vs_parent"] = "not measured (no --parent-root)"
    print(json.dumps(out["unclipped_vs_parent"]), flush=True)

    if args.no_trace:
        out["trace"] = "not measured (--no-trace)"
    else:
        tdir = Path(args.trace_dir)
        tdir.mkdir(parents=True, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tdir), "-o", "clip", "--", *me, "--trace-child",
               "--trace-steps", *map(str, args.trace_steps)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ))
        try:  # (a trace that cannot be read leaves the timings above in the file, and says so)
            if r.returncode != 0:
                raise RuntimeError(f"rocprofv3 failed ({r.returncode}): {r.stderr[-2000:]}")
            out["trace"] = read_trace(tdir, *args.trace_steps)
        except Exception as e:  # noqa: BLE001
            out["trace"] = f"not measured: {e}"
    print(json.dumps(out["trace"]), flush=True)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
