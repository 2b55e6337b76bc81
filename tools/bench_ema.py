#!/usr/bin/env python
"""Dev tool (GPU box): what the averaged weights cost the fused training step (FnoTrainEngine(ema_decay=d); B = 256, 64 x 64, width 20,
L = 4, nMSE, one GPU -- the headline step).  Writes profiles/ema_step.json and prints the table of LABNOTES "Averaged step".

    python tools/bench_ema.py --parent-root DIR [--rounds 3] [--window 0.5] [--no-trace] [--json profiles/ema_step.json]

1. Step time against the PARENT commit, in one session.  Child processes of this file, alternately one on this tree and one on DIR (a
   checkout of the parent commit with its library built), --rounds times each.  A child times its legs alternately (device events around
   >= --window seconds of back-to-back steps after a warm-up), twice each: the parent's `plain` step; this tree's `plain` and `ema`
   (ema_decay = 0.999).  Per leg: median and spread (min, max) over all windows of all rounds -- the spread of repeated runs is the margin
   a difference has to clear.
2. Launches per step and the optimiser kernel's time: one `rocprofv3 --kernel-trace --stats` run of this file's --trace-child mode (this
   tree's two legs one after the other).  From the dispatch list: launches per step of each leg (a step ends with its k_adam_f dispatch)
   and the mean time of k_adam_f per leg.  THE ONE HARD CONDITION: the launch counts of the two legs are equal; the tool exits with
   status 1 when they are not.  No bound on the times is fixed in advance: both numbers are written down.

Every child that uses the GPU runs under a time limit of its own (`timeout -k 10`), one after the other; the first one that fails ends
the tool -- nothing more is started on the GPU -- and what was measured until then is not written."""
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
from bench_clip import _setup, timed_window  # noqa: E402  (the headline step's engines, data and timer)

DECAY = 0.999
LEGS = {"plain": {}, "ema": dict(ema_decay=DECAY)}
N_ELEMENTS_NOTE = "8 more bytes per element of the flat buffer (one load, one store)"


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), windows_ms=[round(v, 4) for v in ms])


def child(root, names, window):
    """--child ROOT: the legs `names` of the tree at ROOT, alternated twice; prints {leg: [ms, ms]} and the flat buffer's size."""
    torch, engine, stepper = _setup(root)
    engines = {n: engine(**LEGS[n]) for n in names}
    legs = {n: stepper(e) for n, e in engines.items()}
    ms = {n: [] for n in names}
    for r in range(2):
        for n, fn in legs.items():
            ms[n].append(timed_window(torch, fn, 10 if r == 0 else 2, window) * 1e3)
    print(json.dumps(dict(ms=ms, numel=int(next(iter(engines.values())).flat.numel))), flush=True)


def trace_child(n_steps):
    torch, engine, stepper = _setup(REPO)
    for n in LEGS:
        step = stepper(engine(**LEGS[n]))
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
    if len(steps) != len(LEGS) * n_steps:
        raise RuntimeError(f"{len(steps)} optimiser launches in the trace, expected {len(LEGS) * n_steps}")
    out = {}
    for k, n in enumerate(LEGS):
        leg = steps[k * n_steps + 1:(k + 1) * n_steps]  # (a leg's first step carries the launches in front of it)
        mean_us = lambda key: round(statistics.mean([ns for s in leg for name, ns in s if name.startswith(key)] or [0]) / 1e3, 3)  # noqa: E731
        out[n] = dict(launches_per_step=sorted({len(s) for s in leg}), k_adam_f_us=mean_us("k_adam_f<"),
                      k_adam_f=sorted({name.split("(")[0] for s in leg for name, _ in s if name.startswith("k_adam_f<")}))
    return out


def gpu_child(cmd, limit, what):
    """One child that uses the GPU, under its own time limit; a failure ends the tool: nothing more is started on the GPU."""
    r = subprocess.run(["timeout", "-k", "10", str(limit), *cmd], capture_output=True, text=True, env=dict(os.environ))
    if r.returncode != 0:
        sys.stderr.write(f"{what} failed (exit status {r.returncode}); nothing more is started on the GPU.\n{r.stderr[-2000:]}\n")
        raise SystemExit(2)
    return r


def markdown(out):
    s, t = out["step_ms"], out.get("trace")
    lines = ["| leg | step, median (min .. max) ms | k_adam_f us | launches per step |", "|---|---|---|---|"]
    for root in ("parent", "this"):
        if not isinstance(s.get(root), dict):
            continue
        for leg, v in s[root].items():
            tr = t.get(leg) if (root == "this" and isinstance(t, dict)) else None
            lines.append(f"| {root}: {leg} | {v['median_ms']:.4f} ({v['min_ms']:.4f} .. {v['max_ms']:.4f}) | "
                         f"{tr['k_adam_f_us'] if tr else '-'} | {tr['launches_per_step'] if tr else '-'} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back steps per timed window (at least)")
    ap.add_argument("--json", default="profiles/ema_step.json")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-dir", default="profiles/ema_trace")
    ap.add_argument("--child-limit", type=int, default=180, help="seconds a timing child may take")
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
        roots["parent"] = (Path(args.parent_root).resolve(), ["plain"])
    ms = {name: {leg: [] for leg in legs} for name, (_, legs) in roots.items()}
    numel = None
    for _ in range(args.rounds):  # alternate: this, parent, this, parent, ...
        for name, (root, legs) in roots.items():
            r = gpu_child([*me, "--child", str(root), "--legs", *legs, "--window", str(args.window)], args.child_limit, f"timing child ({name})")
            res = json.loads(r.stdout.strip().splitlines()[-1])
            numel = res["numel"]
            for leg, v in res["ms"].items():
                ms[name][leg] += v
    out = dict(config=dict(batch=256, grid="64x64", hidden=20, layers=4, loss="nmse", gpus=1, window_s=args.window, rounds=args.rounds,
                           windows_per_leg=2 * args.rounds, ema_decay=DECAY, flat_elements=numel,
                           paper_extra_bytes=None if numel is None else 8 * numel, note=N_ELEMENTS_NOTE),
               step_ms={name: {leg: _summary(v) for leg, v in legs.items()} for name, legs in ms.items()})
    if "parent" not in roots:
        out["step_ms"]["parent"] = "not measured (no --parent-root)"
    print(json.dumps(out["step_ms"]), flush=True)

    equal = None
    if args.no_trace:
        out["trace"] = "not measured (--no-trace)"
    else:
        tdir = Path(args.trace_dir)
        tdir.mkdir(parents=True, exist_ok=True)
        gpu_child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(tdir), "-o", "ema", "--", *me, "--trace-child",
                   "--trace-steps", str(args.trace_steps)], 300, "rocprofv3 --kernel-trace")
        try:  # (a trace that cannot be read leaves the timings above in the file, and says so)
            out["trace"] = read_trace(tdir, args.trace_steps)
            equal = out["trace"]["plain"]["launches_per_step"] == out["trace"]["ema"]["launches_per_step"]
            out["launch_counts_equal"] = equal
        except Exception as e:  # noqa: BLE001
            out["trace"] = f"not measured: {e}"
    print(json.dumps(out["trace"]), flush=True)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(markdown(out), flush=True)
    if equal is False:
        sys.stderr.write("the step with the averaged weights launches another number of kernels than the step without\n")
        raise SystemExit(1)


if __name__ == "__main__":
    main()
