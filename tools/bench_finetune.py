#!/usr/bin/env python
"""Dev tool (GPU box): what a fine-tuning step of the fused FNO engine costs (FnoTrainEngine with frozen parameters / optimizer="adamw";
B = 256, 64 x 64, width 20, L = 4, one GPU).  Writes profiles/finetune_step.json.

    python tools/bench_finetune.py [--rounds 3] [--window 0.5] [--parent-root DIR] [--json profiles/finetune_step.json]

1. ms per train_step of: every parameter trainable with Adam (the step of before this feature), the same with AdamW, and the trainable
   subsets head only (fc1, fc2), last block + head, fc0 + head -- each with Adam; legs alternated --rounds times in one process, device
   events around >= --window seconds of back-to-back steps after a warm-up; medians and spreads.
2. Launches per step of each leg, from the library's own per-kernel profiler over three steps (cfd_prof_begin / cfd_prof_end: the kernels
   the library launches, by name), with the microseconds per step of each kernel.
3. --parent-root DIR (a checkout of the parent commit with its library built): the all-trainable Adam step of the parent, measured in
   child processes alternated with this tree's, in this one call.  Without it: "not measured"."""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
B, N, C, L, P = 256, 64, 20, 4, 5
LEGS = {  # name -> FnoTrainEngine keywords
    "all_adam": {},
    "all_adamw": dict(optimizer="adamw", weight_decay=0.01),
    "head_only": dict(trainable=("fc1", "fc2")),
    "last_block_head": dict(trainable=(f"blocks.{L - 1}", "fc1", "fc2")),
    "fc0_head": dict(trainable=("fc0", "fc1", "fc2")),
}


def _setup(root):
    sys.path.insert(0, str(root))
    import torch
    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_finetune.py measures on the GPU: no device found")
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
    return torch, engine, data


def stepper(eng, data):
    k = [0]

    def step():
        inputs, label, cp, mask = data[k[0] % len(data)]
        k[0] += 1
        eng.train_step(inputs, label, cp, mask)
    return step


def timed_window(torch, fn, warmup, window_s):
    """Seconds per call from device events (tools/bench_accum.py's timed_window)."""
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


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), rounds_ms=[round(v, 4) for v in ms])


def launches(torch, eng, step, n=3):
    """Kernels per step launched by the library, over n steps behind a warm one."""
    step()
    torch.cuda.synchronize()
    eng.api.call("cfd_prof_begin")
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    buf = ctypes.create_string_buffer(1 << 16)
    eng.api.call("cfd_prof_end", buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        rows.append(dict(kernel=f[0], launches_per_step=int(f[1]) / n, us_per_step=round(float(f[2]) / n * 1e3, 2)))
    rows.sort(key=lambda r: -r["us_per_step"])
    return dict(launches_per_step=sum(r["launches_per_step"] for r in rows), kernels=rows)


def child_plain(root, window):
    """--child ROOT: the all-trainable Adam train_step of the tree at ROOT (this one or the parent's), one window; prints the milliseconds."""
    torch, engine, data = _setup(root)
    print(json.dumps(dict(ms=timed_window(torch, stepper(engine(), data), 10, window) * 1e3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back steps per timed leg and round (at least)")
    ap.add_argument("--json", default="profiles/finetune_step.json")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_plain(Path(args.child).resolve(), args.window)

    torch, engine, data = _setup(REPO)
    engines = {name: engine(**kw) for name, kw in LEGS.items()}
    legs = {name: stepper(eng, data) for name, eng in engines.items()}
    out = dict(config=dict(batch=B, grid=f"{N}x{N}", hidden=C, layers=L, gpus=1, window_s=args.window,
                           numel={name: int(eng.flat.numel) for name, eng in engines.items()},
                           last_backward_phase={name: int(eng.last_phase) for name, eng in engines.items()},
                           defer_flags={name: int(eng.defer_flags) for name, eng in engines.items()}))
    t = {k: [] for k in legs}
    for r in range(args.rounds):  # alternate the legs
        for name, fn in legs.items():
            t[name].append(timed_window(torch, fn, 5 if r == 0 else 2, args.window) * 1e3)
    out["step_ms"] = {k: _summary(v) for k, v in t.items()}
    base = out["step_ms"]["all_adam"]["median_ms"]
    out["ratio_to_all_adam"] = {k: round(v["median_ms"] / base, 4) for k, v in out["step_ms"].items()}
    print(json.dumps(out["step_ms"]), flush=True)
    print(json.dumps(out["ratio_to_all_adam"]), flush=True)
    out["launches"] = {name: launches(torch, engines[name], legs[name]) for name in legs}
    print(json.dumps({k: v["launches_per_step"] for k, v in out["launches"].items()}), flush=True)
    del legs, engines
    torch.cuda.synchronize()

    if args.parent_root:
        me = [sys.executable, str(Path(__file__).resolve())]
        roots, ms = {"this": REPO, "parent": Path(args.parent_root).resolve()}, {"this": [], "parent": []}
        for _ in range(args.rounds):  # alternate: this, parent, this, parent, ...
            for name, root in roots.items():
                r = subprocess.run([*me, "--child", str(root), "--window", str(args.window)], capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise RuntimeError(f"child for {name} failed ({r.returncode}): {r.stderr[-2000:]}")
                ms[name].append(json.loads(r.stdout.strip().splitlines()[-1])["ms"])
        out["train_step_vs_parent"] = {k: _summary(v) for k, v in ms.items()}
    else:
        out["train_step_vs_parent"] = "not measured (no --parent-root)"
    print(json.dumps(out["train_step_vs_parent"]), flush=True)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
