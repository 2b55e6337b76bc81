#!/usr/bin/env python
"""Dev tool (GPU box): what an accumulated optimiser step of the fused FNO engine costs (FnoTrainEngine.accumulate / apply_accumulated;
B = 256 per micro-batch, 64 x 64, width 20, L = 4, one GPU).  Writes profiles/accum_step.json.

    python tools/bench_accum.py [--rounds 3] [--window 0.5] [--parent-root DIR] [--json profiles/accum_step.json]

1. One optimiser step over N = 1, 2, 4 micro-batches (N accumulates + one Adam), with and without clipping (a threshold that bites: half
   the first accumulated step's norm), against N plain train_steps of the same engine class in the same process; legs alternated --rounds
   times, device events around >= --window seconds of back-to-back groups after a warm-up; medians and spreads.
2. k_grad_accum alone: the accumulate call (cfd_fno_adam_step with CFD_STEP_ACCUMULATE) issued back to back on one finished pass -- the
   workspace keeps the pass's records, so every call redoes the same work -- with and without CFD_STEP_ACCUM_INIT; microseconds per call,
   launch to launch (a dispatch-bound figure for a 3.7 MB buffer, not an isolated kernel time).
3. --parent-root DIR (a checkout of the parent commit with its library built): N times the parent's train_step, measured in child processes
   alternated with this tree's, in this one call.  Without it: "not measured"."""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
B, N, C, L, P = 256, 64, 20, 4, 5
GROUPS = (1, 2, 4)


def _setup(root):
    sys.path.insert(0, str(root))
    import torch
    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_accum.py measures on the GPU: no device found")
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


def plain_group(eng, data, n):
    """n plain train_steps (what n micro-batches cost without accumulation: n Adams)."""
    k = [0]

    def group():
        for _ in range(n):
            inputs, label, cp, mask = data[k[0] % len(data)]
            k[0] += 1
            eng.train_step(inputs, label, cp, mask)
    return group


def accum_group(eng, data, n):
    k = [0]

    def group():
        for j in range(n):
            inputs, label, cp, mask = data[k[0] % len(data)]
            k[0] += 1
            eng.accumulate(inputs, label, cp, mask, weight=1.0 / n, first=j == 0)
        eng.apply_accumulated()
    return group


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


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), rounds_ms=[round(v, 4) for v in ms])


def kernel_alone(torch, eng, data, init):
    """Microseconds per accumulate call, issued back to back behind one finished pass."""
    from cfdbench_amd._capi import CFD_STEP_ACCUM_INIT, CFD_STEP_ACCUMULATE
    inputs, label, cp, mask = data[0]
    eng.accumulate(inputs, label, cp, mask, weight=0.5, first=True)
    flags = eng.defer_flags | CFD_STEP_ACCUMULATE | (CFD_STEP_ACCUM_INIT if init else 0)

    def call():
        eng._adam_step(eng.astruct, eng.gstruct, eng.accum, eng.flat.grad, False, 0.5, flags, inputs, cp, mask)
    us = timed_window(torch, call, 20, 0.05) * 1e6
    eng.apply_accumulated()
    return round(us, 3)


def child_plain(root, window):
    """--child ROOT: the plain train_step of the tree at ROOT (this one or the parent's), one window; prints the milliseconds."""
    torch, engine, data = _setup(root)
    print(json.dumps(dict(ms=timed_window(torch, plain_group(engine(), data, 1), 10, window) * 1e3)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back groups per timed leg and round (at least)")
    ap.add_argument("--json", default="profiles/accum_step.json")
    ap.add_argument("--parent-root", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child_plain(Path(args.child).resolve(), args.window)

    torch, engine, data = _setup(REPO)
    probe = engine(max_grad_norm=float("inf"))
    accum_group(probe, data, 2)()
    torch.cuda.synchronize()
    thr = 0.5 * float(probe.grad_norm())
    out = dict(config=dict(micro_batch=B, grid=f"{N}x{N}", hidden=C, layers=L, gpus=1, max_grad_norm_clipped=thr, window_s=args.window,
                           numel=int(probe.flat.numel)))
    out["k_grad_accum_back_to_back_us"] = dict(add=kernel_alone(torch, probe, data, False), init=kernel_alone(torch, probe, data, True))
    print(json.dumps(out["k_grad_accum_back_to_back_us"]), flush=True)
    del probe

    legs = {}
    for clip, kw in (("unclipped", {}), ("clipped", dict(max_grad_norm=thr))):
        plain, acc = engine(**kw), engine(**kw)
        for n in GROUPS:
            legs[f"{clip}:N{n}:plain_steps"] = plain_group(plain, data, n)
            legs[f"{clip}:N{n}:accumulated"] = accum_group(acc, data, n)
    t = {k: [] for k in legs}
    for r in range(args.rounds):  # alternate the legs
        for name, fn in legs.items():
            t[name].append(timed_window(torch, fn, 5 if r == 0 else 2, args.window) * 1e3)
    out["group_ms"] = {k: _summary(v) for k, v in t.items()}
    out["ratio_accumulated_to_plain"] = {
        f"{clip}:N{n}": round(out["group_ms"][f"{clip}:N{n}:accumulated"]["median_ms"] / out["group_ms"][f"{clip}:N{n}:plain_steps"]["median_ms"], 4)
        for clip in ("unclipped", "clipped") for n in GROUPS}
    print(json.dumps(out["group_ms"]), flush=True)
    print(json.dumps(out["ratio_accumulated_to_plain"]), flush=True)
    del legs
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
        parent = out["train_step_vs_parent"]["parent"]["median_ms"]
        out["accumulated_vs_n_parent_steps"] = {
            f"unclipped:N{n}": dict(accumulated_ms=out["group_ms"][f"unclipped:N{n}:accumulated"]["median_ms"], n_parent_steps_ms=round(n * parent, 4),
                                    ratio=round(out["group_ms"][f"unclipped:N{n}:accumulated"]["median_ms"] / (n * parent), 4)) for n in GROUPS}
    else:
        out["train_step_vs_parent"] = "not measured (no --parent-root)"
    print(json.dumps(out.get("accumulated_vs_n_parent_steps", out["train_step_vs_parent"])), flush=True)
    Path(args.json).parent.mkdir(parents=True, exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
