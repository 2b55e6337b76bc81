#!/usr/bin/env python
"""Headline benchmark: Auto-FNO training frames/s on synthetic (B,2,64,64) batches (BASELINE.json metric).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus N --steps K --warmup W          # starts its own N ranks (one process per GPU, RCCL over xGMI)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W             # or under an external launcher: WORLD_SIZE set => this process is a rank

A step = forward + nMSE loss + backward + (N>1: RCCL all-reduce of the flat gradient) + Adam on one batch that is
already resident in HBM.  Workload = BASELINE.json configs[1]: Fno2d(in=2,out=2,p=5,L=4,hidden=20,modes=12), B=256 per
GPU, 64x64, fp32.  Weak scaling: every rank processes its own B frames; value = N*B*K / max-over-ranks time.
Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints the contract's keys with `config`,
`final_nmse` and
  roofline_step             the whole step against the ideal-fusion byte count of SURVEY 8d (10.2 MB/frame at C=20, L=4)
  --dump-outputs DIR        after the timed steps, rank 0 writes what the last timed step computed as DIR/<name>.npy (float32):
                            preds, loss_sums (the tensor train_step returns), params / grads (the flat buffers after Adam, in
                            abi_parameters order), adam_exp_avg / adam_exp_avg_sq.  At most 64 MB in all: an array over its share
                            keeps a fixed, seeded sample of its leading-axis rows.  The inputs are seeded, so runs compare file by file.
With --full (off by default) the line also carries
  roofline                  dominant kernel of the step: ALGORITHMIC bytes per launch / HIP-event time vs 8 TB/s
  roofline_spectral_conv2d  the north-star kernel group (SpectralConv2d fwd+bwd, 5N + 3Wb bytes)
  kernels                   every kernel of the step: launches, average time, HBM fraction
  split2                    the same step and SpectralConv2d group with two-piece activation operands (cfd_tune_set("act_pieces", 2): rounds 1-4's default)
  fp32_mfma_route           the same with the transforms on the exact-fp32 MFMA kernels (cfd_tune_set("exact_fp32", 1))
  rollout / rollout_66x65   batched multi-step inference from one HIP graph (configs[4] horizon: 200 steps)
  train_66x65 / train_batch8 / train_c32_*  the same train step on the 66x65 grid (dam / tube / cylinder), at the reference's default batch 8 and default width 32
  unet_cfg2 / auto_deeponet_cfg3 / resnet_b32   train steps of BASELINE configs[2] / configs[3] and of the ResNet baseline on one GPU
  cpu_baseline              the reference's ATen call sequence on the host cores, at B = 256 and B = 32
  dp                        (N > 1) the same K steps with the gradient exchange switched off: the exposed part of the all-reduces
The rollout / rollout_66x65 legs run on EVERY rank (cases shard over the ranks, `n_gpus` inside the leg); the other extra legs
run on rank 0 at N = 1 only.  The --no-* options leave single legs out of a --full run.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
from pathlib import Path

import torch
import torch.distributed as dist

REPO = Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP32_PEAK_TF = 157.3        # MI355X_MICROARCH.md: fp32 vector == f32-input MFMA peak
BF16_MFMA_PEAK_TF = 2500.0  # dense bf16 MFMA peak
# kernels whose GEMM-shaped work runs as split-bf16 products on the bf16 matrix pipe (cfd_common.h): on the default route (three pieces
# per operand since round 5) an fp32-equivalent flop costs SIX bf16 MFMA flops, like the convolutions below
SPLIT_BF16 = ("k_dft_fwd", "k_idft", "k_block", "k_chan_wgrad", "k_head")
# the k = 3 / k = 7 convolutions (conv6.hip): three-piece operands, SIX bf16 MFMAs per fp32-exact product
SPLIT6_BF16 = ("k_conv_fwd", "k_conv_dgrad", "k_conv_wgrad")
# profiler label (cfd_prof, what `roofline.kernel` and the `kernels` table name) -> the symbol rocprofv3's kernel trace shows for it
ROCPROF_SYMBOL = {"k_head_train": "k_head_bwd<5, true, true, true, float, 3, 4> (head.hip: the FUSE instantiation = forward + loss + backward in one pass)",
                  "k_head_bwd": "k_head_bwd<..., false, ...>", "k_block_bwd_dgelu": "k_block<8, 3, 3, false, true, true, true, 3, false, false>",
                  "k_block_fwd_act": "k_block<10, 2, 2, true, false, false, false, 3, false, false>",
                  "k_block_fwd": "k_block<10, 2, 2, false, false, false, false, 3, false, false>",
                  "k_block_bwd_stem": "k_block<8, 3, 3, false, true, false, true, 3, false, true>",
                  "k_mix": "k_modes_mfma<20, false, false, 2, 32>", "k_mixadj_wgrad": "k_modes_mfma<20, true, true, 3, 40>", "k_adam": "k_adam_f<true>",
                  "k_dft_fwd": "k_dft_fwd64_b3<3, false, 3>", "k_dft_fwd_act": "k_dft_fwd64_b3<3, true, 3>"}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle", type=int, default=30,
                    help="untimed steps BEFORE the W warm-up steps (part of set-up, like building the model): the first ~25 steps after a cold "
                         "start run 2-4 %% slower (clock ramp, first touch of the 1.3-GB workspace); the timed region is still exactly K steps "
                         "after W warm-up steps, bracketed by barriers")
    ap.add_argument("--batch", type=int, default=256, help="frames per GPU per step (BASELINE configs[1]: 256)")
    ap.add_argument("--hidden", type=int, default=20)
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--height", type=int, default=64)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--n-case-params", type=int, default=5)
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: the per-kernel roofline, rollout, extra-size / precision / route "
                         "legs, the other model families, the CPU baseline and (N > 1) the exchange-off timing (module docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed to DIR/<name>.npy (module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-steps", type=int, default=10, help="timed steps of the cpu_baseline leg (SURVEY 8d: >= 10 after 3 warm-up steps)")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--graph", action="store_true", help="replay forward+backward from a HIP graph")
    ap.add_argument("--no-rollout", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the U-Net / Auto-DeepONet / exact-fp32 legs")
    ap.add_argument("--rollout-batch", type=int, default=64)
    ap.add_argument("--rollout-steps", type=int, default=200)
    ap.add_argument("--only", default=None,
                    help="run ONE extra leg and print {leg: result} (what the rocprofv3 --pmc passes of tools/pmc_traffic.sh profile): "
                         "spectral | unet | auto_deeponet | resnet | deeponet | auto_edeeponet | auto_ffn | auto_deeponet_cnn")
    ap.add_argument("--backend", default="nccl", choices=("nccl", "gloo"),
                    help="torch.distributed backend of the N > 1 job: nccl = RCCL over xGMI (the product); gloo only with --dry-dp")
    ap.add_argument("--dry-dp", action="store_true",
                    help="no GPU: run ONLY the data-parallel skeleton of the step (rank launch, rendezvous, GradSync's per-phase "
                         "exchange of the model's flat gradient buffer, barrier / max-over-ranks timing, the JSON line) on host "
                         "tensors -- what tests/test_cpu_host.py drives; the line is marked dry_dp and is not a measurement")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.dump_outputs and (args.only or args.dry_dp):
        ap.error("--dump-outputs writes the headline step's outputs: not with --only or --dry-dp")
    return args


# ----------------------------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` starts its own N ranks (one process per GPU)
# ----------------------------------------------------------------------------------------------------------------------
def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(n):
    """Called when --gpus N > 1 and no rendezvous environment is set (i.e. not under torch.distributed.run): start the N ranks
    of this same command line ourselves -- RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / a free MASTER_PORT, exactly
    what torchrun would export -- inherit stdout (rank 0 prints the one JSON line), and return the worst exit code.  If a rank
    dies the others are terminated by PID (they would otherwise sit in the rendezvous or a collective until its timeout)."""
    import subprocess
    port = free_port()
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_SELF_LAUNCHED="1")
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: what RCCL needs on these hosts
        env.setdefault("OMP_NUM_THREADS", "8")
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), *sys.argv[1:]], env=env))
    rc, live = 0, list(procs)
    while live:
        for pr in list(live):
            code = pr.poll()
            if code is None:
                continue
            live.remove(pr)
            if code != 0 and rc == 0:
                rc = code
                for other in live:  # exact PIDs of our own children
                    other.terminate()
        time.sleep(0.05)
    return rc


# ----------------------------------------------------------------------------------------------------------------------
# rooflines
# ----------------------------------------------------------------------------------------------------------------------
def read_prof(api):
    """cfd_prof_end -> [(name, launches, total_ms, algorithmic_bytes, flops)], slowest first."""
    buf = ctypes.create_string_buffer(1 << 16)
    api.call("cfd_prof_end", buf, len(buf))
    rows = []
    for line in buf.value.decode().splitlines():
        f = line.split()
        rows.append((f[0], int(f[1]), float(f[2]), float(f[3]), float(f[4])))
    rows.sort(key=lambda r: -r[2])
    return rows


def roofline_of(name, launches, total_ms, total_bytes, total_flops):
    """the FNO / U-Net / DeepONet kernels are priced against HBM (algorithmic bytes of the launches, declared at
    the launch sites, / their HIP-event time); a kernel whose matrix work would take LONGER than its bytes at the peak of the
    pipe it issues on is priced against that pipe instead."""
    if total_ms <= 0 or launches <= 0:
        return None
    t = total_ms * 1e-3
    split, split6 = name.startswith(SPLIT_BF16), name.startswith(SPLIT6_BF16)
    pipe_tf = BF16_MFMA_PEAK_TF / 6.0 if (split or split6) else FP32_PEAK_TF  # fp32-equivalent flops/s of the pipe
    pipe = "bf16 MFMA, six products of three-piece (fp32-exact) operands (fp32-equivalent flops)" if (split or split6) else "fp32 MFMA / VALU"
    t_hbm = total_bytes / (HBM_PEAK_GBS * 1e9)
    t_pipe = total_flops / (pipe_tf * 1e12)
    out = dict(kernel=name, avg_us=round(total_ms / launches * 1e3, 2), launches=launches,
               algorithmic_bytes_per_launch=int(total_bytes / launches))
    if total_bytes <= 0 and total_flops <= 0:
        return dict(out, bound=None, frac=None, note="partial-sum reduction / data movement: no algorithmic bytes of its own")
    if t_pipe > t_hbm:
        tfs = total_flops / t / 1e12
        return dict(out, bound="mfma", achieved=round(tfs, 2), peak=round(pipe_tf, 1), unit="TFLOP/s", frac=round(tfs / pipe_tf, 4),
                    traffic=None, pipe=pipe)
    gbs = total_bytes / t / 1e9
    return dict(out, bound="hbm", achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(gbs / HBM_PEAK_GBS, 4), traffic=None,
                fp32_equiv_tflops=round(total_flops / t / 1e12, 2))


def latest_profile(suffix):
    """Newest profiles/r<round><letters>_<suffix> (e.g. suffix "pmc_traffic.json" = the step's counters, "unet_pmc_traffic.json" = a
    leg's): the round tag is matched exactly, so a leg's file never passes for another leg's or for the step's."""
    import re
    pat = re.compile(r"^r\d+[a-z]*_" + re.escape(suffix) + "$")
    files = sorted(f for f in (REPO / "profiles").iterdir() if pat.match(f.name))
    return (json.loads(files[-1].read_text()), files[-1]) if files else (None, None)


def profile_avg_us(tag, name):
    """Average duration of kernel ``name`` in the rocprofv3 --stats summary committed with the same profile tag, or None."""
    import csv
    f = REPO / "profiles" / f"{tag}_step_kernel_stats.csv"
    if not f.exists():
        return None
    tot, calls = 0.0, 0
    for r in csv.DictReader(f.open()):
        k = r["Name"].replace("void ", "")
        if k.startswith(name + "<") or k.startswith(name + "("):
            tot += float(r["TotalDurationNs"])
            calls += int(r["Calls"])
    return tot / calls / 1e3 if calls else None


def attach_pmc(rl, name, applies):
    """HBM traffic per launch and unit-busy percentages of the dominant kernel from the committed rocprofv3 PMC passes of this
    same command (tools/profile_step.sh, tools/pmc_step.sh: FETCH_SIZE doubled per MI355X_MICROARCH.md + WRITE_SIZE).  The
    counters are NOT measured in this run: the line names the profile they come from, and they are dropped (null + reason) when
    the kernel's time in this run is more than 15 % away from its time in that profile -- i.e. when the kernel has changed."""
    if not (rl and applies):
        return
    try:
        sym = {"k_head_train": "k_head_bwd"}.get(name, name)  # profiler label -> kernel symbol (the fused head is k_head_bwd<.., FUSE>)
        pmc, pf = latest_profile("pmc_traffic.json")
        if not pmc:
            return
        tag = pf.name.split("_pmc_traffic")[0]
        ref_us = profile_avg_us(tag, sym)
        rl["pmc_profile"] = dict(file=f"profiles/{pf.name}", kernel_avg_us_in_profile=None if ref_us is None else round(ref_us, 2))
        if ref_us is None or abs(rl["avg_us"] - ref_us) > 0.15 * ref_us:
            rl["traffic"] = None
            rl["pmc_profile"]["dropped"] = ("kernel time in this run deviates > 15 % from the profiled build (or the profile has no row for it): "
                                            "counters of another build are not attached")
            return
        match = [v for k, v in pmc.items() if k.startswith(sym + "<") or k == sym]
        if match:
            rl["traffic"] = int(sum(m["traffic_bytes"] for m in match) / len(match))
            rl["traffic_source"] = f"profiles/{pf.name} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same command, per launch)"
        busy, bf = latest_profile("step_busy.json")
        match = [v for k, v in (busy or {}).items() if k.startswith(sym + "<") or k == sym]
        if match and bf.name.startswith(tag):
            rl["busy_pct"] = {k: match[0][k] for k in ("mfma", "valu", "lds", "wait") if k in match[0]}
            rl["busy_source"] = f"profiles/{bf.name} (rocprofv3 --pmc SQ_* busy counters of the same step)"
    except Exception:  # noqa: BLE001
        pass


def attach_leg_traffic(rl, leg, kernel=None):
    """Counter-based HBM traffic of a leg's roofline object from the committed rocprofv3 --pmc passes of `bench.py --only LEG`
    (tools/pmc_traffic.sh -> profiles/r*_LEG_pmc_traffic.json; FETCH_SIZE doubled per MI355X_MICROARCH.md, + WRITE_SIZE).
    kernel = None: the whole leg is one kernel GROUP (SpectralConv2d forward+backward): bytes of all launches of the profiled
    command / its number of group calls.  Not measured in this run -- the line names the file."""
    if not rl:
        return
    pmc, pf = latest_profile(f"{leg}_pmc_traffic.json")
    if not pmc:
        return
    try:
        if kernel is None:
            # one adjoint-mix + weight-gradient launch per group call (round 6: k_modes_mfma<C, CONJT = true, WGRAD = true, ..>)
            calls = sum(v["launches"] for k, v in pmc.items() if isinstance(v, dict) and
                        (k.startswith("k_mixadj_wgrad") or (k.startswith("k_modes_mfma<") and ", true, true," in k)))
            if calls:
                rl["traffic"] = int(sum(v["traffic_bytes"] * v["launches"] for k, v in pmc.items() if isinstance(v, dict) and k.startswith("k_")) / calls)
        else:
            # profiler label -> (symbol prefix, required template-argument substring)
            sym, need = {"k_head_train": ("k_head_bwd", ""), "k_conv_dgrad": ("k_conv6", ", true, "), "k_conv_fwd": ("k_conv6", ", false, "),
                         "k_conv_wgrad": ("k_conv6_wgrad", "")}.get(kernel, (kernel, ""))
            match = [v for k, v in pmc.items() if isinstance(v, dict) and (k == sym or k.startswith(sym + "<")) and need in k]
            n = sum(m["launches"] for m in match)
            if n:
                rl["traffic"] = int(sum(m["traffic_bytes"] * m["launches"] for m in match) / n)
        if rl.get("traffic"):
            rl["traffic_source"] = f"profiles/{pf.name} (rocprofv3 --pmc FETCH_SIZE x 2 + WRITE_SIZE passes of `bench.py --only {leg}`, per launch)"
    except Exception:  # noqa: BLE001
        pass


def fno_step_bytes_per_frame(C, L, HW, training=True):
    """SURVEY.md 8(d) ideal fusion: every activation crosses HBM once per layer boundary, the 128-wide head never exists.
    forward = inputs (3 ch) + [label (2)] + stem write A + L (read A + write A) + head read A + preds (2); backward ~ 2x."""
    A = C * HW * 4
    fwd = (2 * L + 2) * A + (3 + 2 + (2 if training else 0)) * HW * 4
    return 3 * fwd if training else fwd


# ----------------------------------------------------------------------------------------------------------------------
# legs
# ----------------------------------------------------------------------------------------------------------------------
def settle():
    """Between legs: collect the previous leg's engines / graphs NOW (their destruction -- hipGraphExecDestroy, pool frees -- is
    host-synchronous and otherwise lands inside the next leg's timed loop: 3-ms outliers were observed) and drain the device."""
    import gc
    gc.collect()
    torch.cuda.synchronize()


def time_steps(fn, steps, warmup):
    settle()
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def profiled(api, fn, steps):
    api.call("cfd_prof_begin")
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return read_prof(api)


def spectral_leg(api, _lib, dev, B, C, H, W, reps):
    """North-star kernel group: SpectralConv2d forward+backward alone, algorithmic bytes 5N + 3Wb."""
    plan = _lib.plan(H, W, 12, 12, dev.index)
    x = torch.randn(B, C, H, W, device=dev)
    gy = torch.randn(B, C, H, W, device=dev)
    w1 = torch.view_as_real(torch.rand(C, C, 12, 12, dtype=torch.cfloat, device=dev) / (C * C)).contiguous()
    w2 = torch.view_as_real(torch.rand(C, C, 12, 12, dtype=torch.cfloat, device=dev) / (C * C)).contiguous()
    y, gx = torch.empty_like(x), torch.empty_like(x)
    gw1, gw2 = torch.empty_like(w1), torch.empty_like(w2)
    xh = torch.empty(B, C, 24, 12, 2, device=dev)
    z = torch.empty(B, C, 24, 12, 2, device=dev)
    ws = torch.empty(api.size("cfd_spectral_conv2d_bwd_workspace_bytes", plan, B, C, C), dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def spec():
        api.call("cfd_spectral_conv2d_fwd", plan, x.data_ptr(), w1.data_ptr(), w2.data_ptr(), y.data_ptr(), xh.data_ptr(),
                 z.data_ptr(), B, C, C, st)
        api.call("cfd_spectral_conv2d_bwd", plan, gy.data_ptr(), xh.data_ptr(), w1.data_ptr(), w2.data_ptr(), gx.data_ptr(),
                 gw1.data_ptr(), gw2.data_ptr(), ws.data_ptr(), B, C, C, st)

    settle()
    for _ in range(3):
        spec()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        spec()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / reps * 1e3
    alg = 5 * B * C * H * W * 4 + 3 * 2 * C * C * 144 * 8
    gbs = alg / (us * 1e-6) / 1e9
    return dict(what=f"SpectralConv2d fwd+bwd, B={B}, C={C}, {H}x{W}, modes 12 (dft, mix, idft | dft, adjoint mix + weight gradient, idft)",
                bound="hbm", algorithmic_bytes=alg, avg_us=round(us, 2), achieved=round(gbs, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                frac=round(gbs / HBM_PEAK_GBS, 4), traffic=None)


def rollout_leg(model, B, steps, H, W, p, dev, reps=3, dtype="f32", seed=99):
    from cfdbench_amd.rollout import FnoRollout
    g = torch.Generator(device="cpu").manual_seed(seed)
    x0 = torch.randn(B, 2, H, W, generator=g).to(dev)
    cp = torch.randn(B, p, generator=g).to(dev)
    mask = torch.ones(B, 1, H, W, device=dev)
    if (H, W) != (64, 64):  # tube / dam style border
        mask[:, :, 0, :] = 0
        mask[:, :, -1, :] = 0
        mask[:, :, :, 0] = 0
    kw = {} if dtype == "f32" else dict(dtype=dtype)
    ro = FnoRollout(model, **kw)
    ro.generate_frames(x0, cp, mask, steps)  # builds + captures the graph
    settle()
    t0 = time.perf_counter()
    for _ in range(reps):
        fr = ro.generate_frames(x0, cp, mask, steps)  # the graph's own frame buffer: no copies in the timed region
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    cfg = model.abi_config()
    bpf = fno_step_bytes_per_frame(cfg["hidden"], cfg["num_layers"], H * W, training=False)
    if dtype != "f32":
        A = cfg["hidden"] * H * W * 4
        bpf -= (2 * cfg["num_layers"] + 2) * A // 2  # activations stored in 2 bytes
    fps = B * steps / dt
    out = dict(what=f"FnoRollout: {B} cases x {steps} steps, Fno2d(hidden {cfg['hidden']}, L {cfg['num_layers']}), {H}x{W}, "
                    f"{'fp32' if dtype == 'f32' else 'bf16 activation storage, fp32 accumulate'}, one HIP graph per horizon",
               frames_per_s=round(fps, 1), ms_per_step=round(dt / steps * 1e3, 4),
               roofline=dict(bound="hbm", bytes_per_frame=bpf, achieved=round(fps * bpf / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                             frac=round(fps * bpf / 1e9 / HBM_PEAK_GBS, 4)))
    if dtype == "f32":
        with torch.no_grad():
            plain = model.generate_many(x0, cp, mask, 3)
        out["bitwise_equal_to_generate_many"] = bool(all(torch.equal(a, b) for a, b in zip(plain, fr[1:4])))
    return out, fr


def unet_bytes_per_frame(dim, cin, H, W):
    """Ideal fusion for the U-Net (conv + BatchNorm + ReLU as one pass, pooling / concat by addressing): every conv reads its
    input and writes its output once in the forward pass; backward ~ 2x (unet.py:11-108)."""
    e = 0
    chans = [dim * 2 ** i for i in range(5)]
    e += (cin + chans[0]) * H * W + 2 * chans[0] * H * W  # in_conv
    for i in range(1, 5):
        hw = (H >> i) * (W >> i)
        e += (chans[i - 1] + chans[i]) * hw + 2 * chans[i] * hw
    for i in range(4, 0, -1):
        hw_lo, hw = (H >> i) * (W >> i), (H >> (i - 1)) * (W >> (i - 1))
        e += chans[i] * hw_lo + chans[i - 1] * hw  # transposed conv
        e += (chans[i] + chans[i - 1]) * hw + 2 * chans[i - 1] * hw  # double conv on the concatenation
    e += (chans[0] + 2) * H * W
    return 3 * e * 4


DP = dict(world=1, rank=0, steps=None, warmup=None, force=False, comm_stream_overlaps=None)  # set by main() for `--gpus N --only LEG`: the leg as a data-parallel job


def model_dp_leg(name, model, batch, frames, what):
    """`bench.py --gpus N --only unet|auto_deeponet|...`: the train step of a graph-replayed model as a DATA-PARALLEL job, one process
    per GPU (BASELINE configs[2] "DDP 8x", configs[3] "4x"): forward + backward + gradient pack from one HIP graph, ONE all-reduce of
    the flat gradient over RCCL, Adam from a second graph (cfdbench_amd/graph.py).  Weak scaling: every rank trains on its own batch;
    value = N * B * K / max-over-ranks time between barriers -- the contract of the headline line."""
    from cfdbench_amd.graph import GraphedTrainStep
    from cfdbench_amd.optim import Adam as MultiTensorAdam
    world, rank = DP["world"], DP["rank"]
    steps, warmup = DP["steps"] or 20, DP["warmup"] if DP["warmup"] is not None else 5
    opt = MultiTensorAdam(model.parameters(), lr=1e-3)
    gs = GraphedTrainStep(model, opt, batch)
    assert gs.dp == (world > 1 or DP["force"])
    for _ in range(warmup):
        gs(**gs.static)  # (the batch in the step's own buffers: DeviceBatchLoader.bind)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        gs(**gs.static)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=batch["inputs"].device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    return {"metric": f"train frames/sec, {name}", "value": round(world * frames * steps / elapsed, 1), "unit": "frames/s", "n_gpus": world,
            "steps": steps, "warmup": warmup, "ms_per_step": round(elapsed / steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": what, "global_batch": world * frames, "parallelism": f"dp{world}",
                       "step": "ONE HIP graph per step: forward + backward + gradient pack -> all-reduce of the flat gradient (RCCL, captured) -> Adam "
                               "(CFDBENCH_DP_ONE_GRAPH=0: graph A -> eager all-reduce -> graph B, the round-5 form)",
                       "flat_gradient_bytes": int(gs.exchange.numel * 4) if gs.exchange is not None else 0,
                       "collective_in_graph": bool(gs.one_graph), "comm_stream_overlaps": DP["comm_stream_overlaps"]},
            "final_nmse": round(float(gs.loss["nmse"].item()), 6)}


def model_train_leg(api, name, model, batch, steps, warmup, frames, bytes_per_frame, what):
    if DP["world"] > 1 or DP["force"]:
        return model_dp_leg(name, model, batch, frames, what)
    from cfdbench_amd.optim import Adam as MultiTensorAdam
    opt = MultiTensorAdam(model.parameters(), lr=1e-3)  # torch.optim.Adam's update as one launch per 80 tensors (cfd_adam_multi)
    from cfdbench_amd.graph import GraphedTrainStep

    def eager():
        out = model(**batch)
        out["loss"]["nmse"].backward()
        opt.step()
        # set_to_none: the next backward pass hands autograd's gradient tensors over as they are (with set_to_none=False every step paid
        # one fill and one accumulate-add launch per parameter -- 46 + 56 stock ATen launches per U-Net step in round 4's rocprof table)
        opt.zero_grad(set_to_none=True)

    dt_eager = time_steps(eager, steps, warmup)
    rows = profiled(api, eager, steps)
    res = dict(what=what, frames_per_s=round(frames / dt_eager, 1), ms_per_step=round(dt_eager * 1e3, 3), mode="eager")
    try:
        if getattr(model, "graph_unsafe", False):  # per-step HOST state a replayed graph would freeze (no model of this tree since the ResNet's
            raise RuntimeError("model is graph_unsafe: eager launches only")  # dropout step counter moved to the device, round 4)
        gs = GraphedTrainStep(model, opt, batch)
        # the batch sits in the step's own buffers, as the resident loader leaves it (harness/data.py: DeviceBatchLoader.bind gathers every
        # batch straight into GraphedTrainStep.static) -- handing over OTHER tensors costs four device-to-device copies per step
        dt_graph = time_steps(lambda: gs(**gs.static), steps, warmup)
        if dt_graph < dt_eager:
            res.update(frames_per_s=round(frames / dt_graph, 1), ms_per_step=round(dt_graph * 1e3, 3), mode="one HIP graph per step",
                       eager_ms_per_step=round(dt_eager * 1e3, 3))
    except Exception as e:  # noqa: BLE001
        res["graph_error"] = str(e)[:200]
    fps = res["frames_per_s"]
    if bytes_per_frame:
        res["roofline_step"] = dict(bound="hbm", bytes_per_frame=int(bytes_per_frame), achieved=round(fps * bytes_per_frame / 1e9, 1),
                                    peak=HBM_PEAK_GBS, unit="GB/s", frac=round(fps * bytes_per_frame / 1e9 / HBM_PEAK_GBS, 4))
    tot = sum(r[2] for r in rows)
    res["kernels"] = [dict(kernel=r[0], launches_per_step=r[1] // steps, us_per_step=round(r[2] / steps * 1e3, 1), share=round(r[2] / tot, 3))
                      for r in rows[:8]]
    dom = next((r for r in rows if r[3] > 0 or r[4] > 0), rows[0])
    res["roofline"] = roofline_of(*dom)
    attach_leg_traffic(res["roofline"], name, dom[0])
    return res


# ----------------------------------------------------------------------------------------------------------------------
# train-step legs of the other model families (rank 0, N = 1); each also runs alone under `--only NAME`
# ----------------------------------------------------------------------------------------------------------------------
def _fields(B, H, W, p, gen, dev, border=False):
    if DP["rank"]:  # data-parallel leg: every rank draws its own shard
        gen.manual_seed(gen.initial_seed() + 1000 * DP["rank"])
    x = torch.randn(B, 2, H, W, generator=gen).to(dev)
    mask = torch.ones(B, 1, H, W, device=dev)
    if border:
        mask[:, :, 0, :] = 0
        mask[:, :, -1, :] = 0
        mask[:, :, :, 0] = 0
    return dict(inputs=x, label=(x.cpu() + 0.1 * torch.randn(B, 2, H, W, generator=gen)).to(dev),
                case_params=torch.randn(B, p, generator=gen).to(dev), mask=mask)


def leg_unet(api, dev):
    from cfdbench_amd.models.loss import loss_name_to_fn
    from cfdbench_amd.models.unet import UNet
    Bu, pu = 128, 8
    torch.manual_seed(0)
    unet = UNet(2, 2, loss_name_to_fn("nmse"), pu, insert_case_params_at="input", dim=12).to(dev)
    bu = _fields(Bu, 64, 64, pu, torch.Generator(device="cpu").manual_seed(7), dev)
    return model_train_leg(api, "unet", unet, bu, 10, 3, Bu, unet_bytes_per_frame(12, 2 + 1 + pu, 64, 64),
                           "BASELINE configs[2] per GPU: U-Net(dim 12, p=8) train step (fwd+nMSE+bwd+Adam), batch 128, 64x64, fp32")


def ffn_stack_bytes(rows, widths):
    """Ideal fusion of a Linear(+activation) stack over `rows` rows (ffn.py:12-35): the input rows are read once, the output rows
    written once and every weight matrix read once in the forward pass; backward ~ 2x (the same streams + their gradients)."""
    w = sum(a * b + b for a, b in zip(widths[:-1], widths[1:]))
    return 3 * 4 * (rows * (widths[0] + widths[-1]) + w)


def leg_auto_deeponet(api, dev):
    from cfdbench_amd.models.auto_deeponet import AutoDeepONet
    from cfdbench_amd.models.loss import loss_name_to_fn
    Bd, Hd, Wd, w, d = 512, 66, 65, 100, 8
    torch.manual_seed(0)
    don = AutoDeepONet(Hd * Wd + 5, 2, loss_name_to_fn("nmse"), branch_depth=d, trunk_depth=d, width=w, act_name="relu").to(dev)
    bd = _fields(Bd, Hd, Wd, 5, torch.Generator(device="cpu").manual_seed(8), dev)
    # SURVEY 8(a-8) ideal fusion: the branch stack over B rows of H*W+p inputs, the trunk stack over the k = H*W query points, and the
    # inner product reading both (B + k) x w outputs, the residual u and the label and writing the (B, k) predictions -- never (B, k, w)
    k = Hd * Wd
    step_bytes = ffn_stack_bytes(Bd, [k + 5] + [w] * d) + ffn_stack_bytes(k, [2] + [w] * d) + 3 * 4 * ((Bd + k) * w + 3 * Bd * k)
    return model_train_leg(api, "auto_deeponet", don, bd, 10, 3, Bd, step_bytes / Bd,
                           "BASELINE configs[3] per GPU: Auto-DeepONet(width 100, depth 8/8) train step, batch 512, 66x65, fp32")


def leg_resnet(api, dev):
    # ResNet (SURVEY a-7: the one MFMA-bound path, 4.37 GFLOP per frame forward); training mode = dropout active
    from cfdbench_amd.models.loss import loss_name_to_fn
    from cfdbench_amd.models.resnet import ResNet
    Br = 32
    torch.manual_seed(0)
    rn = ResNet(2, 2, 5, loss_name_to_fn("nmse"), hidden_chan=16, num_blocks=4, kernel_size=7, padding=3).to(dev)
    br = _fields(Br, 64, 64, 5, torch.Generator(device="cpu").manual_seed(9), dev)
    leg = model_train_leg(api, "resnet", rn, br, 5, 2, Br, None,
                          "ResNet(hidden 16, depth 4, 7x7) train step (src/models/resnet.py:145-198), batch 32, 64x64, fp32")
    fl = 3 * 4.37e9 * Br
    tf = fl / (leg["ms_per_step"] * 1e-3) / 1e12
    pk = round(BF16_MFMA_PEAK_TF / 6.0, 1)
    leg["roofline_step"] = dict(bound="mfma", flops_per_step=fl, achieved=round(tf, 2), peak=pk, unit="TFLOP/s", frac=round(tf / pk, 4),
                                pipe="bf16 MFMA at six products per fp32-exact product (conv6.hip: three-piece operands): 2.5 PF / 6")
    return leg


def leg_deeponet(api, dev):
    """the NON-autoregressive DeepONet of train.py (src/models/deeponet.py:153-223): branch over the case parameters,
    trunk over (t, x, y) for k = 1000 random lattice points per step, NormAct activations."""
    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.train import init_model
    B, H, W, k = 256, 64, 64, 1000
    torch.manual_seed(0)
    m = init_model(Args(model="deeponet", data_name="cavity_prop_bc_geo", loss_name="nmse")).to(dev)
    g = torch.Generator(device="cpu").manual_seed(10)
    batch = dict(case_params=torch.randn(B, 5, generator=g).to(dev), t=torch.rand(B, 1, generator=g).to(dev),
                 label=torch.randn(B, 3, H, W, generator=g).to(dev),
                 query_idxs=torch.stack([torch.randint(0, H, (k,), generator=g), torch.randint(0, W, (k,), generator=g)], -1).to(dev))
    w, d = 100, 8
    # ideal fusion: the trunk stack runs over B*k rows whose FIRST layer input is built in-kernel from (b, p) + (k, p) rows; only the
    # (B, k) predictions / sampled labels and the parameters cross HBM
    step_bytes = 3 * 4 * (2 * B * k + (B + k) * w) + ffn_stack_bytes(0, [w] * (d + 1)) + ffn_stack_bytes(B, [5] + [w] * d)
    leg = model_train_leg(api, "deeponet", m, batch, 10, 3, B, None,
                          f"DeepONet (non-autoregressive, train.py) train step: batch {B} x {k} query points, width 100, depth 8/8, NormAct, fp32")
    # the trunk stack over B*k rows dominates (2 * rows * w * w per w x w layer, forward + 2x backward); its GEMMs are exact fp32 MFMA
    fl = 3 * 2.0 * B * k * (d - 1) * w * w
    tf = fl / (leg["ms_per_step"] * 1e-3) / 1e12
    leg["roofline_step"] = dict(bound="mfma", flops_per_step=fl, achieved=round(tf, 2), peak=FP32_PEAK_TF, unit="TFLOP/s", frac=round(tf / FP32_PEAK_TF, 4),
                                pipe="fp32 MFMA (exact-fp32 GEMMs: ReLU / NormAct kinks, DESIGN.md section 4)",
                                ideal_fusion_bytes_per_step=int(step_bytes))
    return leg


def _auto_leg(api, dev, name, B, what, **flags):
    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.autoregressive import init_model
    torch.manual_seed(0)
    m = init_model(Args(model=name, data_name="cavity_prop_bc_geo", loss_name="nmse", **flags)).to(dev)
    batch = _fields(B, 64, 64, 5, torch.Generator(device="cpu").manual_seed(11), dev)
    return model_train_leg(api, name, m, batch, 10, 3, B, None, what)


def leg_auto_edeeponet(api, dev):
    return _auto_leg(api, dev, "auto_edeeponet", 128, "SURVEY 8f-3: Auto-EDeepONet (two branches x trunk, width 100, depth 8) train step, batch 128, 64x64, fp32")


def leg_auto_ffn(api, dev):
    return _auto_leg(api, dev, "auto_ffn", 32, "SURVEY 8f-3: Auto-FFN (width 200, depth 8; first Linear split over [frame | query]) train step, batch 32, 64x64, fp32")


def leg_auto_deeponet_cnn(api, dev):
    return _auto_leg(api, dev, "auto_deeponet_cnn", 32, "SURVEY 8f-3: Auto-DeepONet-CNN (5x5 conv branch, 512-wide output FFN) train step, batch 32, 64x64, fp32")


# leg name -> (key in the JSON line, function)
MODEL_LEGS = {
    "unet": ("unet_cfg2", leg_unet), "auto_deeponet": ("auto_deeponet_cfg3", leg_auto_deeponet), "resnet": ("resnet_b32", leg_resnet),
    "deeponet": ("deeponet_nonauto", leg_deeponet), "auto_edeeponet": ("auto_edeeponet", leg_auto_edeeponet),
    "auto_ffn": ("auto_ffn", leg_auto_ffn), "auto_deeponet_cnn": ("auto_deeponet_cnn", leg_auto_deeponet_cnn),
}


def dry_dp(args, rank, world):
    """--dry-dp: the step's data-parallel skeleton on host tensors (module docstring of parse()).  The flat gradient buffer has
    the layout of the benchmark's Fno2d (engine.flatten_layout / backward_phase_slices), every rank fills it with its own
    values, and each 'step' runs GradSync's per-phase asynchronous exchange in backward-phase order followed by the 1/world
    scale -- the same calls FnoTrainEngine.forward_backward_overlapped makes between its kernels."""
    from cfdbench_amd.engine import GradSync, backward_phase_slices, flatten_layout
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(args.backend if args.backend == "gloo" or torch.cuda.is_available() else "gloo", rank=rank, world_size=world)
    B, C, L, p = args.batch, args.hidden, args.layers, args.n_case_params
    torch.manual_seed(0)
    model = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C)
    offs, numel = flatten_layout(model.abi_parameters())
    slices = backward_phase_slices(offs, numel, L)
    sync = GradSync(None)
    g = torch.Generator().manual_seed(1234 + rank)
    mine = torch.randn(numel, generator=g)
    flat = torch.empty_like(mine)

    def step():
        flat.copy_(mine)
        scale = sync.wait_all([sync.reduce_slice_async(flat, a, b) for a, b in slices])
        flat.mul_(scale)

    def barrier():
        if world > 1:
            dist.barrier()

    for _ in range(args.warmup):
        step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    # every rank must now hold the mean of all ranks' buffers: checked against an all-gather of the originals
    ok = True
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        parts = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(parts, mine)
        ok = bool(torch.allclose(flat, torch.stack(parts).sum(0) / world, rtol=1e-6, atol=1e-7))
    elapsed = float(t.item())
    if rank == 0:
        print(json.dumps({
            "metric": "train frames/sec (64x64x2), Auto-FNO cavity", "value": None, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic", "dry_dp": True,
            "config": {"workload": "DRY RUN of the data-parallel skeleton (no kernels, no GPU): launcher + rendezvous + per-phase gradient "
                                   "exchange of the Fno2d flat gradient buffer on host tensors; not a measurement",
                       "global_batch": world * B, "parallelism": f"dp{world}", "backend": dist.get_backend() if world > 1 else None,
                       "flat_gradient_floats": numel, "exchange_slices": len(slices), "self_launched": os.environ.get("CFDBENCH_SELF_LAUNCHED") == "1"},
            "gradient_mean_ok": ok}), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if not ok:
        sys.exit(4)


DUMP_BYTES = 64 << 20


def dump_outputs(out_dir, tensors):
    """--dump-outputs: {name: tensor} -> out_dir/<name>.npy as float32, smallest first, each within an equal share of what is left of
    DUMP_BYTES.  An array over its share keeps a seeded sample of its leading-axis rows (of its elements where one row is already too
    large), so the same shape always keeps the same rows."""
    import numpy as np
    out = Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    arrays = sorted(((k, t.detach().float().cpu().numpy()) for k, t in tensors.items()), key=lambda kv: kv[1].nbytes)
    left = DUMP_BYTES
    for i, (name, a) in enumerate(arrays):
        share = left // (len(arrays) - i)
        if a.nbytes > share:
            if a.ndim > 1 and a.nbytes // a.shape[0] > share:
                a = a.reshape(-1)
            k = max(1, share // (a.nbytes // a.shape[0]))
            a = a[np.sort(np.random.default_rng(0).choice(a.shape[0], k, replace=False))]
        np.save(out / f"{name}.npy", np.ascontiguousarray(a))
        left -= a.nbytes


def main():
    args = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args.gpus))  # plain `python bench.py --gpus N`: one process per GPU, started here
    if world != args.gpus and rank == 0:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}: running the {world} ranks the launcher started", file=sys.stderr)
    if args.dry_dp:
        return dry_dp(args, rank, world)
    if args.backend != "nccl":
        print("bench.py: --backend gloo is for --dry-dp only; the measured job exchanges gradients over RCCL", file=sys.stderr)
        sys.exit(1)
    if not torch.cuda.is_available():
        print("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU fallback", file=sys.stderr)
        sys.exit(1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # CFDBENCH_DP_ALWAYS_EXCHANGE=1 with --only LEG on ONE GPU: the leg's data-parallel form over a one-rank RCCL group whose collectives
    # are forced on (engine.GradSync) -- how a 1-GPU box exercises that code path (tests/test_gpu_dp.py); not a measurement of scaling
    force_dp = world == 1 and args.only in MODEL_LEGS and os.environ.get("CFDBENCH_DP_ALWAYS_EXCHANGE", "0") == "1"
    if world > 1 or force_dp:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if force_dp:
            os.environ.setdefault("MASTER_PORT", str(free_port()))
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        # the communicator's stream must not share the compute stream's hardware queue (one pool entry in four does): probe, and
        # take a fresh group until one overlaps (harness/dist_util.py); the verdict travels in the line
        from cfdbench_amd.harness.dist_util import steer_comm_stream
        DP["comm_stream_overlaps"] = steer_comm_stream()

    from cfdbench_amd import _lib
    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn

    api = _lib.api()
    B, C, L, H, W, p = args.batch, args.hidden, args.layers, args.height, args.width, args.n_case_params
    if args.only:  # one leg alone (profiling target); not the benchmark line
        if args.only == "spectral":
            out = {"roofline_spectral_conv2d": spectral_leg(api, _lib, dev, B, C, H, W, max(args.steps, 20))}
        elif args.only in MODEL_LEGS:
            if world > 1 or force_dp:  # the leg as a data-parallel job: ONE contract-style line from rank 0
                DP.update(world=world, rank=rank, steps=args.steps, warmup=args.warmup, force=force_dp)
                out = MODEL_LEGS[args.only][1](api, dev)
                if rank == 0:
                    print(json.dumps(out), flush=True)
                dist.barrier()
                dist.destroy_process_group()
                return
            out = {MODEL_LEGS[args.only][0]: MODEL_LEGS[args.only][1](api, dev)}
        else:
            print(f"bench.py: unknown --only {args.only!r}", file=sys.stderr)
            sys.exit(1)
        print(json.dumps(out), flush=True)
        return
    torch.manual_seed(0)  # identical weights on every rank
    model = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C).to(dev)
    eng = FnoTrainEngine(model, lr=1e-3, loss_name="nmse")
    g = torch.Generator(device="cpu").manual_seed(1234 + rank)  # SURVEY.md 8(d) synthetic inputs; a shard per rank
    inputs = torch.randn(B, 2, H, W, generator=g).to(dev)
    label = (inputs.cpu() + 0.1 * torch.randn(B, 2, H, W, generator=g)).to(dev)
    cp = torch.randn(B, p, generator=g).to(dev)
    mask = torch.ones(B, 1, H, W, device=dev)
    step = eng.train_step_graph if args.graph else eng.train_step

    def barrier():
        if world > 1:
            dist.barrier()

    for _ in range(args.settle + args.warmup):
        step(inputs, label, cp, mask)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(inputs, label, cp, mask)
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:  # the last timed step's results, before anything below runs another step
        dump_outputs(args.dump_outputs, dict(preds=eng.preds, loss_sums=eng.sums, params=eng.flat.data, grads=eng.gradients(),
                                             adam_exp_avg=eng.exp_avg, adam_exp_avg_sq=eng.exp_avg_sq))
    final = eng.scores()
    fps = world * B * args.steps / elapsed
    dp_info = None
    if args.full and eng.sync.exchange and not args.graph:
        # what the exchange costs this rank per step: the same K steps with the collectives switched off (same kernels: a data-parallel
        # engine keeps the step's five own launches), between the same barriers.  On N GPUs this is the exposed (un-hidden) part of the
        # all-reduces plus their host calls; it explains the scaling curve the driver computes from the per-N values.
        eng.sync.exchange = False
        for _ in range(3):
            step(inputs, label, cp, mask)
        torch.cuda.synchronize()
        barrier()
        t1 = time.perf_counter()
        for _ in range(args.steps):
            step(inputs, label, cp, mask)
        torch.cuda.synchronize()
        t_no = (time.perf_counter() - t1) / args.steps
        barrier()
        eng.sync.exchange = True
        dp_info = dict(comm_stream_overlaps=DP["comm_stream_overlaps"], step_ms_without_exchange=round(t_no * 1e3, 4),
                       exposed_comm_us=round((elapsed / args.steps - t_no) * 1e6, 1), rank=rank,
                       flat_gradient_bytes=int(eng.flat.numel * 4), buckets="one per backward phase (head, FnoBlocks, lifting layer)")

    result = {
        "metric": "train frames/sec (64x64x2), Auto-FNO cavity", "value": round(fps, 1),
        "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": f"BASELINE configs[1]: Auto-FNO train step (fwd+nMSE+bwd+Adam), Fno2d(L={L},hidden={C},modes=12,p={p}), "
                               f"{H}x{W}, batch {B}/GPU, fp32, random-init weights",
                   "precision": "fp32 storage and accumulation; every contraction on bf16 MFMAs with BOTH operands in three bf16 pieces, six "
                                "products per product term down to 2^-24 (fp32-exact class; nMSE vs the fp64 oracle 4e-14 whole model)",
                   "act_pieces": 3,
                   "global_batch": world * B, "parallelism": f"dp{world}", "graph": bool(args.graph), "settle_steps": args.settle},
        "final_nmse": round(final["nmse"], 6),
    }
    if dp_info:
        result["dp"] = dp_info
    bpf = fno_step_bytes_per_frame(C, L, H * W)
    per_gpu = fps / world
    result["roofline_step"] = dict(bound="hbm", what="whole train step vs the ideal-fusion byte count of SURVEY.md 8(d)", bytes_per_frame=bpf,
                                   achieved=round(per_gpu * bpf / 1e9, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                                   frac=round(per_gpu * bpf / 1e9 / HBM_PEAK_GBS, 4), frames_per_s_at_roofline=round(HBM_PEAK_GBS * 1e9 / bpf, 0))

    # ---- roofline leg: the same K steps again with per-kernel HIP events on the launch stream -------------------
    # EVERY rank runs these steps (they contain the gradient all-reduce, a collective); only rank 0 records events.
    roofline = args.full and not args.no_roofline
    if roofline:
        if rank == 0:
            api.call("cfd_prof_begin")
        for _ in range(args.steps):
            eng.train_step(inputs, label, cp, mask)
        torch.cuda.synchronize()
    if rank == 0 and roofline:
        rows = read_prof(api)
        tot_ms = sum(r[2] for r in rows)
        kern = []
        for r in rows:
            rl = roofline_of(*r) or {}
            kern.append(dict(kernel=r[0], launches_per_step=r[1] // args.steps, avg_us=round(r[2] / r[1] * 1e3, 2),
                             share=round(r[2] / tot_ms, 4), bound=rl.get("bound"), frac=rl.get("frac")))
        result["kernels"] = kern
        result["kernel_time_ms_per_step"] = round(tot_ms / args.steps, 4)
        result["roofline"] = roofline_of(*rows[0])
        attach_pmc(result["roofline"], rows[0][0], B == 256 and C == 20 and (H, W) == (64, 64))
        result["roofline_spectral_conv2d"] = spectral_leg(api, _lib, dev, B, C, H, W, max(args.steps, 20))
        if B == 256 and C == 20 and (H, W) == (64, 64):
            attach_leg_traffic(result["roofline_spectral_conv2d"], "spectral")
        # the north star's own figure and the whole-step fraction ride INSIDE the roofline object (the driver's record keeps that
        # object whole and only the names of the other extra keys)
        sc = result["roofline_spectral_conv2d"]
        result["roofline"]["spectral_conv2d"] = {k: sc.get(k) for k in ("avg_us", "algorithmic_bytes", "achieved", "frac", "traffic", "target_frac", "target_us") if k in sc}
        result["roofline"]["step"] = dict(frac=result["roofline_step"]["frac"], bytes_per_frame=bpf, ms_per_step=result["ms_per_step"])
        # ... and once more as SCALAR keys (round 6: the driver's parse of round 5 kept only the scalar members of `roofline`)
        result["roofline"].update(
            kernel_symbol=ROCPROF_SYMBOL.get(result["roofline"]["kernel"], result["roofline"]["kernel"]),
            spectral_conv2d_us=sc.get("avg_us"), spectral_conv2d_frac=sc.get("frac"), spectral_conv2d_achieved_gbs=sc.get("achieved"),
            spectral_conv2d_bytes=sc.get("algorithmic_bytes"), spectral_conv2d_traffic=sc.get("traffic"),
            step_frac=result["roofline_step"]["frac"], step_bytes_per_frame=bpf, step_ms=result["ms_per_step"])

    extra = args.full and rank == 0 and world == 1
    # ---- rollout legs: batched multi-step inference from one HIP graph (the metric's "rollout" half; configs[4]) ----
    # Cases shard over the ranks with no collective on the data path (harness/test_multistep.py): EVERY rank rolls
    # out its own `--rollout-batch` cases, the legs are bracketed by barriers and timed by the slowest rank (weak scaling).
    def rollout_all_ranks(mdl, Hx, Wx, **kw):
        barrier()
        res, _ = rollout_leg(mdl, args.rollout_batch, args.rollout_steps, Hx, Wx, p, dev, seed=99 + rank, **kw)
        if world > 1:
            t = torch.tensor([res["ms_per_step"]], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            ms = float(t.item())
            scale = res["ms_per_step"] / ms
            res["ms_per_step"] = round(ms, 4)
            res["frames_per_s"] = round(res["frames_per_s"] * scale * world, 1)  # whole job: all ranks' cases / the slowest rank's time
            for k in ("achieved", "frac"):
                res["roofline"][k] = round(res["roofline"][k] * scale, 4)  # per GPU
        res["n_gpus"] = world
        res["cases_per_gpu"] = args.rollout_batch
        return res

    if args.full and not args.no_rollout:
        ro = rollout_all_ranks(model, H, W)
        torch.manual_seed(0)
        m32 = Fno2d(2, 2, p, loss_name_to_fn("nmse"), 4, 12, 12, 32).to(dev)  # the reference's default width (args.py:190)
        ro32 = rollout_all_ranks(m32, 66, 65)
        if rank == 0:
            result["rollout"], result["rollout_66x65"] = ro, ro32
    if extra and not args.no_rollout:
        try:  # the same horizon with four times the cases in flight (the general-grid kernels are latency-bound at 64 cases)
            result["rollout_66x65_256cases"], _ = rollout_leg(m32, 4 * args.rollout_batch, args.rollout_steps, 66, 65, p, dev)
        except Exception as e:  # noqa: BLE001
            result["rollout_66x65_256cases"] = dict(error=str(e)[:200])
        try:
            result["rollout_66x65_bf16"], _ = rollout_leg(m32, args.rollout_batch, args.rollout_steps, 66, 65, p, dev, dtype="bf16")
        except TypeError:
            result["rollout_66x65_bf16"] = None  # bf16 activation storage not built in this tree
        del m32

    # ---- the training step on the 66 x 65 grid of the dam / tube / cylinder problems, and at the reference's default batch ----
    if extra and not args.no_extra:
        def train_leg(Bx, Hx, Wx, Cx, what):
            torch.manual_seed(0)
            mx = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, Cx).to(dev)
            ex = FnoTrainEngine(mx, lr=1e-3, loss_name="nmse")
            gx = torch.Generator(device="cpu").manual_seed(4321)
            xi = torch.randn(Bx, 2, Hx, Wx, generator=gx).to(dev)
            lb = (xi.cpu() + 0.1 * torch.randn(Bx, 2, Hx, Wx, generator=gx)).to(dev)
            cpx = torch.randn(Bx, p, generator=gx).to(dev)
            mk = torch.ones(Bx, 1, Hx, Wx, device=dev)
            dt = min(time_steps(lambda: ex.train_step(xi, lb, cpx, mk), max(args.steps, 20), 10) for _ in range(2))  # best of two timed runs
            mode, dt_eager = "eager launches", dt
            if Bx <= 32:  # launch-bound sizes: forward + backward replayed from one HIP graph (engine.train_step_graph)
                dt_g = min(time_steps(lambda: ex.train_step_graph(xi, lb, cpx, mk), max(args.steps, 20), 10) for _ in range(2))
                if dt_g < dt:
                    dt, mode = dt_g, "forward + backward as one HIP graph, Adam behind it"
            bpf = fno_step_bytes_per_frame(Cx, L, Hx * Wx)
            return dict(what=what, mode=mode, eager_ms_per_step=round(dt_eager * 1e3, 4), ms_per_step=round(dt * 1e3, 4), frames_per_s=round(Bx / dt, 1),
                        roofline_step=dict(bound="hbm", bytes_per_frame=bpf, achieved=round(Bx / dt * bpf / 1e9, 1), peak=HBM_PEAK_GBS,
                                           unit="GB/s", frac=round(Bx / dt * bpf / 1e9 / HBM_PEAK_GBS, 4)))
        try:
            # bf16-storage training: saved activations as bf16, master weights / gradients / Adam fp32; NOT the headline
            # (its results are outside the fp32 path's 1e-5 budget: tests/test_gpu_bf16_train.py states the tolerance)
            torch.manual_seed(0)
            m16 = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C).to(dev)
            e16 = FnoTrainEngine(m16, lr=1e-3, loss_name="nmse", act_dtype="bf16")
            dt16 = min(time_steps(lambda: e16.train_step(inputs, label, cp, mask), max(args.steps, 20), 5) for _ in range(2))
            result["train_bf16_storage"] = dict(
                what=f"the same train step with the saved activations stored as bf16 (fp32 master weights, gradients, accumulation, Adam), batch {B}, {H}x{W}",
                ms_per_step=round(dt16 * 1e3, 4), frames_per_s=round(B / dt16, 1), final_nmse=round(e16.scores()["nmse"], 6))
            del e16, m16
        except Exception as e:  # noqa: BLE001
            result["train_bf16_storage"] = dict(error=str(e)[:300])
        try:
            result["train_66x65"] = train_leg(B, 66, 65, C, f"the same train step on the 66x65 grid (general-width kernels), batch {B}, hidden {C}")
            result["train_batch8"] = train_leg(8, H, W, C, f"the same train step at the reference's default batch size 8 (src/args.py:44), {H}x{W}, hidden {C}")
            # the reference's DEFAULT width (--fno_hidden_dim 32, src/args.py:190) on both grids
            result["train_c32_64x64"] = train_leg(B, H, W, 32, f"the same train step at the reference's default width 32 (src/args.py:190), {H}x{W}, batch {B}")
            result["train_c32_66x65"] = train_leg(B, 66, 65, 32, f"the same train step at width 32 on the 66x65 grid (dam / tube / cylinder), batch {B}")
        except Exception as e:  # noqa: BLE001
            result["train_66x65"] = dict(error=str(e)[:200])

    # ---- the same step on the round 1-4 default route (two-piece activation operands) and on the old fp32-MFMA transforms ----------
    if extra and not args.no_extra:
        def timed_route(knob, value):
            api.call("cfd_tune_set", knob, value)
            try:
                dt = min(time_steps(lambda: eng.train_step(inputs, label, cp, mask), args.steps, 10) for _ in range(2))
                sp = min((spectral_leg(api, _lib, dev, B, C, H, W, max(args.steps, 20)) for _ in range(2)), key=lambda r: r["avg_us"])  # best of two, like dt
            finally:
                api.call("cfd_tune_set", knob, -1)
            return dict(ms_per_step=round(dt * 1e3, 4), frames_per_s=round(B / dt, 1), spectral_conv2d_us=sp["avg_us"], spectral_conv2d_frac=sp["frac"])
        try:
            result["split2"] = dict(
                timed_route(b"act_pieces", 2),
                priced="spectral_conv2d_frac is bytes / time / 8 TB/s (HBM); no matrix-pipe ceiling is applied to this leg (with two activation "
                       "pieces a product costs four bf16 MFMAs, not the six `roofline_of` assumes for the default route)",
                what="the same step / SpectralConv2d group with the ACTIVATION operands in two bf16 pieces (cfd_tune_set('act_pieces', 2), the "
                     "default of rounds 1-4): rel. 2^-16 per product, nMSE vs the fp64 oracle 2e-11 .. 5e-11 per kernel -- NOT fp32-class "
                     "arithmetic, kept as a selectable route")
            result["fp32_mfma_route"] = dict(timed_route(b"exact_fp32", 1),
                                             what="round 1-3's exact route: every DFT / inverse DFT on v_mfma_f32_16x16x4_f32 kernels, the FnoBlock as two passes")
        except Exception as e:  # noqa: BLE001
            result["split2"] = dict(error=str(e)[:300])

    # ---- the PCIe-inclusive rate: the same step fed from PINNED HOST batches (never `value`: the C ABI takes device pointers and the
    # harness keeps the data set resident, harness/data.py:DeviceBatchLoader; this is what a caller that hands over host batches gets) ----
    if extra and not args.no_extra:
        try:
            dev_t = (inputs, label, cp, mask)
            hb = [tuple(t.cpu().pin_memory() for t in dev_t) for _ in range(2)]
            db = [tuple(torch.empty_like(t) for t in dev_t) for _ in range(2)]
            nbytes = sum(t.numel() * t.element_size() for t in dev_t)
            turn = [0]

            def serial_step():  # upload on the step's own stream, then the step
                k = turn[0] & 1
                turn[0] += 1
                for d, h in zip(db[k], hb[k]):
                    d.copy_(h, non_blocking=True)
                eng.train_step(*db[k])
            dt_ser = min(time_steps(serial_step, args.steps, 5) for _ in range(2))
            from cfdbench_amd.harness.data import overlapping_copy_stream
            cur = torch.cuda.current_stream()
            side, side_overlaps = overlapping_copy_stream(dev)  # (one stream in four shares the step's hardware queue and cannot overlap it)
            ready, free = [torch.cuda.Event() for _ in range(2)], [torch.cuda.Event() for _ in range(2)]
            for e in free:
                e.record(cur)

            def upload(k):  # batch k: host -> its device buffers on the copy stream, once the step that last read them has finished
                side.wait_event(free[k])
                with torch.cuda.stream(side):
                    for d, h in zip(db[k], hb[k]):
                        d.copy_(h, non_blocking=True)
                ready[k].record(side)
            turn[0] = 0
            upload(0)

            def overlapped_step():  # step i on buffer set i & 1 while set (i + 1) & 1 is uploaded behind it
                k = turn[0] & 1
                turn[0] += 1
                upload(k ^ 1)
                cur.wait_event(ready[k])
                eng.train_step(*db[k])
                free[k].record(cur)
            dt_ov = min(time_steps(overlapped_step, args.steps, 5) for _ in range(2))
            result["train_host_batches"] = dict(
                what=f"the headline step fed from pinned host batches (inputs, label, mask, case parameters: {nbytes / 1e6:.1f} MB per step over PCIe)",
                serial_ms_per_step=round(dt_ser * 1e3, 4), serial_frames_per_s=round(B / dt_ser, 1),
                overlapped_ms_per_step=round(dt_ov * 1e3, 4), overlapped_frames_per_s=round(B / dt_ov, 1),
                h2d_bytes_per_step=nbytes, serial_h2d_share_ms=round((dt_ser - elapsed / args.steps) * 1e3, 4),
                copy_stream_overlaps=bool(side_overlaps),
                note="serial: hipMemcpyAsync on the step's stream; overlapped: two buffer sets, the next batch's copies on a second stream during the "
                     "step (a stream probed not to share the step's hardware queue: harness/data.py:overlapping_copy_stream).  An upload KERNEL "
                     "reading the pinned pages does not overlap on any stream (tools/exp/host_batches.py)")
            del hb, db
        except Exception as e:  # noqa: BLE001
            result["train_host_batches"] = dict(error=f"{type(e).__name__}: {str(e)[:300]}")

    # ---- other model families of BASELINE.json (one GPU's share of configs[2] and configs[3]) and of SURVEY 8 a-9 / f-3 ----
    if extra and not args.no_extra:
        for leg in MODEL_LEGS:
            try:
                result[MODEL_LEGS[leg][0]] = MODEL_LEGS[leg][1](api, dev)
            except Exception as e:  # noqa: BLE001
                result[MODEL_LEGS[leg][0]] = dict(error=f"{type(e).__name__}: {str(e)[:300]}")

    # ---- CPU baseline leg (rank 0, N=1): the reference's ATen call sequence on the host cores, SURVEY 8(d) protocol -----------
    if extra and not args.no_cpu_baseline:
        from oracle import torch_port
        ncpu = os.cpu_count() or 1
        # kind "port" = oracle/torch_port.py, the reference's PyTorch-CPU call sequence: the reference is Python and cannot travel to
        # the GPU box in any form.  Where /root/reference/src exists (never on a GPU box) the reference's own module is timed too, in a
        # child process, and reported beside the port (`reference_frames_per_s`) -- `value` is the port on every box, so it compares.
        # ATen's CPU kernels do not scale to every hardware thread at this size (one batch-32 step on the GPU box's 256 threads took
        # 28 MINUTES in round 5): sweep {8, 16, 32, 64} with one timed step each at batch 32 inside a 20-s budget, stop at the first
        # count that is slower than its predecessor.
        timer = torch_port.time_train_steps
        cands = sorted({t for t in (8, 16, 32, 64) if t <= ncpu} or {ncpu})
        probe, t_probe0 = {}, time.perf_counter()
        for t in cands:
            probe[t] = timer(32, 1, warmup=1, C=C, L=L, H=H, W=W, p=p, threads=t)["frames_per_s"]
            if time.perf_counter() - t_probe0 > 20.0 or (len(probe) > 1 and probe[t] < 0.8 * max(probe.values())):
                break
        # the batch-32 ranking does not carry over to the full batch (8 threads win at 32, 16 at 256 on the 2 x EPYC 9575F box): the two
        # best probe counts get two steps each on the real workload, the faster one runs the protocol: 3 warm-up + >= 10 timed steps, median
        top = sorted(probe, key=probe.get, reverse=True)[:2]
        pick = {t: timer(B, 2, warmup=1, C=C, L=L, H=H, W=W, p=p, threads=t)["frames_per_s"] for t in top}
        best_t = max(pick, key=pick.get)
        cb = timer(B, max(10, args.cpu_steps), warmup=3, C=C, L=L, H=H, W=W, p=p, threads=best_t)
        cb32 = timer(32, 5, warmup=1, C=C, L=L, H=H, W=W, p=p, threads=best_t)
        ref = None
        if torch_port.reference_importable():
            try:
                ref = torch_port.time_reference_steps(B, max(10, args.cpu_steps), warmup=3, C=C, L=L, H=H, W=W, p=p, threads=best_t)
            except RuntimeError:
                ref = None
        result["cpu_baseline"] = dict(
            value=round(cb["frames_per_s"], 1), unit="frames/s", cores=cb["threads"], kind="port",
            sample=f"the SAME workload (train step fwd+nMSE+bwd+Adam, batch {B}, synthetic inputs of SURVEY 8d) on oracle/torch_port.py (the "
                   f"reference's PyTorch-CPU ATen call sequence, fp32; checked against the oracle in tests/test_oracle_golden.py): {cb['steps']} timed "
                   f"steps after 3 warm-up steps, median; thread count = the faster of { {t: round(v, 1) for t, v in pick.items()} } (two steps "
                   f"each), candidates from a batch-32 sweep { {t: round(v, 1) for t, v in probe.items()} } frames/s; {ncpu} host threads on the box",
            steps=cb["steps"], warmup=3, median_s=round(cb["median_s"], 4), min_s=round(cb["min_s"], 4), max_s=round(cb["max_s"], 4),
            spread=round((cb["max_s"] - cb["min_s"]) / cb["median_s"], 4),
            cpu_model=torch_port.cpu_model(), host_cores=ncpu,
            value_batch32=round(cb32["frames_per_s"], 1), thread_sweep_batch32={str(t): round(v, 1) for t, v in probe.items()},
            reference_frames_per_s=None if ref is None else round(ref["frames_per_s"], 1),
            reference_note=("the reference's own Fno2d (src/models/fno/fno2d.py) timed by the same protocol in a child process" if ref else
                            "the reference is Python source and may not travel to the GPU box: not timed here (in the build container, batch 8 on "
                            "8 threads, the port ran 105 and the reference module 118 frames/s)"))

    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()  # the other ranks wait here while rank 0 finishes its (collective-free) extra legs
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
