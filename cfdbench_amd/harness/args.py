"""Command-line configuration with the reference's flag names and defaults (src/args.py:5-217).

The reference declares flags as annotated class attributes of a ``tap.Tap`` subclass; ``tap`` is not a dependency here, so
the same attribute table drives ``argparse``.  Differences, all documented in SURVEY.md section 0.1:
  * ``lr_step_size`` / ``lr_gamma`` exist (train_auto.py:357 reads ``args.lr_step_size`` but the reference's Args lacks it);
  * ``--data`` is an explicit alias of ``--data_name`` (README.md:179 uses it; argparse prefix matching would be ambiguous);
  * additions: ``infer_steps`` (test_multistep.py:198 hard-codes 20), ``fused`` (FnoTrainEngine instead of autograd+Adam),
    ``resume`` (continue from ``train_state.pt``: optimiser moments, schedule, epoch, RNG -- the reference saves weights only),
    ``device_loader`` (frames resident in HBM, batches gathered on the device instead of DataLoader + collate_fn),
    ``lr_scheduler`` (step = the reference's StepLR | plateau = ReduceLROnPlateau(lr_scheduler_factor, lr_scheduler_patience) |
    cosine), ``early_stop`` (1: stop after early_stopping_patience evaluations without early_stopping_delta improvement),
    ``gradient_accumulation_steps`` (args.py:323; micro-batches per optimiser step),
    ``fno_padding`` (Fno2d's ``padding``: the FnoBlocks run on a grid zero-padded by that many rows and columns; default None),
    ``graph`` (1: the autograd train step -- forward, loss, backward, Adam -- is captured once as a HIP graph and replayed per batch;
    single process, no gradient accumulation, models without per-step host state, i.e. not the ResNet's dropout),
    ``dtype`` ("bf16": the FNO's activations between kernels are stored as bf16 -- test_multistep: BASELINE configs[4];
    train_auto --fused 1: bf16-storage training with fp32 master weights, gradients and optimiser),
    ``unroll_steps`` (train_auto, K > 1: the FNO is trained through a K-step rollout -- loss = mean nmse of K steps with every prediction
    fed back as the next input, cfdbench_amd/unroll.py; 1 = the reference's one-step loop.  On the autograd path, or with --fused 1 as
    FnoTrainEngine windows; with --device_loader 1 on both; with --fused_accumulation_steps N: N windows per optimiser step.  Not with
    --graph 1, not with a model other than the FNO, and with --dtype bf16 only together with --unroll_detach 1),
    ``unroll_detach`` (1: the fed-back frame of a window carries no gradient -- the pushforward trick; the gradient is the mean of K
    one-step gradients taken along the model's own rollout; 0 = the full gradient through every fed-back frame),
    ``max_grad_norm`` (> 0: global gradient-norm clipping at that threshold before every optimiser step -- --fused 1: inside the engine's
    optimiser call, eager paths: torch.nn.utils.clip_grad_norm_; 0.0 = off; not with --graph 1),
    ``fused_accumulation_steps`` (train_auto --fused 1, N > 1: N micro-batches per fused optimiser step -- FnoTrainEngine.accumulate /
    apply_accumulated; what --gradient_accumulation_steps is to the autograd path; not with --graph 1),
    ``freeze`` / ``train_only`` (comma-separated state_dict key prefixes, mutually exclusive: the parameters they cover are frozen /
    are the only ones trained -- ``requires_grad_`` on any model, before the optimiser or engine is built; a prefix that matches nothing
    is an error; --fused 1: FnoTrainEngine trains the subset on compact buffers and stops the backward pass behind its shallowest tensor),
    ``optimizer`` (adam = the reference's loop, ``weight_decay`` still unused as there | adamw = decoupled decay by ``weight_decay``:
    torch.optim.AdamW on the eager paths, FnoTrainEngine(optimizer="adamw") with --fused 1; not with --graph 1),
    ``init_from`` (a model.pt to load through ``load_ckpt`` before training: fine-tuning from another run's weights; ignored, with a log
    line, when --resume 1 finds a train_state.pt),
    ``skip_nonfinite`` (1: an optimiser step whose gradient norm is NaN or inf is skipped instead of applied -- --fused 1: on the device,
    inside the engine's optimiser call, no host sync (FnoTrainEngine(skip_nonfinite=True)); eager paths: the norm of
    torch.nn.utils.clip_grad_norm_ is tested on the host, ONE HOST SYNC PER OPTIMISER STEP; the log line and train_state.pt carry the
    skipped count; not with --graph 1; a run resumed with the other value just continues, the count from the state),
    ``max_consecutive_skips`` (with --skip_nonfinite 1: abort with a RuntimeError once that many optimiser steps in a row were skipped --
    checked at the log interval on the fused path, per step on the eager ones; the last good checkpoint stays; 0 = never abort),
    ``ema_decay`` (D in (0, 1): an exponential moving average of the trainable weights, ``ema = D ema + (1 - D) weights`` behind every
    applied optimiser step -- --fused 1: inside the engine's optimiser launch (FnoTrainEngine(ema_decay=D)), eager paths:
    ``common.EagerEma``; every checkpoint epoch also writes ``ckpt-{ep}/model_ema.pt`` beside ``model.pt``, train_state.pt carries the
    average; 0.0 = off; not with --graph 1),
    ``ema_warmup`` (1: the decay of optimiser step t is min(D, (1 + t) / (10 + t))),
    ``ema_eval`` (1: validation and the final test run on the averaged weights; the trained ones are back afterwards; the multi-step
    rollout of the averaged weights is ``python -m cfdbench_amd.harness.multistep_ema``, which takes test_multistep's flags),
    ``objective`` (train_auto, the fno model: what the step MINIMISES -- nmse = the reference's loop, unchanged | rel_l2 = the per-sample
    relative L2 norm, LpLoss(d=2, p=2).rel of the reference's src/models/fno/utilities3.py | nmse_sample | nmse_channel; --fused 1:
    FnoTrainEngine(objective=), eager: ``loss.ObjectiveLoss``; the loss history and the log line carry its value beside nmse, dev_loss
    and the checkpoint choice stay on nmse; not with --graph 1 or --dtype bf16; hs = the relative Sobolev norm, HsLoss of the same
    file: FnoTrainEngine(objective="hs") / ``loss.SobolevLoss``),
    ``hs_k`` (1 | 2: the highest derivative order of --objective hs), ``hs_a`` (A1[,A2]: the weights of the orders, "" = ones),
    ``hs_group`` (1: HsLoss's balanced form, every order's relative norm on its own).
Flags of models that are not built yet are carried so existing command lines and args.json files keep working.
"""
from __future__ import annotations

import argparse
import json
from typing import Any, Dict, List, Optional

_FLAGS: Dict[str, Any] = dict(
    # 1. general (args.py:22-29)
    mode="train", seed=0, output_dir="result",
    # 2. training (args.py:37-84)
    lr=1e-4, weight_decay=1e-5, num_epochs=100, batch_size=8, eval_batch_size=16,
    lr_scheduler_factor=0.5, lr_scheduler_patience=5, loss_name="mse", log_interval=50, eval_interval=2,
    save_checkpoint_every_n_epochs=20, save_images_every_n_epochs=20, early_stopping_patience=20,
    early_stopping_delta=1e-5,
    # 3. dataset (args.py:88-112)
    data_name="cylinder_geo", data_dir="../data", num_rows=64, num_cols=64, delta_time=0.1, norm_props=1, norm_bc=1,
    # 4. model selection (args.py:119-136)
    model="pixel_diffusion", in_chan=2, out_chan=2,
    # 5. model hyper-parameters (args.py:143-217)
    ffn_depth=8, ffn_width=100, autoffn_depth=8, autoffn_width=200, deeponet_width=100, branch_depth=8, trunk_depth=8,
    act_fn="relu", act_scale_invariant=1, act_on_output=0, autoedeeponet_width=100, autoedeeponet_depth=8,
    autoedeeponet_act_fn="relu", fno_depth=4, fno_hidden_dim=32, fno_modes_x=12, fno_modes_y=12, unet_dim=12,
    unet_insert_case_params_at="input", resnet_depth=4, resnet_hidden_chan=16, resnet_kernel_size=7, resnet_padding=3,
    # missing in the reference's Args but read by its trainers (train_auto.py:357, :188-189)
    lr_step_size=20, lr_gamma=0.9,
    # additions of this harness
    infer_steps=20, fused=0, plot_interval=1, resume=0, device_loader=0, dtype="fp32", graph=0,
    lr_scheduler="step", early_stop=0, gradient_accumulation_steps=1, unroll_steps=1, max_grad_norm=0.0,
    fused_accumulation_steps=1, unroll_detach=0, freeze="", train_only="", optimizer="adam", init_from="",
    skip_nonfinite=0, max_consecutive_skips=100, ema_decay=0.0, ema_warmup=0, ema_eval=0, objective="nmse",
    hs_k=1, hs_a="", hs_group=0,
    # Fno2d(padding=): the reference's constructor argument (fno2d.py:139) that its init_model never passes; None = no domain padding
    fno_padding=None,
)
OBJECTIVES = ("nmse", "rel_l2", "nmse_sample", "nmse_channel")  # --objective: nmse = today's loop
ALL_OBJECTIVES = OBJECTIVES + ("hs",)  # ... and the Sobolev objective with its --hs_* flags


def parse_hs_a(text: str):
    """--hs_a "A1[,A2]" -> (A1[, A2]); "" -> None (ones)."""
    return tuple(float(x) for x in str(text).split(",")) if str(text).strip() else None


def hs_arguments_of(args) -> dict:
    """The (k, a, group) of --objective hs as keyword arguments of ``loss.SobolevLoss``; {} for every other objective."""
    if getattr(args, "objective", "nmse") != "hs":
        return {}
    return dict(k=int(args.hs_k), a=parse_hs_a(args.hs_a), group=bool(args.hs_group))
_OPTIONAL_INT = ("fno_padding",)  # flags whose default is None: parsed as int when given


class Args:
    """Attribute bag with ``parse_args`` / ``save`` / ``as_dict`` like the reference's Tap class."""

    def __init__(self, **overrides):
        for k, v in _FLAGS.items():
            setattr(self, k, v)
        for k, v in overrides.items():
            if k not in _FLAGS:
                raise AttributeError(f"unknown flag {k!r}")
            setattr(self, k, v)

    def parse_args(self, argv: Optional[List[str]] = None) -> "Args":
        ap = argparse.ArgumentParser(allow_abbrev=False)
        for k, v in _FLAGS.items():
            names = [f"--{k}"] + (["--data"] if k == "data_name" else [])
            ap.add_argument(*names, dest=k, type=int if k in _OPTIONAL_INT else type(v), default=getattr(self, k))
        ns = ap.parse_args(argv)
        for k in _FLAGS:
            setattr(self, k, getattr(ns, k))
        return self

    def as_dict(self) -> Dict[str, Any]:
        return {k: getattr(self, k) for k in _FLAGS}

    def save(self, path: str) -> None:
        with open(path, "w") as f:
            json.dump(self.as_dict(), f, indent=4, sort_keys=True)

    def __repr__(self) -> str:
        return "Args(" + ", ".join(f"{k}={getattr(self, k)!r}" for k in _FLAGS) + ")"


def is_args_valid(args: Args) -> None:
    """Validate argument values (src/args.py:372-378): the reference's two asserts (the model name is left to
    ``init_model``, like there), then this harness's own additions -- a flag combination that is not implemented is an
    error, never silently ignored.  Called by every ``main`` right after parsing."""
    assert any(key in args.data_name for key in ["poiseuille", "cavity", "karman", "tube", "dam", "cylinder"])
    assert args.batch_size > 0
    assert args.eval_batch_size > 0 and args.gradient_accumulation_steps >= 1
    assert args.lr_scheduler in ("step", "plateau", "cosine"), args.lr_scheduler
    assert args.dtype in ("fp32", "bf16"), args.dtype
    if args.dtype == "bf16":  # bf16 activation STORAGE: FNO inference (test_multistep) and the fused FNO trainer
        assert args.model == "fno", "--dtype bf16 is built for the FNO (test_multistep, train_auto --fused 1)"
    if args.fused:
        assert args.model == "fno", "--fused 1 is the FnoTrainEngine path"
        assert args.gradient_accumulation_steps == 1, ("--fused 1 takes its micro-batches per optimiser step from "
                                                       "--fused_accumulation_steps N, not from --gradient_accumulation_steps")
    if args.graph:
        assert not args.fused, "--graph 1 captures the autograd step; the fused FNO engine has its own launch path"
        assert args.gradient_accumulation_steps == 1, "--graph 1 captures one optimiser step per batch"
    assert args.fused_accumulation_steps >= 1, "--fused_accumulation_steps counts the micro-batches of one fused optimiser step (1 = none)"
    if args.fused_accumulation_steps > 1:
        assert args.fused, "--fused_accumulation_steps > 1 is the fused FNO engine's option (--fused 1)"
        assert not args.graph, "--fused_accumulation_steps > 1 with --graph 1 is not built"
    assert args.max_grad_norm >= 0.0, "--max_grad_norm is a threshold on the gradient's 2-norm (0 = no clipping)"
    if args.graph:
        assert not args.max_grad_norm > 0.0, "--graph 1 with --max_grad_norm is not built: the captured multi-tensor Adam has no clipping"
    assert args.unroll_steps >= 1, "--unroll_steps counts the model steps of one training window (1 = the one-step loop)"
    assert args.unroll_detach in (0, 1), "--unroll_detach is 0 (full gradient through the fed-back frames) or 1 (none)"
    if args.unroll_steps > 1:
        assert args.model == "fno", ("--unroll_steps > 1 needs the fno model: the one model whose step hands back the gradient of its "
                                     "inputs")
        assert not args.graph, "--unroll_steps > 1 with --graph 1 is not built: the captured step is the one-step loop"
        assert args.dtype == "fp32" or args.unroll_detach, ("--dtype bf16 --unroll_steps > 1 needs --unroll_detach 1: the input gradient "
                                                           "of a bf16-storage pass is not built")
        if not args.fused:
            assert args.gradient_accumulation_steps == 1, "--unroll_steps > 1 on the autograd path needs gradient_accumulation_steps == 1"
    else:
        assert not args.unroll_detach, "--unroll_detach 1 is an option of --unroll_steps > 1"
    assert not (args.freeze and args.train_only), "--freeze and --train_only are mutually exclusive: give one of them"
    assert args.optimizer in ("adam", "adamw"), "--optimizer is adam (weight_decay unused, as in the reference) or adamw (decoupled decay)"
    if args.graph:
        assert args.optimizer == "adam", "--graph 1 with --optimizer adamw is not built: cfd_adam_multi has no decoupled form"
    assert args.skip_nonfinite in (0, 1), "--skip_nonfinite is 0 (apply every step, the reference's loop) or 1 (skip non-finite steps)"
    assert args.max_consecutive_skips >= 0, "--max_consecutive_skips counts skipped optimiser steps in a row (0 = never abort)"
    if args.graph:
        assert not args.skip_nonfinite, "--graph 1 with --skip_nonfinite 1 is not built: cfd_adam_multi has no flags to carry the guard"
    assert 0.0 <= args.ema_decay < 1.0, "--ema_decay is the decay of the averaged weights, 0 <= D < 1 (0 = no average)"
    assert args.ema_warmup in (0, 1) and args.ema_eval in (0, 1), "--ema_warmup / --ema_eval are 0 or 1"
    if not args.ema_decay > 0.0:
        assert not args.ema_warmup and not args.ema_eval, "--ema_warmup / --ema_eval are options of --ema_decay D > 0"
    if args.graph:
        assert not args.ema_decay > 0.0, "--graph 1 with --ema_decay is not built: cfd_adam_multi has no averaged form"
    assert args.objective in ALL_OBJECTIVES, f"--objective is one of {', '.join(ALL_OBJECTIVES)}"
    if args.objective == "hs":
        assert args.hs_k in (1, 2), "--hs_k is 1 or 2"
        assert args.hs_group in (0, 1), "--hs_group is 0 or 1"
        try:
            hs_a = parse_hs_a(args.hs_a)
        except ValueError:
            raise AssertionError("--hs_a is A1 or A1,A2: numbers separated by a comma") from None
        assert hs_a is None or len(hs_a) == args.hs_k, "--hs_a gives one weight per order: --hs_k numbers"
    else:
        assert args.hs_k == 1 and args.hs_a == "" and args.hs_group == 0, "--hs_k / --hs_a / --hs_group are options of --objective hs"
    if args.objective != "nmse":
        assert args.model == "fno", "--objective other than nmse is built for the fno model (its gradient enters Fno2d's backward pass)"
        assert not args.graph, "--graph 1 with an --objective is not built: the captured step backpropagates loss['nmse']"
        assert args.dtype == "fp32", "--dtype bf16 with an --objective is not built: bf16 storage runs the one-pass head"
        assert args.loss_name == "nmse", "an --objective keeps --loss_name nmse for the reported scores"
    assert args.unet_insert_case_params_at in ("input", "hidden")
    if args.fno_padding is not None:
        assert args.model == "fno", "--fno_padding is Fno2d's domain padding"
        assert args.fno_padding >= 1, "--fno_padding must be >= 1 (leave it out for no padding)"
        assert args.dtype == "fp32", "--fno_padding runs with fp32 activation storage (--dtype bf16 is refused by the library)"
