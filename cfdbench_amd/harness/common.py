"""Result-tree and checkpoint conventions of the reference (src/utils/common.py:16-33,161-284).  File names and JSON
schemas are what scripts/visualization/get_result.py:19-37 and plot_multistep_inference.py:107-110 read."""
from __future__ import annotations

import contextlib
import json
from pathlib import Path
from typing import List, Optional, Union

import torch


def dump_json(data, path):  # common.py:16-23
    with open(path, "w", encoding="utf8") as f:
        json.dump(data, f, indent=4, ensure_ascii=False)


def load_json(path):  # common.py:26-33
    with open(path, "r", encoding="utf8") as f:
        return json.load(f)


def get_output_dir(args, is_auto: bool = False) -> Path:
    """result/{auto|non-auto}/{data_name}/dt{delta_time}/{model}/{hyper-parameter string}  (common.py:182-275)."""
    output_dir = Path(args.output_dir, "auto" if is_auto else "non-auto", args.data_name, f"dt{args.delta_time}", args.model)
    m = args.model
    if m == "deeponet":
        name = (f"lr{args.lr}_width{args.deeponet_width}_depthb{args.branch_depth}_deptht{args.trunk_depth}"
                f"_normprop{args.norm_props}_act{args.act_fn}-{args.act_scale_invariant}-{args.act_on_output}")
    elif m == "unet":
        name = f"lr{args.lr}_d{args.unet_dim}_cp{args.unet_insert_case_params_at}"
    elif m == "fno":
        name = f"lr{args.lr}_d{args.fno_depth}_h{args.fno_hidden_dim}_m1{args.fno_modes_x}_m2{args.fno_modes_y}"
        if getattr(args, "fno_padding", None) is not None:  # (only when set: every run without padding keeps its directory)
            name += f"_pad{args.fno_padding}"
        if getattr(args, "objective", "nmse") != "nmse":  # (likewise: a run on another objective gets a directory of its own)
            name += f"_obj-{args.objective}"
            if args.objective == "hs":  # (_obj-hs-k{k}[-a...][-grp])
                name += f"-k{args.hs_k}" + (f"-a{args.hs_a}" if args.hs_a else "") + ("-grp" if args.hs_group else "")
    elif m == "resnet":
        name = f"lr{args.lr}_d{args.resnet_depth}_w{args.resnet_hidden_chan}"
    elif m == "auto_edeeponet":
        name = (f"lr{args.lr}_width{args.autoedeeponet_width}_depthb{args.autoedeeponet_depth}"
                f"_deptht{args.autoedeeponet_depth}_normprop{args.norm_props}_act{args.autoedeeponet_act_fn}")
    elif m == "auto_deeponet":
        name = (f"lr{args.lr}_width{args.deeponet_width}_depthb{args.branch_depth}_deptht{args.trunk_depth}"
                f"_normprop{args.norm_props}_act{args.act_fn}")
    elif m == "auto_ffn":
        name = f"lr{args.lr}_width{args.autoffn_width}_depth{args.autoffn_depth}"
    elif m == "auto_deeponet_cnn":
        name = f"lr{args.lr}_depth{args.autoffn_depth}"
    elif m == "ffn":
        name = f"lr{args.lr}_width{args.ffn_width}_depth{args.ffn_depth}"
    else:
        raise NotImplementedError(f"get_output_dir: model {m!r}")
    return output_dir / name


def get_best_ckpt(output_dir: Path) -> Union[Path, None]:
    """ckpt-* directory with the smallest dev_loss in its scores.json; None if there is none (common.py:161-174)."""
    best_loss, best = float("inf"), None
    for ckpt_dir in sorted(Path(output_dir).glob("ckpt-*")):
        dev_loss = load_json(ckpt_dir / "scores.json")["dev_loss"]
        if dev_loss < best_loss:
            best_loss, best = dev_loss, ckpt_dir
    return best


def load_ckpt(model, ckpt_path: Path) -> None:  # common.py:177-179
    print(f"Loading checkpoint from {ckpt_path}")
    model.load_state_dict(torch.load(ckpt_path, map_location="cpu"))


def split_prefixes(text: str) -> List[str]:
    """``--freeze a,b`` / ``--train_only a,b`` -> ["a", "b"]."""
    return [q.strip() for q in (text or "").split(",") if q.strip()]


def apply_trainable(model, freeze: str = "", train_only: str = "") -> List[str]:
    """--freeze / --train_only on any model: ``requires_grad_`` by state_dict key prefix (engine.match_prefixes: a prefix that matches
    nothing is an error), before the optimiser or engine is built.  Returns the names left trainable."""
    from ..engine import match_prefixes
    fr, only = split_prefixes(freeze), split_prefixes(train_only)
    if fr and only:
        raise ValueError("--freeze and --train_only are mutually exclusive")
    named = list(model.named_parameters())
    names = [k for k, _ in named]
    if fr or only:
        hit = match_prefixes(names, fr or only)
        for (_, p_), h in zip(named, hit):
            p_.requires_grad_(h != bool(fr))
    left = [k for k, p_ in named if p_.requires_grad]
    if not left:
        raise ValueError("--freeze / --train_only leave nothing trainable")
    return left


def make_optimizer(params, kind: str, lr, weight_decay: float = 0.0, **kw):
    """The eager paths' optimiser: adam = torch.optim.Adam as in the reference (``weight_decay`` is not passed, as there); adamw =
    torch.optim.AdamW with ``weight_decay``, decoupled."""
    if kind == "adam":
        return torch.optim.Adam(params, lr=lr, **kw)
    if kind == "adamw":
        return torch.optim.AdamW(params, lr=lr, weight_decay=float(weight_decay), **kw)
    raise ValueError("optimizer must be 'adam' or 'adamw'")


class SkipGuard:
    """--skip_nonfinite / --max_consecutive_skips: the count of skipped optimiser steps and the rule that ends a hopeless run, for every
    trainer.  The eager paths decide on the host (``eager_step``: one sync per optimiser step); the fused engine decides on the device
    and hands its counters over where the loop reads device scalars anyway (``check``)."""

    def __init__(self, enabled: bool = False, max_consecutive: int = 100, skipped: int = 0):
        self.enabled, self.max_consecutive = bool(enabled), int(max_consecutive)
        self.skipped, self.consecutive = int(skipped), 0

    def check(self, consecutive: int, ep: int, step: int, skipped: Optional[int] = None) -> None:
        """RuntimeError once ``max_consecutive`` (> 0) optimiser steps in a row were skipped: a run that silently skips everything is
        worse than one that stops.  Raised before anything is written: the last good checkpoint stays in place."""
        if skipped is not None:
            self.skipped = int(skipped)
        self.consecutive = int(consecutive)
        if self.enabled and 0 < self.max_consecutive <= self.consecutive:
            raise RuntimeError(f"--skip_nonfinite: {self.consecutive} optimiser steps in a row had a non-finite gradient norm "
                               f"(epoch {ep}, step {step}; {self.skipped} skipped in all; --max_consecutive_skips "
                               f"{self.max_consecutive}): the run is not training any more")

    def eager_step(self, params, optimizer, max_grad_norm: float, ep: int, step: int):
        """The optimiser step of an eager path behind backward and the gradient exchange: norm = clip_grad_norm_(params, max_grad_norm
        or inf) -- ``.item()`` on it is the one host sync per step this option costs here -- and ``optimizer.step()`` only when it is
        finite.  Returns (norm, applied)."""
        norm = torch.nn.utils.clip_grad_norm_(params, float(max_grad_norm) if float(max_grad_norm) > 0.0 else float("inf"))
        if bool(torch.isfinite(norm).item()):
            optimizer.step()
            self.consecutive = 0
            return norm, True
        self.skipped += 1
        self.check(self.consecutive + 1, ep, step)
        return norm, False


class EagerEma:
    """--ema_decay on the eager training paths: an exponential moving average of the TRAINABLE parameters with the rule of the fused
    engine (FnoTrainEngine(ema_decay=): cfd_fno_adam_step_ema) in torch -- ``ema.mul_(d_t).add_(p, alpha=1 - d_t)`` with d_t =
    ``decay``, or with ``warmup`` min(decay, (1 + t) / (10 + t)), t = the optimiser step's number (1 for the first; it runs on over a
    skipped step).  d_t and 1 - d_t are the fp32 values the engine's kernel works with: d_t formed in double and rounded once, 1 - d_t
    formed in fp32.  The average starts as a copy of the weights; frozen parameters (and buffers) are their own average.  ``update`` is
    called behind every optimiser step with whether it was applied (``SkipGuard.eager_step``): a skipped step leaves the average alone."""

    def __init__(self, model, decay: float, warmup: bool = False):
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError("ema_decay must be >= 0 and < 1")
        self.model, self.decay, self.warmup = model, float(decay), bool(warmup)
        self.step_count = 0
        self.named = [(k, p_) for k, p_ in model.named_parameters() if p_.requires_grad]
        self.shadow = [p_.detach().clone() for _, p_ in self.named]

    def decay_at(self, t: int) -> float:
        return min(self.decay, (1.0 + t) / (10.0 + t)) if self.warmup else self.decay

    @torch.no_grad()
    def update(self, applied: bool = True) -> None:
        self.step_count += 1
        if not applied:
            return
        d = torch.tensor(self.decay_at(self.step_count), dtype=torch.float32)
        d, omd = float(d), float(torch.tensor(1.0, dtype=torch.float32) - d)
        for e, (_, p_) in zip(self.shadow, self.named):
            e.mul_(d).add_(p_.detach(), alpha=omd)

    def ema_state_dict(self):
        """The model's ``state_dict`` (reference keys) with the averaged tensors in place of the trainable ones; copies."""
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for (k, _), e in zip(self.named, self.shadow):
            sd[k] = e.detach().clone()
        return sd

    @contextlib.contextmanager
    def averaged(self):
        """Inside: the model holds the averaged weights; on exit the trained ones are back, bit for bit."""
        with torch.no_grad():
            saved = [p_.detach().clone() for _, p_ in self.named]
            for (_, p_), e in zip(self.named, self.shadow):
                p_.copy_(e)
        try:
            yield self.model
        finally:
            with torch.no_grad():
                for (_, p_), s in zip(self.named, saved):
                    p_.copy_(s)

    def state_dict(self):
        return dict(ema=[e.detach().clone() for e in self.shadow], ema_step_count=int(self.step_count), ema_decay=self.decay)

    def load_state_dict(self, state) -> None:
        """A state without the average (a run without --ema_decay) restarts it from the weights the model holds now."""
        with torch.no_grad():
            src = state.get("ema") if state else None
            for i, (e, (_, p_)) in enumerate(zip(self.shadow, self.named)):
                e.copy_(p_.detach() if src is None else src[i].to(e.device))
        self.step_count = int(state.get("ema_step_count", 0)) if state else 0


def averaged_weights(ema):
    """``with averaged_weights(x):`` -- x an FnoTrainEngine with ema_decay, an EagerEma, or None (no average: nothing happens)."""
    return contextlib.nullcontext() if ema is None else ema.averaged()


def best_ckpt_file(output_dir: Path, use_ema: bool = False) -> Path:
    """``model.pt`` of the ckpt-* directory with the smallest dev loss -- with ``use_ema`` the averaged weights the run wrote beside it
    (``model_ema.pt``, --ema_decay); a run that kept none is an error that names the file."""
    print(f"Finding the best checkpoint from {output_dir}")
    best = get_best_ckpt(output_dir)
    assert best is not None, f"no ckpt-*/scores.json under {output_dir}"
    if use_ema and not (best / "model_ema.pt").exists():
        raise FileNotFoundError(f"{best / 'model_ema.pt'} does not exist: the run that wrote {best.name} kept no averaged weights (train "
                                "it with --ema_decay D), so there is nothing to load")
    return best / ("model_ema.pt" if use_ema else "model.pt")


def load_best_ckpt(model, output_dir: Path, use_ema: bool = False) -> Path:  # common.py:278-284
    path = best_ckpt_file(output_dir, use_ema)
    print(f"Loading best checkpoint from {path.parent}")
    load_ckpt(model, path)
    return path.parent


# ---- plotting (common.py:35-158): same artefact names; out of scope for acceleration, skipped without matplotlib ----
def _plt():
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        return plt
    except Exception:  # noqa: BLE001
        return None


def plot_loss(losses, out: Path, fontsize: int = 12, linewidth: int = 2):
    plt = _plt()
    if plt is None:
        return
    plt.plot(losses, linewidth=linewidth)
    plt.xlabel("Step", fontsize=fontsize)
    plt.ylabel("Loss", fontsize=fontsize)
    plt.savefig(out)
    plt.clf()
    plt.close()


def plot_predictions(label, pred, out_dir: Path, step: int, inp: Optional[torch.Tensor] = None):
    """images/{input,label,pred}/{step:04d}.png as the reference writes them (common.py:35-93)."""
    plt = _plt()
    if plt is None:
        return
    for name, t in (("input", inp), ("label", label), ("pred", pred)):
        if t is None:
            continue
        d = Path(out_dir) / name
        d.mkdir(exist_ok=True, parents=True)
        plt.imsave(d / f"{step:04d}.png", t.detach().float().cpu().numpy(), cmap="coolwarm")


def plot(inp, label, pred, out_path: Path):
    plt = _plt()
    if plt is None:
        return
    fig, axs = plt.subplots(1, 3, figsize=(9, 3))
    for ax, t, title in zip(axs, (inp, label, pred), ("input", "label", "pred")):
        ax.imshow(t.detach().float().cpu().numpy(), cmap="coolwarm")
        ax.set_title(title)
        ax.axis("off")
    fig.savefig(out_path, bbox_inches="tight")
    plt.close(fig)
