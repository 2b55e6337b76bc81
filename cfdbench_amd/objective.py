"""The autograd node of the training objectives beside mse / nmse / mae (include/cfdbench_amd.h, "Training objectives";
csrc/objective.hip).  ``functional.objective_loss`` is the public entry; ``FnoTrainEngine(objective=)`` calls the same two entry points
without autograd."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from . import _lib
from ._capi import CFD_OBJ_REC_FLOATS
from .functional import _f32c, _ptr, _require_cuda, _stream


class ObjectiveLossFn(torch.autograd.Function):
    """A training objective beside mse / nmse / mae (include/cfdbench_amd.h, "Training objectives") as ONE autograd node: forward is
    cfd_objective_fwd, backward cfd_objective_bwd with the upstream gradient read on the device (``upstream_dev``: no host sync).
    Differentiable in ``preds``; ``labels`` and ``mask`` get no gradient."""

    @staticmethod
    def forward(ctx, preds: Tensor, labels: Tensor, mask: Optional[Tensor], kind: int):
        _require_cuda(preds, labels, mask)
        if preds.shape != labels.shape or preds.dim() < 2:
            raise RuntimeError(f"objective_loss: preds {tuple(preds.shape)} vs labels {tuple(labels.shape)} (at least (B, C))")
        p, l, m = _f32c(preds), _f32c(labels.detach()), _f32c(None if mask is None else mask.detach())
        B, Co = p.shape[0], (p.shape[1] if p.dim() > 2 else 1)
        HW = p.numel() // (B * Co) if p.numel() else 0
        if m is not None and m.numel() != B * HW:
            raise RuntimeError(f"objective_loss: mask {tuple(mask.shape)} is not one value per sample and pixel of preds {tuple(preds.shape)}")
        rec = torch.empty(CFD_OBJ_REC_FLOATS(B, Co), dtype=torch.float32, device=p.device)
        value = torch.empty((), dtype=torch.float32, device=p.device)
        _lib.api().call("cfd_objective_fwd", _ptr(p), _ptr(l), _ptr(m), _ptr(rec), _ptr(value), B, Co, HW, kind, _stream())
        ctx.save_for_backward(p, l, rec, *([m] if m is not None else []))
        ctx.dims, ctx.in_dtype = (B, Co, HW, kind), preds.dtype
        return value

    @staticmethod
    def backward(ctx, g: Tensor):
        p, l, rec, *m = ctx.saved_tensors
        B, Co, HW, kind = ctx.dims
        gp = torch.empty_like(p)
        _lib.api().call("cfd_objective_bwd", _ptr(p), _ptr(l), _ptr(m[0] if m else None), _ptr(rec), None, _ptr(_f32c(g)), 1.0, _ptr(gp),
                        B, Co, HW, kind, _stream())
        return gp.to(ctx.in_dtype), None, None, None
