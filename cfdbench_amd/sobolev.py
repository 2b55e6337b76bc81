"""The autograd node of the Sobolev (H^s) objective (include/cfdbench_amd.h, "Sobolev objective"; csrc/sobolev.hip): the reference's
HsLoss of src/models/fno/utilities3.py.  ``functional.sobolev_loss`` is the public entry; ``FnoTrainEngine(objective="hs")`` calls the same
two entry points without autograd."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from ._capi import CFD_HS_REC_FLOATS
from .functional import _f32c, _ptr, _require_cuda, _stream

HS_NAME = "hs"  # the objective's name: FnoTrainEngine(objective=), --objective, the entry of a loss dict


def hs_arguments(k: int = 1, a: Optional[Sequence[float]] = None, group: bool = False) -> Tuple[int, float, float, int]:
    """(k, a1, a2, balanced) as cfd_sobolev_fwd / _bwd take them, from HsLoss's (k, a, group): k is 1 or 2, ``a`` None (all ones) or at
    least k numbers; a2 is 1 where k = 1 (not read)."""
    if isinstance(k, bool) or int(k) != k or int(k) not in (1, 2):
        raise ValueError(f"the Sobolev objective is built for k = 1 and k = 2, not k = {k!r}")
    k = int(k)
    if a is None:
        a = (1.0,) * k
    a = tuple(float(x) for x in a)
    if len(a) < k:
        raise ValueError(f"the Sobolev objective with k = {k} needs {k} coefficients a, got {a}")
    return k, a[0], (a[1] if k == 2 else 1.0), int(bool(group))


class SobolevLossFn(torch.autograd.Function):
    """The Sobolev objective as ONE autograd node: forward is cfd_sobolev_fwd, backward cfd_sobolev_bwd with the upstream gradient read on
    the device (``upstream_dev``: no host sync).  Differentiable in ``preds``; ``labels`` and ``mask`` get no gradient."""

    @staticmethod
    def forward(ctx, preds: Tensor, labels: Tensor, mask: Optional[Tensor], k: int, a1: float, a2: float, balanced: int):
        _require_cuda(preds, labels, mask)
        if preds.shape != labels.shape or preds.dim() != 4:
            raise RuntimeError(f"sobolev_loss: preds {tuple(preds.shape)} vs labels {tuple(labels.shape)}: both (B, C, H, W)")
        p, l, m = _f32c(preds), _f32c(labels.detach()), _f32c(None if mask is None else mask.detach())
        B, Co, H, W = p.shape
        if m is not None and m.numel() != B * H * W:
            raise RuntimeError(f"sobolev_loss: mask {tuple(mask.shape)} is not one value per sample and pixel of preds {tuple(preds.shape)}")
        rec = torch.empty(CFD_HS_REC_FLOATS(B, Co), dtype=torch.float32, device=p.device)
        value = torch.empty((), dtype=torch.float32, device=p.device)
        _lib.api().call("cfd_sobolev_fwd", _ptr(p), _ptr(l), _ptr(m), _ptr(rec), _ptr(value), B, Co, H, W, k, a1, a2, balanced, _stream())
        ctx.save_for_backward(p, l, rec, *([m] if m is not None else []))
        ctx.dims, ctx.in_dtype = (B, Co, H, W, k, a1, a2, balanced), preds.dtype
        return value

    @staticmethod
    def backward(ctx, g: Tensor):
        p, l, rec, *m = ctx.saved_tensors
        gp = torch.empty_like(p)
        _lib.api().call("cfd_sobolev_bwd", _ptr(p), _ptr(l), _ptr(m[0] if m else None), _ptr(rec), None, _ptr(_f32c(g)), 1.0, _ptr(gp),
                        *ctx.dims, _stream())
        return gp.to(ctx.in_dtype), None, None, None, None, None, None
