"""``MseLoss`` / ``loss_name_to_fn`` with the reference's names and semantics (src/models/loss.py:8-50); the three
full-tensor reductions run as ONE fused HIP pass instead of F.mse_loss + F.l1_loss + mean, the whole loss as one autograd node
(functional.MseLossFn: cfd_mse_loss_fwd / cfd_mse_loss_bwd)."""
from typing import List

from torch import Tensor, nn

from .._capi import OBJECTIVE_IDS
from ..functional import mse_loss_scores, objective_loss, sobolev_loss


class MseLoss(nn.Module):
    def __init__(self, normalize: bool, is_masked: bool = False):
        super().__init__()
        self.normalize = normalize
        self.is_masked = is_masked

    def get_score_names(self) -> List[str]:  # loss.py:14-20
        names = ["mse", "rmse", "mae"]
        if self.normalize:
            names += ["nmse"]
        return names

    def forward(self, preds: Tensor, labels: Tensor) -> dict:  # loss.py:22-37
        return mse_loss_scores(preds, labels, self.normalize)


class ObjectiveLoss(MseLoss):
    """The four scores of ``MseLoss(normalize=True)`` plus a training objective under its own name ("rel_l2": the per-sample relative L2
    norm, LpLoss(d=2, p=2).rel of the reference's src/models/fno/utilities3.py; "nmse_sample"; "nmse_channel"), listed last.  A model
    that knows its mask (Fno2d) evaluates the objective with it."""

    def __init__(self, objective: str):
        if objective not in OBJECTIVE_IDS:
            raise NotImplementedError
        super().__init__(normalize=True)
        self.objective = objective

    def get_score_names(self) -> List[str]:
        return super().get_score_names() + [self.objective]

    def objective_value(self, preds: Tensor, labels: Tensor, mask=None) -> Tensor:
        return objective_loss(preds, labels, self.objective, mask)

    def forward(self, preds: Tensor, labels: Tensor) -> dict:
        out = super().forward(preds, labels)
        out[self.objective] = self.objective_value(preds, labels)
        return out


class SobolevLoss(ObjectiveLoss):
    """The four scores of ``MseLoss(normalize=True)`` plus "hs", the relative Sobolev norm HsLoss(d=2, p=2, k, a, group) of the reference's
    src/models/fno/utilities3.py (``functional.sobolev_loss``), listed last."""

    def __init__(self, k: int = 1, a=None, group: bool = False):
        from ..sobolev import HS_NAME, hs_arguments
        hs_arguments(k, a, group)  # (raises on what the kernels refuse)
        MseLoss.__init__(self, normalize=True)
        self.objective = HS_NAME
        self.hs_k, self.hs_a, self.hs_group = int(k), (None if a is None else tuple(float(x) for x in a)), bool(group)

    def objective_value(self, preds: Tensor, labels: Tensor, mask=None) -> Tensor:
        return sobolev_loss(preds, labels, mask, self.hs_k, self.hs_a, self.hs_group)


def objective_to_fn(name: str, **hs) -> MseLoss:
    """"nmse" (``loss_name_to_fn``'s), an objective's name, or "hs" with ``SobolevLoss``'s arguments (k, a, group); anything else raises
    like ``loss_name_to_fn``."""
    name = name.lower()
    if name == "hs":
        return SobolevLoss(**hs)
    if hs:
        raise ValueError(f"k, a and group are arguments of the objective 'hs', not of {name!r}")
    return ObjectiveLoss(name) if name in OBJECTIVE_IDS else loss_name_to_fn(name)


def loss_name_to_fn(name: str, masked: bool = False) -> MseLoss:  # loss.py:40-50
    name = name.lower()
    if masked:
        raise NotImplementedError
    if name == "mse":
        return MseLoss(normalize=False)
    if name == "nmse":
        return MseLoss(normalize=True)
    raise NotImplementedError
