"""``MseLoss`` / ``loss_name_to_fn`` with the reference's names and semantics (src/models/loss.py:8-50); the three
full-tensor reductions run as ONE fused HIP pass instead of F.mse_loss + F.l1_loss + mean, the whole loss as one autograd node
(functional.MseLossFn: cfd_mse_loss_fwd / cfd_mse_loss_bwd)."""
from typing import List

from torch import Tensor, nn

from .._capi import OBJECTIVE_IDS
from ..functional import mse_loss_scores, objective_loss


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

    def forward(self, preds: Tensor, labels: Tensor) -> dict:
        out = super().forward(preds, labels)
        out[self.objective] = objective_loss(preds, labels, self.objective)
        return out


def objective_to_fn(name: str) -> MseLoss:
    """"nmse" (``loss_name_to_fn``'s) or an objective's name; anything else raises like ``loss_name_to_fn``."""
    name = name.lower()
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
