"""Training through a K-step rollout: the loss of K model steps with every prediction fed back as the next input, differentiated through
the fed-back frames (``Fno2d.forward`` hands autograd the gradient of its inputs: functional.FnoForwardFn, csrc/ingrad.hip).

The autoregressive datasets (harness/flow_data.FlowAutoDataset, harness/data.SyntheticAutoDataset) keep ``inputs``, ``labels`` and
``case_ids`` flat -- item i is (frame t, frame t + time_step_size) of a case -- so the label of step k of a window that starts at item i is
``labels[i + k * time_step_size]`` and no new storage is needed."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import torch
from torch import Tensor


def unroll_windows(dataset, K: int) -> Tuple[List[int], Tensor]:
    """The windows of ``K`` consecutive steps inside one case: ``(starts, label_idx)`` with ``starts`` the item indices i for which
    i + (K - 1) * time_step_size lies in the same case as i, and ``label_idx`` (len(starts), K) the item whose label frame step k of the
    window is trained against (column 0 is the start itself)."""
    if K < 1:
        raise ValueError("unroll_windows: K must be at least 1")
    step = int(getattr(dataset, "time_step_size", 1))
    case_ids = [int(c) for c in dataset.case_ids]
    n = len(case_ids)
    last = (K - 1) * step
    starts = [i for i in range(n - last) if case_ids[i + last] == case_ids[i]]
    label_idx = torch.tensor([[i + k * step for k in range(K)] for i in starts], dtype=torch.long).reshape(len(starts), K)
    return starts, label_idx


def unrolled_loss(model, inputs: Tensor, labels_seq: Sequence[Tensor], case_params: Tensor, mask: Optional[Tensor] = None,
                  detach: bool = False, key: str = "nmse"):
    """``preds_1 = model(inputs)``, ``preds_k = model(preds_{k-1})``; returns ``(loss, preds)`` with ``loss = (1/K) sum_k nmse_k`` against
    ``labels_seq[k - 1]`` and ``preds`` the K predictions.  ``key``: the entry of the model's loss dict to sum, e.g. "rel_l2" for a
    model built with ``loss.objective_to_fn("rel_l2")``.  ``loss.backward()`` reaches the parameters through every fed-back frame.

    ``detach`` (the pushforward trick): the fed-back frame is ``preds.detach()`` -- step k + 1 trains on the model's own prediction as a
    constant input, so the gradient is the sum of K one-step gradients and nothing flows through the frames."""
    K = len(labels_seq)
    if K < 1:
        raise ValueError("unrolled_loss: no label frames")
    if labels_seq[0].shape[1] != inputs.shape[1]:
        raise ValueError(f"unrolled_loss: the predictions are fed back as inputs, so in_chan == out_chan is required "
                         f"(inputs have {inputs.shape[1]} channels, labels {labels_seq[0].shape[1]})")
    x, preds, loss = inputs, [], None
    for label in labels_seq:
        out = model(inputs=x, case_params=case_params, mask=mask, label=label)
        preds.append(out["preds"])
        x = out["preds"].detach() if detach else out["preds"]
        loss = out["loss"][key] if loss is None else loss + out["loss"][key]
    return loss / K, preds


def collate_windows(dataset, label_idx: Tensor, windows: Sequence[int], collate_fn, device: Optional[str] = "cuda") -> dict:
    """The batch of the windows numbered ``windows`` (rows of ``label_idx``): ``collate_fn``'s batch of the start items plus ``labels_seq``,
    the K label frames without their mask channel (``labels_seq[0]`` is the batch's ``label``)."""
    rows = label_idx[torch.as_tensor(list(windows), dtype=torch.long)]
    batch = collate_fn([dataset[int(i)] for i in rows[:, 0]], device=device)
    seq = [batch["label"]]
    for k in range(1, rows.shape[1]):
        frames = dataset.labels[rows[:, k].to(dataset.labels.device)][:, :-1]
        seq.append(frames.to(batch["label"].device).contiguous())
    batch["labels_seq"] = seq
    return batch
