"""Reference-pinned fixture of the relative L2 objective:
  tests/golden/lploss_rel.npz   B 3, 2 channels, 5 x 7: seeded fp32 preds (carrying the mask), label and a 0/1 mask, and in fp64 the value
                                and the autograd gradient with respect to preds of the reference's LpLoss(d=2, p=2).rel(preds, label * mask)
                                (src/models/fno/utilities3.py) evaluated on those inputs cast to fp64.
tests/test_cpu_objective.py holds tests/objective_checks.reference to it, tests/test_gpu_fno_objective.py the kernels.  Writes the fixture
only.  Run from the repository root where the reference sources are present (oracle/make_golden.py finds them):
    python tools/make_golden_lploss.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import oracle.make_golden  # noqa: E402,F401  (puts the reference's src on the path)
from models.fno.utilities3 import LpLoss  # noqa: E402  (the reference's module)

OUT = REPO / "tests" / "golden"
B, CO, H, W, SEED = 3, 2, 5, 7, 20


def main():
    rng = np.random.default_rng(SEED)
    mask = (rng.random((B, 1, H, W)) > 0.2).astype(np.float32)
    preds = (rng.standard_normal((B, CO, H, W)).astype(np.float32) * mask).astype(np.float32)
    label = (rng.standard_normal((B, CO, H, W)) * (1.0 + np.arange(B)[:, None, None, None])).astype(np.float32)
    x = torch.from_numpy(preds.astype(np.float64)).requires_grad_(True)
    y = torch.from_numpy(label.astype(np.float64)) * torch.from_numpy(mask.astype(np.float64))
    value = LpLoss(d=2, p=2).rel(x, y)
    value.backward()
    np.savez(OUT / "lploss_rel.npz", preds=preds, label=label, mask=mask, value=np.float64(value.item()), grad=x.grad.numpy(),
             meta=np.array([B, CO, H, W, SEED]))
    print(OUT / "lploss_rel.npz", value.item())


if __name__ == "__main__":
    main()
