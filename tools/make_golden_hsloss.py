"""Reference-pinned fixture of the Sobolev objective:
  tests/golden/hsloss.npz   for the grids 5 x 7 (odd / odd) and 6 x 9 (even / odd), B 3, 2 channels: seeded fp32 preds (carrying the mask),
                            label and a 0/1 mask, and in fp64 the value and the autograd gradient with respect to preds of the reference's
                            HsLoss(d=2, p=2, k, a, group)(preds, label * mask) (src/models/fno/utilities3.py), both tensors permuted to the
                            channels-last layout that class takes, for (k, a, group) = (1, [1], False), (2, [0.5, 0.25], False),
                            (2, [1, 1], True).  Keys: {grid}_preds / _label / _mask, {grid}_{case}_value / _grad; meta.
The reference forms its weight tensor in torch's DEFAULT dtype: under the default float32 its fp64 result is off by about 1e-8.  This tool
therefore calls torch.set_default_dtype(torch.float64) before it evaluates the class; the fixture is the fp64 definition.
tests/test_cpu_sobolev.py holds tests/sobolev_checks.reference to it.  Writes the fixture only (data, no program text).  Run from the
repository root where the reference sources are present (oracle/make_golden.py finds them):
    python tools/make_golden_hsloss.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

import oracle.make_golden  # noqa: E402,F401  (puts the reference's src on the path)
from models.fno.utilities3 import HsLoss  # noqa: E402  (the reference's module)

OUT = REPO / "tests" / "golden"
B, CO, SEED = 3, 2, 21
GRIDS = ((5, 7), (6, 9))
CASES = {"k1": (1, [1.0], False), "k2": (2, [0.5, 0.25], False), "k2_grouped": (2, [1.0, 1.0], True)}


def main():
    torch.set_default_dtype(torch.float64)  # (module docstring: the reference's weight tensor takes the default dtype)
    out = dict(meta=np.array([B, CO, SEED] + [n for g in GRIDS for n in g]))
    for H, W in GRIDS:
        rng = np.random.default_rng(SEED + 100 * H + W)
        mask = (rng.random((B, 1, H, W)) > 0.2).astype(np.float32)
        preds = (rng.standard_normal((B, CO, H, W)).astype(np.float32) * mask).astype(np.float32)
        label = (rng.standard_normal((B, CO, H, W)) * (1.0 + np.arange(B)[:, None, None, None])).astype(np.float32)
        grid = f"g{H}x{W}"
        out.update({f"{grid}_preds": preds, f"{grid}_label": label, f"{grid}_mask": mask})
        for name, (k, a, group) in CASES.items():
            x = torch.from_numpy(preds.astype(np.float64)).requires_grad_(True)
            y = torch.from_numpy(label.astype(np.float64)) * torch.from_numpy(mask.astype(np.float64))
            value = HsLoss(d=2, p=2, k=k, a=a, group=group)(x.permute(0, 2, 3, 1).contiguous(), y.permute(0, 2, 3, 1).contiguous())
            value.backward()
            out[f"{grid}_{name}_value"] = np.float64(value.item())
            out[f"{grid}_{name}_grad"] = x.grad.numpy().copy()
            print(grid, name, value.item())
    np.savez(OUT / "hsloss.npz", **out)
    print(OUT / "hsloss.npz")


if __name__ == "__main__":
    main()
