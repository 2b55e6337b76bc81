"""Reference-pinned fixtures of the FNO's many-modes route (modes1 > 15 or modes2 > 16): writes tests/golden/fno_m32x33_64x64.npz (forward,
losses and gradient summaries of a 64 x 64 model at modes (32, 33): every row and the Nyquist column) and tests/golden/spectral_m33_66x65.npz
(one SpectralConv2d forward / backward at 66 x 65, modes (33, 33)).  oracle/make_golden.py's generators run the reference's own modules on
the CPU but build their models at 12 modes; the model generator here is theirs with the modes as arguments.  Run from the repository root
where the reference sources are present:
    python tools/make_golden_modes.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oracle import synth  # noqa: E402
from oracle.make_golden import OUT, _t, build_ref_model, gen_spectral, summarize  # noqa: E402


def gen_fno_modes(name, pseed, bseed, B, C, L, H, W, m1, m2, p=5, border=True, gain=4.0):
    """oracle.make_golden.gen_fno(..., full_grads=False) at modes (m1, m2); meta gains the two mode counts."""
    params = synth.make_fno_params(pseed, C, L, m1, m2, p, spectral_gain=gain)
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=border)
    model = build_ref_model(params, C, L, m1, m2, p)
    tb = {k: _t(v) for k, v in batch.items()}
    tb["inputs"].requires_grad_(True)
    out = model(**tb)
    out["loss"]["nmse"].backward()
    save = dict(meta=np.array([pseed, bseed, B, C, L, H, W, p, int(border), m1, m2]), gain=np.array(gain),
                preds=out["preds"].detach().numpy(), g_inputs=tb["inputs"].grad.numpy(),
                **{f"loss_{k}": v.detach().numpy() for k, v in out["loss"].items()})
    for k, prm in model.named_parameters():
        for kk, vv in summarize(prm.grad.numpy(), 7).items():
            save[f"gsum::{k}::{kk}"] = vv
    np.savez_compressed(OUT / f"{name}.npz", **save)
    print(name, "ok", {k: float(v) for k, v in out["loss"].items()})


if __name__ == "__main__":
    gen_fno_modes("fno_m32x33_64x64", 95, 96, 2, 8, 2, 64, 64, 32, 33)
    gen_spectral("spectral_m33_66x65", 97, 1, 3, 2, 66, 65, 33, 33)
