"""Reference-pinned fixtures of the FNO with domain padding (Fno2d(padding=p), src/models/fno/fno2d.py:219-226): writes
tests/golden/fno_pad8_64x64.npz (64 x 64, padding 8: the blocks on 72 x 72) and tests/golden/fno_pad9_66x65.npz (66 x 65, padding 9: 75 x 74)
-- predictions, the four losses, the input gradient and gradient summaries of a B 2, width 8, 2-layer model at modes (12, 12) with a border
mask.  oracle/make_golden.py's model generator builds the reference without padding; the one here is it with `padding` as an argument.  Run
from the repository root where the reference sources are present:
    python tools/make_golden_pad.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from oracle import synth  # noqa: E402
from oracle.make_golden import OUT, Fno2d, MseLoss, _t, summarize  # noqa: E402


def gen_fno_pad(name, pseed, bseed, B, C, L, H, W, pad, m1=12, m2=12, p=5, border=True, gain=4.0):
    """oracle.make_golden.gen_fno(..., full_grads=False) with Fno2d(padding=pad); meta gains the mode counts and the padding."""
    params = synth.make_fno_params(pseed, C, L, m1, m2, p, spectral_gain=gain)
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=border)
    model = Fno2d(2, 2, p, MseLoss(normalize=True), L, m1, m2, C, padding=pad)
    model.load_state_dict({k: _t(v) for k, v in params.items()})
    tb = {k: _t(v) for k, v in batch.items()}
    tb["inputs"].requires_grad_(True)
    out = model(**tb)
    out["loss"]["nmse"].backward()
    save = dict(meta=np.array([pseed, bseed, B, C, L, H, W, p, int(border), m1, m2, pad]), gain=np.array(gain),
                preds=out["preds"].detach().numpy(), g_inputs=tb["inputs"].grad.numpy(),
                **{f"loss_{k}": v.detach().numpy() for k, v in out["loss"].items()})
    for k, prm in model.named_parameters():
        for kk, vv in summarize(prm.grad.numpy(), 7).items():
            save[f"gsum::{k}::{kk}"] = vv
    np.savez_compressed(OUT / f"{name}.npz", **save)
    print(name, "ok", {k: float(v) for k, v in out["loss"].items()})


if __name__ == "__main__":
    gen_fno_pad("fno_pad8_64x64", 101, 102, 2, 8, 2, 64, 64, 8)
    gen_fno_pad("fno_pad9_66x65", 103, 104, 2, 8, 2, 66, 65, 9)
