"""Reference-pinned fixture of the FNO at three input and three output channels: writes tests/golden/fno_c3_64x64.npz -- predictions,
the four losses and sampled gradient entries (oracle/synth.py: summarize) of the reference's own Fno2d(in_chan=3, out_chan=3, ...) run on
the CPU on the seeded weights and batch of tests/chan_checks.py.  Run from the repository root where the reference sources are present
(oracle/make_golden.py finds them):
    python tools/make_golden_chan.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle import synth  # noqa: E402
from oracle.make_golden import Fno2d, MseLoss, _t  # noqa: E402  (the reference's modules)
from tests.chan_checks import make_batch, make_params  # noqa: E402


def gen_fno_chan(name, pseed, bseed, B, C, L, H, W, cin, cout, p=5, border=True, gain=4.0):
    params = make_params(pseed, C, L, 12, 12, p, cin, cout, gain)
    batch = make_batch(bseed, B, H, W, p, cin, cout, border)
    model = Fno2d(cin, cout, p, MseLoss(normalize=True), L, 12, 12, C)
    model.load_state_dict({k: _t(v) for k, v in params.items()})
    out = model(**{k: _t(v) for k, v in batch.items()})
    out["loss"]["nmse"].backward()
    save = dict(meta=np.array([pseed, bseed, B, C, L, H, W, p, int(border), cin, cout]), gain=np.array(gain),
                preds=out["preds"].detach().numpy(), **{f"loss_{k}": v.detach().numpy() for k, v in out["loss"].items()})
    for k, prm in model.named_parameters():
        for kk, vv in synth.summarize(prm.grad.numpy(), 7).items():
            save[f"gsum::{k}::{kk}"] = vv
    np.savez_compressed(REPO / "tests" / "golden" / f"{name}.npz", **save)
    print(name, "ok", {k: float(v.detach()) for k, v in out["loss"].items()})


if __name__ == "__main__":
    gen_fno_chan("fno_c3_64x64", 95, 96, 2, 20, 2, 64, 64, 3, 3)
