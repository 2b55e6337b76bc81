"""Reference-pinned fixtures of the FNO's gradients with respect to its inputs and case parameters, and of training through a rollout:
  tests/golden/fno_ingrad_c3.npz  the reference's Fno2d(in_chan = out_chan = 3, 8 case parameters) on 64 x 64, B 3, width 8, 2 layers: the
                                  four losses, case_params.grad, 512 sampled entries of inputs.grad and sampled parameter gradients (gsum::)
                                  of loss["nmse"].backward()
  tests/golden/fno_unroll3.npz    K = 3 steps through the reference's Fno2d (2 channels, 5 case parameters, B 2, width 8, 2 layers, 64 x 64)
                                  with each prediction fed back as the next input: 512 sampled entries of the three stacked predictions
                                  (K, B, C, H, W), loss = (1/3) sum_k nmse_k, case_params.grad, sampled inputs.grad and parameter gradients
                                  of loss.backward()
Weights and batches are the seeded ones of tests/chan_checks.py, the label frames tests/ingrad_checks.unroll_labels.  Writes fixtures only.
Run from the repository root where the reference sources are present (oracle/make_golden.py finds them):
    python tools/make_golden_ingrad.py"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle import synth  # noqa: E402
from oracle.make_golden import Fno2d, MseLoss, _t  # noqa: E402  (the reference's modules)
from tests.chan_checks import make_batch, make_params  # noqa: E402
from tests.ingrad_checks import unroll_labels  # noqa: E402

OUT = REPO / "tests" / "golden"


def _model(params, cin, p, L, m1, m2, C):
    model = Fno2d(cin, cin, p, MseLoss(normalize=True), L, m1, m2, C)
    model.load_state_dict({k: _t(v) for k, v in params.items()})
    return model


def _leaves(batch):
    tb = {k: _t(v) for k, v in batch.items()}
    tb["inputs"].requires_grad_(True)
    tb["case_params"].requires_grad_(True)
    return tb


def _sampled(name, a, idx_seed, n=512):
    """`n` seeded entries of the flattened array, in the gsum:: style: {name::idx, name::vals}."""
    flat = np.ascontiguousarray(a).reshape(-1)
    idx = np.random.default_rng(idx_seed).integers(0, flat.size, size=n)
    return {f"{name}::idx": idx, f"{name}::vals": flat[idx]}


def _save(name, kind, meta, gain, model, tb, extra):
    save = dict(kind=np.array(kind), meta=np.array(meta), gain=np.array(gain), g_case_params=tb["case_params"].grad.numpy(),
                **_sampled("g_inputs", tb["inputs"].grad.numpy(), 8), **extra)
    for k, prm in model.named_parameters():
        for kk, vv in synth.summarize(prm.grad.numpy(), 7).items():
            save[f"gsum::{k}::{kk}"] = vv
    np.savez_compressed(OUT / f"{name}.npz", **save)


def gen_ingrad(name, pseed, bseed, B, C, L, H, W, cin, p, m1=12, m2=12, border=True, gain=4.0):
    params = make_params(pseed, C, L, m1, m2, p, cin, cin, gain)
    batch = make_batch(bseed, B, H, W, p, cin, cin, border)
    model, tb = _model(params, cin, p, L, m1, m2, C), _leaves(batch)
    out = model(**tb)
    out["loss"]["nmse"].backward()
    _save(name, "ingrad", [pseed, bseed, B, C, L, H, W, p, int(border), m1, m2, 0, cin], gain, model, tb,
          {f"loss_{k}": v.detach().numpy() for k, v in out["loss"].items()})
    print(name, "ok", {k: float(v.detach()) for k, v in out["loss"].items()})


def gen_unroll(name, pseed, bseed, lseed, B, C, L, H, W, cin, p, K, m1=12, m2=12, border=True, gain=4.0):
    params = make_params(pseed, C, L, m1, m2, p, cin, cin, gain)
    batch = make_batch(bseed, B, H, W, p, cin, cin, border)
    labels = unroll_labels(lseed, batch, K)
    model, tb = _model(params, cin, p, L, m1, m2, C), _leaves(batch)
    x, preds, loss = tb["inputs"], [], 0.0
    for k in range(K):
        out = model(inputs=x, case_params=tb["case_params"], mask=tb["mask"], label=_t(labels[k]))
        x = out["preds"]
        preds.append(x)
        loss = loss + out["loss"]["nmse"] / K
    loss.backward()
    _save(name, "unroll", [pseed, bseed, B, C, L, H, W, p, int(border), m1, m2, 0, cin, K, lseed], gain, model, tb,
          dict(loss=loss.detach().numpy(), **_sampled("preds", np.stack([q.detach().numpy() for q in preds]), 9)))
    print(name, "ok", float(loss.detach()))


if __name__ == "__main__":
    gen_ingrad("fno_ingrad_c3", 111, 112, 3, 8, 2, 64, 64, 3, 8)
    gen_unroll("fno_unroll3", 113, 114, 115, 2, 8, 2, 64, 64, 2, 5, 3)
