"""Parity checks of the FNO's wide-channel route (hidden 33 .. 128, cfdbench_amd/csrc/wide.hip) that the shared helpers of
tests/kernel_checks.py do not reach: the forward-only entry points (1x1 convolution and its input gradient, the lifting
layer, the projection head with its loss sums, the whole-model forward) and the clean refusal of bf16 activation storage.  Used by tests/test_emul_fno_wide.py (CPU, SIMT emulator) and tests/test_gpu_fno_wide.py (MI355X)."""
from __future__ import annotations

import ctypes

import numpy as np

from cfdbench_amd._capi import CfdError, FnoShape
from oracle import fno_oracle as O
from oracle import synth
from tests import fno_checks as F
from tests import kernel_checks as K

f64 = np.float64
nm = K.nm


def check_chanmix_fwd(be, B, Ci, Co, HW, act, seed=2):
    """cfd_chanmix forward (GELU on load with act) and transposed (the input gradient of a 1x1 conv)."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Ci, HW)).astype(np.float32)
    w = rng.standard_normal((Co, Ci)).astype(np.float32)
    b = rng.standard_normal((Co,)).astype(np.float32)
    g = rng.standard_normal((B, Co, HW)).astype(np.float32)
    f = O.gelu(x.astype(f64)) if act else x.astype(f64)
    res = {}
    out = be.out((B, Co, HW))
    dx, dw, db, dg = be.dev(x), be.dev(w), be.dev(b), be.dev(g)
    api.call("cfd_chanmix", P(dx), P(dw), P(db), P(out), B, Ci, Co, HW, int(act), 0, be.stream)
    be.sync()
    res["fwd"] = nm(be.host(out), np.einsum("oi,bip->bop", w.astype(f64), f) + b[None, :, None])
    gin = be.out((B, Ci, HW))
    api.call("cfd_chanmix", P(dg), P(dw), None, P(gin), B, Co, Ci, HW, 0, 1, be.stream)
    be.sync()
    res["bwd_in"] = nm(be.host(gin), np.einsum("oi,bop->bip", w.astype(f64), g.astype(f64)))
    return res


def check_stem_fwd(be, B, H, W, P_, C, border, seed=3):
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    batch = synth.make_batch(seed, B, H, W, P_, border_mask=border)
    F = 2 + 3 + P_
    w = rng.standard_normal((C, F)).astype(np.float32)
    b = rng.standard_normal((C,)).astype(np.float32)
    plan = api.plan_create(H, W, 12, 12)
    try:
        feats = O.assemble_features(batch["inputs"].astype(f64), batch["case_params"].astype(f64), batch["mask"].astype(f64))
        res = {}
        di, dm, dc = (be.dev(batch[k]) for k in ("inputs", "mask", "case_params"))
        dw, db = be.dev(w), be.dev(b)
        out = be.out((B, C, H, W))
        api.call("cfd_fno_stem_fwd", plan, P(di), P(dm), P(dc), P(dw), P(db), P(out), B, 2, P_, C, be.stream)
        be.sync()
        res["fwd"] = nm(be.host(out), O.conv1x1(feats, w.astype(f64), b.astype(f64)))
        out2 = be.out((B, C, H, W))
        api.call("cfd_fno_stem_fwd", plan, P(di), None, P(dc), P(dw), P(db), P(out2), B, 2, P_, C, be.stream)
        be.sync()
        feats1 = O.assemble_features(batch["inputs"].astype(f64), batch["case_params"].astype(f64),
                                     np.ones_like(batch["mask"], dtype=f64))
        res["fwd_nomask"] = nm(be.host(out2), O.conv1x1(feats1, w.astype(f64), b.astype(f64)))
        return res
    finally:
        api.plan_destroy(plan)


def check_head_fwd(be, B, C, HW, act, Co=2, border=True, seed=4):
    """cfd_fno_head_fwd: predictions and the four loss sums."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    Hd = 128
    a = rng.standard_normal((B, C, HW)).astype(np.float32)
    mask = np.ones((B, 1, HW), np.float32)
    if border:
        mask[:, :, ::7] = 0
    label = rng.standard_normal((B, Co, HW)).astype(np.float32)
    w1 = (rng.standard_normal((Hd, C)) / np.sqrt(C)).astype(np.float32)
    b1 = rng.standard_normal((Hd,)).astype(np.float32) * 0.1
    w2 = (rng.standard_normal((Co, Hd)) / np.sqrt(Hd)).astype(np.float32)
    b2 = rng.standard_normal((Co,)).astype(np.float32) * 0.1
    M, Lb = mask.astype(f64), label.astype(f64)
    _, _, _, preds = K._head_ref(a.astype(f64), M, Lb, w1.astype(f64), b1.astype(f64), w2.astype(f64), b2.astype(f64), act)
    d = preds - Lb * M
    ref_sums = np.array([(d * d).sum(), np.abs(d).sum(), ((Lb * M) ** 2).sum(), B * Co * HW])
    dv = {k: be.dev(v) for k, v in dict(a=a, mask=mask, label=label, w1=w1, b1=b1, w2=w2, b2=b2).items()}
    ws = be.scratch(api.size("cfd_fno_head_workspace_bytes", B, C, Hd, Co, HW))
    out, sums = be.out((B, Co, HW)), be.out((4,))
    api.call("cfd_fno_head_fwd", P(dv["a"]), P(dv["mask"]), P(dv["label"]), P(dv["w1"]), P(dv["b1"]), P(dv["w2"]), P(dv["b2"]),
             P(out), P(sums), P(ws), B, C, Hd, Co, HW, int(act), be.stream)
    be.sync()
    hs = be.host(sums)
    res = {"preds": nm(be.host(out), preds)}
    for k in range(3):
        res[f"sum{k}"] = nm(hs[k:k + 1], ref_sums[k:k + 1])
    res["count"] = abs(hs[3] - ref_sums[3])
    out2 = be.out((B, Co, HW))
    api.call("cfd_fno_head_fwd", P(dv["a"]), None, None, P(dv["w1"]), P(dv["b1"]), P(dv["w2"]), P(dv["b2"]), P(out2), None, None,
             B, C, Hd, Co, HW, int(act), be.stream)
    be.sync()
    _, _, _, preds1 = K._head_ref(a.astype(f64), np.ones_like(M), Lb, w1.astype(f64), b1.astype(f64), w2.astype(f64),
                                  b2.astype(f64), act)
    res["preds_nomask"] = nm(be.host(out2), preds1)
    return res


def check_fno_forward_vs_oracle(be, B, C, L, H, W, p=5, border=False, gain=4.0, pseed=7, bseed=8):
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=gain)
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=border)
    out = F.run_fno(be, params, batch, L, C, H, W, p, backward=False)  # (the wide route's backward: K.check_fno_vs_oracle)
    p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else f64) for k, v in params.items()}
    b64 = {k: v.astype(f64) for k, v in batch.items()}
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
    res = {"preds": nm(out["preds"], ref["preds"]), "preds_infer": nm(out["preds_infer"], ref["preds"])}
    d = ref["preds"] - b64["label"] * (b64["mask"][:, None] if b64["mask"].ndim == 3 else b64["mask"])
    res["sum_d2"] = nm(out["sums"][:1], np.array([(d * d).sum()]))
    res["bitwise_infer"] = 0.0 if np.array_equal(out["preds"], out["preds_infer"]) else 1.0
    return res


def refused(be, fn, *args):
    """True iff the call raises CfdError (a clean refusal, no launch)."""
    try:
        be.api.call(fn, *args)
    except CfdError:
        return True
    return False


def check_wide_refusals(be, C=64, B=1, H=64, W=64, L=1, p=5):
    """bf16 activation storage stays at hidden <= 32: above it the inference forward and the training step refuse cleanly."""
    api, P = be.api, be.ptr
    params = synth.make_fno_params(3, C, L, 12, 12, p)
    batch = synth.make_batch(4, B, H, W, p)
    plan = api.plan_create(H, W, 12, 12)
    try:
        shape = FnoShape(B, H, W, 2, 2, p, C, L, 12, 12, 128)
        pd = {k: be.dev(v) for k, v in params.items()}
        gd = {k: be.out(v.shape, np.complex64 if np.iscomplexobj(v) else np.float32) for k, v in params.items()}
        ps, gs = F.make_param_struct(be, pd, L), F.make_param_struct(be, gd, L)
        di, dc, dm, dl = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask", "label"))
        ws = be.scratch(api.size("cfd_fno_workspace_bytes_ex", plan, ctypes.byref(shape), 1, 0))
        preds, sums, coef = be.out((B, 2, H, W)), be.out((4,)), be.out((2,))
        sh, pr, gr = ctypes.byref(shape), ctypes.byref(ps), ctypes.byref(gs)
        return {
            "bf16_forward": refused(be, "cfd_fno_forward_ex", plan, sh, pr, P(di), P(dc), P(dm), None, P(preds), None, P(ws), 0, 1,
                                    be.stream),
            "bf16_train": refused(be, "cfd_fno_forward_train_ex", plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), P(sums),
                                  P(coef), P(ws), 1, 1.0, 1, be.stream),
        }
    finally:
        api.plan_destroy(plan)
