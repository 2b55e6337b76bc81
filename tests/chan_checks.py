"""Parity checks of the FNO at channel counts other than 2 / 2: the projection head's channel route (out_chan 3 .. 8,
cfdbench_amd/csrc/head.hip k_head_fwd_co / k_head_bwd_co, and the generalised wide head of wide.hip) and the lifting layer at
in_chan 1 and 3 .. 8.  The helpers of tests/kernel_checks.py fix both counts at 2; these are their channel-generic forms, on the same
seeding scheme and against the same fp64 oracle.  Used by tests/test_emul_fno_chan.py (CPU, SIMT emulator) and
tests/test_gpu_fno_chan.py (MI355X)."""
from __future__ import annotations

import ctypes

import numpy as np

from cfdbench_amd._capi import CfdError, FnoShape
from oracle import fno_oracle as O
from oracle import synth
from tests import fno_checks as F
from tests import kernel_checks as K
from tests.backends import POISON_WORD

f64, c128 = np.float64, np.complex128
nm = K.nm
WHICH = {"mse": 0, "nmse": 1, "mae": 2}


def make_params(seed, C, L, m1=12, m2=12, p=5, cin=2, cout=2, spectral_gain=1.0):
    """synth.make_fno_params for any in_chan / out_chan (the same distributions, one NumPy stream in state_dict order)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, (shape, is_c) in synth.fno_param_shapes(C, L, m1, m2, p, cin, cout).items():
        if is_c:
            scale = spectral_gain / (shape[0] * shape[1])
            re = rng.random(shape)
            im = rng.random(shape)
            out[name] = (scale * (re + 1j * im)).astype(np.complex64)
        else:
            fan_in = shape[1] if len(shape) == 4 else out[name.replace("bias", "weight")].shape[1]
            bound = 1.0 / np.sqrt(fan_in)
            out[name] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


def make_batch(seed, B, H, W, p=5, cin=2, cout=2, border=False):
    """synth.make_batch for any channel counts: the label is the leading inputs (cyclically, where cout > cin) plus noise."""
    rng = np.random.default_rng(seed)
    inputs = rng.standard_normal((B, cin, H, W))
    label = inputs[:, np.arange(cout) % cin] + 0.1 * rng.standard_normal((B, cout, H, W))
    case_params = rng.standard_normal((B, p))
    mask = np.ones((B, 1, H, W))
    if border:
        mask[:, :, 0, :] = 0
        mask[:, :, -1, :] = 0
        mask[:, :, :, 0] = 0
    f32 = np.float32
    return dict(inputs=inputs.astype(f32), label=label.astype(f32), case_params=case_params.astype(f32), mask=mask.astype(f32))


def _to64(params, batch):
    p64 = {k: v.astype(c128 if np.iscomplexobj(v) else f64) for k, v in params.items()}
    return p64, {k: v.astype(f64) for k, v in batch.items()}


def _head_inputs(rng, B, C, Co, HW, border):
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
    return a, mask, label, w1, b1, w2, b2


def _head_grads_ref(A, M, z1, h, a1, w1, w2, graw, act):
    ga1 = np.einsum("cj,bcp->bjp", w2.astype(f64), graw)
    gz = ga1 * O.gelu_grad(z1)
    gh = np.einsum("ji,bjp->bip", w1.astype(f64), gz)
    return dict(ga=gh * O.gelu_grad(A) if act else gh, gw1=np.einsum("bjp,bip->ji", gz, h), gb1=gz.sum(axis=(0, 2)),
                gw2=np.einsum("bcp,bjp->cj", graw, a1), gb2=graw.sum(axis=(0, 2)))


def check_head(be, B, C, HW, act, Co, which="nmse", with_ext=False, label_loss=True, border=True, seed=4):
    """cfd_fno_head_fwd + cfd_loss_coef + cfd_fno_head_bwd at Co output channels (K.check_head fixes 2).  label_loss = False: the
    backward gets an external upstream gradient INSTEAD of a label."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    Hd = 128
    a, mask, label, w1, b1, w2, b2 = _head_inputs(rng, B, C, Co, HW, border)
    gext = rng.standard_normal((B, Co, HW)).astype(np.float32) if (with_ext or not label_loss) else None
    A, M, Lb = a.astype(f64), mask.astype(f64), label.astype(f64)
    h, z1, a1, preds_ref = K._head_ref(A, M, Lb, w1.astype(f64), b1.astype(f64), w2.astype(f64), b2.astype(f64), act)
    lab_m = Lb * M
    res = {}
    da, dm, dl = be.dev(a), be.dev(mask), be.dev(label)
    dw1, db1, dw2, db2 = be.dev(w1), be.dev(b1), be.dev(w2), be.dev(b2)
    ws = be.scratch(api.size("cfd_fno_head_workspace_bytes", B, C, Hd, Co, HW))
    preds, sums = be.out((B, Co, HW)), be.out((4,))
    api.call("cfd_fno_head_fwd", P(da), P(dm), P(dl), P(dw1), P(db1), P(dw2), P(db2), P(preds), P(sums), P(ws), B, C, Hd, Co,
             HW, int(act), be.stream)
    be.sync()
    res["preds"] = nm(be.host(preds), preds_ref)
    d = preds_ref - lab_m
    sref = np.array([np.sum(d * d), np.sum(np.abs(d)), np.sum(lab_m * lab_m), d.size])
    res["sums"] = float(np.max(np.abs(be.host(sums) - sref) / np.abs(sref)))
    scores = be.out((4,))
    api.call("cfd_loss_scores", P(sums), P(scores), be.stream)
    be.sync()
    lr = O.mse_loss(preds_ref, lab_m, True)
    sc = be.host(scores)
    res["scores"] = K.nan_max(abs(sc[0] - lr["mse"]) / lr["mse"], abs(sc[1] - lr["rmse"]) / lr["rmse"],
                              abs(sc[2] - lr["mae"]) / lr["mae"], abs(sc[3] - lr["nmse"]) / lr["nmse"])
    coef = be.out((2,))
    api.call("cfd_loss_coef", P(sums), P(coef), WHICH[which], 1.0, be.stream)
    gp = O.loss_grad_wrt_preds(preds_ref, lab_m, which) if label_loss else np.zeros_like(preds_ref)
    if gext is not None:
        gp = gp + gext.astype(f64)
    ref = _head_grads_ref(A, M, z1, h, a1, w1, w2, gp * M, act)
    out = {k: be.out(s) for k, s in dict(ga=(B, C, HW), gw1=(Hd, C), gb1=(Hd,), gw2=(Co, Hd), gb2=(Co,)).items()}
    dgext = be.dev(gext) if gext is not None else None
    api.call("cfd_fno_head_bwd", P(da), P(dm), P(dl) if label_loss else None, P(preds) if label_loss else None, P(dgext),
             P(coef) if label_loss else None, P(dw1), P(db1), P(dw2), P(out["ga"]), P(out["gw1"]), P(out["gb1"]), P(out["gw2"]),
             P(out["gb2"]), P(ws), B, C, Hd, Co, HW, int(act), be.stream)
    be.sync()
    for k in out:
        res[k] = nm(be.host(out[k]), ref[k])
    return res


def check_head_train(be, B, C, HW, act, Co, which="nmse", border=True, seed=14):
    """cfd_label_energy_coef + cfd_fno_head_train at Co output channels (K.check_head_train fixes 2)."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    Hd = 128
    a, mask, label, w1, b1, w2, b2 = _head_inputs(rng, B, C, Co, HW, border)
    A, M, Lb = a.astype(f64), mask.astype(f64), label.astype(f64)
    h, z1, a1, preds_ref = K._head_ref(A, M, Lb, w1.astype(f64), b1.astype(f64), w2.astype(f64), b2.astype(f64), act)
    lab_m = Lb * M
    da, dm, dl = be.dev(a), be.dev(mask), be.dev(label)
    dw1, db1, dw2, db2 = be.dev(w1), be.dev(b1), be.dev(w2), be.dev(b2)
    ws = be.scratch(api.size("cfd_fno_head_workspace_bytes", B, C, Hd, Co, HW))
    wse = be.scratch(api.size("cfd_label_energy_workspace_bytes"))
    preds, sums, coef = be.out((B, Co, HW)), be.out((4,)), be.out((2,))
    out = {k: be.out(s) for k, s in dict(ga=(B, C, HW), gw1=(Hd, C), gb1=(Hd,), gw2=(Co, Hd), gb2=(Co,)).items()}
    api.call("cfd_label_energy_coef", P(dl), P(dm), P(sums), P(coef), P(wse), B, Co, HW, WHICH[which], 1.0, be.stream)
    api.call("cfd_fno_head_train", P(da), P(dm), P(dl), P(coef), P(dw1), P(db1), P(dw2), P(db2), P(preds), P(sums), P(out["ga"]),
             P(out["gw1"]), P(out["gb1"]), P(out["gw2"]), P(out["gb2"]), P(ws), B, C, Hd, Co, HW, int(act), be.stream)
    be.sync()
    res = {"preds": nm(be.host(preds), preds_ref)}
    d = preds_ref - lab_m
    sref = np.array([np.sum(d * d), np.sum(np.abs(d)), np.sum(lab_m * lab_m), d.size])
    res["sums"] = float(np.max(np.abs(be.host(sums) - sref) / np.abs(sref)))
    ref = _head_grads_ref(A, M, z1, h, a1, w1, w2, O.loss_grad_wrt_preds(preds_ref, lab_m, which) * M, act)
    for k in out:
        res[k] = nm(be.host(out[k]), ref[k])
    return res


def check_stem(be, B, H, W, P_, C, cin, border=True, seed=3):
    """cfd_fno_stem_fwd (with and without mask) and cfd_fno_stem_bwd at cin input channels (K.check_stem fixes 2)."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    batch = make_batch(seed, B, H, W, P_, cin, 1, border)
    F = cin + 3 + P_
    w = rng.standard_normal((C, F)).astype(np.float32)
    b = rng.standard_normal((C,)).astype(np.float32)
    g = rng.standard_normal((B, C, H, W)).astype(np.float32)
    plan = api.plan_create(H, W, 12, 12)
    try:
        I64, C64, M64 = (batch[k].astype(f64) for k in ("inputs", "case_params", "mask"))
        feats = O.assemble_features(I64, C64, M64)
        res = {}
        out = be.out((B, C, H, W))
        di, dm, dc = be.dev(batch["inputs"]), be.dev(batch["mask"]), be.dev(batch["case_params"])
        dw, db, dg = be.dev(w), be.dev(b), be.dev(g)
        api.call("cfd_fno_stem_fwd", plan, P(di), P(dm), P(dc), P(dw), P(db), P(out), B, cin, P_, C, be.stream)
        be.sync()
        res["fwd"] = nm(be.host(out), O.conv1x1(feats, w.astype(f64), b.astype(f64)))
        out2 = be.out((B, C, H, W))
        api.call("cfd_fno_stem_fwd", plan, P(di), None, P(dc), P(dw), P(db), P(out2), B, cin, P_, C, be.stream)
        be.sync()
        feats1 = O.assemble_features(I64, C64, np.ones_like(M64))
        res["fwd_nomask"] = nm(be.host(out2), O.conv1x1(feats1, w.astype(f64), b.astype(f64)))
        ws = be.scratch(api.size("cfd_fno_stem_bwd_workspace_bytes", plan, B, cin, P_, C))
        gw, gb = be.out((C, F)), be.out((C,))
        api.call("cfd_fno_stem_bwd", plan, P(dg), P(di), P(dm), P(dc), P(gw), P(gb), P(ws), B, cin, P_, C, be.stream)
        be.sync()
        res["gw"] = nm(be.host(gw), np.einsum("bohw,bihw->oi", g.astype(f64), feats))
        res["gb"] = nm(be.host(gb), g.astype(f64).sum(axis=(0, 2, 3)))
        return res
    finally:
        api.plan_destroy(plan)


def check_fno_vs_oracle(be, B, C, L, H, W, cin, cout, p=5, m1=12, m2=12, border=True, gain=4.0, pseed=7, bseed=8):
    """Whole model: predictions (both workspaces), the four scores and every parameter gradient against the fp64 oracle."""
    params = make_params(pseed, C, L, m1, m2, p, cin, cout, gain)
    batch = make_batch(bseed, B, H, W, p, cin, cout, border)
    out = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2)
    p64, b64 = _to64(params, batch)
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
    rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], "nmse"), L)
    res = {"preds": nm(out["preds"], ref["preds"]), "preds_infer": nm(out["preds_infer"], ref["preds"])}
    lr = ref["loss"]
    res["losses"] = K.nan_max(*(abs(out["scores"][i] - lr[k]) / lr[k] for i, k in enumerate(("mse", "rmse", "mae", "nmse"))))
    for k in params:
        res["g:" + k] = nm(out["grads"][k], rg[k])
    return res


def check_fno_train_step(be, B, C, L, H, W, cin, cout, p=5, which="nmse", flags=7, steps=2, border=True, pseed=27, bseed=28):
    """K.check_fno_train_step_deferred at any channel counts: the fused step (cfd_fno_forward_train_f, the backward phases,
    cfd_fno_adam_step) with `flags` against flags = 0 -- parameters after `steps` steps, predictions, sums, the first gradient -- and
    the first gradient of the flagged run (every tensor) against the oracle."""
    params = make_params(pseed, C, L, 12, 12, p, cin, cout, 4.0)
    batch = make_batch(bseed, B, H, W, p, cin, cout, border)
    # (out_chan > 2 defers nothing: the buffer holds the loss's own gradient whatever the flags say; at out_chan <= 2 the deferred
    # normaliser leaves the gradient of sum d^2 / n, rescaled here as K.check_fno_train_step_deferred does)
    out, layout = F.run_fused_steps(be, params, batch, L, C, H, W, p, which=which, flags=flags, steps=steps)
    for fl, o in out.items():
        if cout <= 2 and (fl & 1) and which == "nmse":
            o["g1"] = o["g1"] * (o["sums1"][3] / o["sums1"][2])
    a, b = out[0], out[flags]
    res = {"params": nm(b["flat"], a["flat"]), "preds": nm(b["preds1"], a["preds1"]), "grad_vs_immediate": nm(b["g1"], a["g1"]),
           "sums": float(np.max(np.abs(b["sums1"] - a["sums1"]) / np.abs(a["sums1"])))}
    p64, b64 = _to64(params, batch)
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
    rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], which), L)
    for k in params:
        for fl in (0, flags):
            res[f"oracle{fl}:" + k] = nm(F.flat_slice(out[fl]["g1"], layout, k), F.flat_view(rg[k]))
    return res


def _still_poisoned(be, buf):
    return bool(np.all(be.host(buf).reshape(-1).view(np.uint32) == POISON_WORD))


def check_refusals(be, C=20, B=1, H=24, W=26, L=1, p=5):
    """out_chan = 9 and bf16 activation storage at out_chan = 3 are refused (CfdError) before any launch: every output buffer still
    holds its poison afterwards (the guard bands are the caller's fixture)."""
    api, P = be.api, be.ptr
    res = {}
    plan = api.plan_create(H, W, 12, 12)
    try:
        for name, cout, dt in (("out_chan9", 9, 0), ("bf16_out_chan3", 3, 1)):
            params = make_params(3, C, L, 12, 12, p, 3, cout)
            batch = make_batch(4, B, H, W, p, 3, cout)
            shape = FnoShape(B, H, W, 3, cout, p, C, L, 12, 12, 128)
            sh = ctypes.byref(shape)
            pd = {k: be.dev(v) for k, v in params.items()}
            gd = {k: be.out(v.shape, np.complex64 if np.iscomplexobj(v) else np.float32) for k, v in params.items()}
            ps, gs = F.make_param_struct(be, pd, L), F.make_param_struct(be, gd, L)
            pr, gr = ctypes.byref(ps), ctypes.byref(gs)
            di, dc, dm, dl = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask", "label"))
            ws = be.scratch(1 << 22)  # (the size functions answer for refused shapes too; any workspace will do: nothing may touch it)
            preds, sums, coef = be.out((B, cout, H, W)), be.out((4,)), be.out((2,))
            calls = {
                "forward": ("cfd_fno_forward_ex", plan, sh, pr, P(di), P(dc), P(dm), None, P(preds), None, P(ws), 0, dt, be.stream),
                "train": ("cfd_fno_forward_train_ex", plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), P(sums), P(coef), P(ws), 1,
                          1.0, dt, be.stream),
            }
            for cname, args in calls.items():
                try:
                    api.call(*args)
                    res[f"{name}:{cname}"] = False
                except CfdError:
                    res[f"{name}:{cname}"] = True
            be.sync()
            bufs = [preds, sums, coef, ws] + list(gd.values())
            res[f"{name}:untouched"] = all(_still_poisoned(be, x) for x in bufs)
        # the head entry points on their own
        rng = np.random.default_rng(5)
        HW = 150
        for name, Co in (("head9", 9),):
            a, mask, label, w1, b1, w2, b2 = _head_inputs(rng, B, C, Co, HW, True)
            dv = [be.dev(x) for x in (a, mask, label, w1, b1, w2, b2)]
            ws, preds, sums = be.scratch(1 << 20), be.out((B, Co, HW)), be.out((4,))
            try:
                api.call("cfd_fno_head_fwd", *(P(x) for x in dv), P(preds), P(sums), P(ws), B, C, 128, Co, HW, 1, be.stream)
                res[name] = False
            except CfdError:
                res[name] = True
            be.sync()
            res[name + ":untouched"] = all(_still_poisoned(be, x) for x in (ws, preds, sums))
        return res
    finally:
        api.plan_destroy(plan)


def case_head(be, ar, B, C=20, Co=4, HW=150, act=1, seed=92):
    """K.check_dirty_reuse case: the head's three entry points at Co output channels on one workspace and one set of outputs."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    Hd = 128
    a, mask, label, w1, b1, w2, b2 = _head_inputs(rng, B, C, Co, HW, True)
    da, dm, dl, dw1, db1, dw2, db2 = (be.dev(x) for x in (a, mask, label, w1, b1, w2, b2))
    ws = ar.scratch(api.size("cfd_fno_head_workspace_bytes", B, C, Hd, Co, HW))
    wse = ar.scratch(api.size("cfd_label_energy_workspace_bytes"))
    preds, sums, coef = ar.out((B, Co, HW)), ar.out((4,)), ar.out((2,))
    g = {k: ar.out(s) for k, s in dict(ga=(B, C, HW), gw1=(Hd, C), gb1=(Hd,), gw2=(Co, Hd), gb2=(Co,)).items()}
    api.call("cfd_fno_head_fwd", P(da), P(dm), P(dl), P(dw1), P(db1), P(dw2), P(db2), P(preds), P(sums), P(ws), B, C, Hd, Co, HW, act,
             be.stream)
    api.call("cfd_loss_coef", P(sums), P(coef), 1, 1.0, be.stream)
    api.call("cfd_fno_head_bwd", P(da), P(dm), P(dl), P(preds), None, P(coef), P(dw1), P(db1), P(dw2), P(g["ga"]), P(g["gw1"]),
             P(g["gb1"]), P(g["gw2"]), P(g["gb2"]), P(ws), B, C, Hd, Co, HW, act, be.stream)
    be.sync()
    res = {"preds": be.host(preds), "sums": be.host(sums), "coef": be.host(coef)}
    res.update({k: be.host(v) for k, v in g.items()})
    preds2, sums2, coef2 = ar.out((B, Co, HW)), ar.out((4,)), ar.out((2,))
    g2 = {k: ar.out(s) for k, s in dict(ga=(B, C, HW), gw1=(Hd, C), gb1=(Hd,), gw2=(Co, Hd), gb2=(Co,)).items()}
    api.call("cfd_label_energy_coef", P(dl), P(dm), P(sums2), P(coef2), P(wse), B, Co, HW, 1, 1.0, be.stream)
    api.call("cfd_fno_head_train", P(da), P(dm), P(dl), P(coef2), P(dw1), P(db1), P(dw2), P(db2), P(preds2), P(sums2), P(g2["ga"]),
             P(g2["gw1"]), P(g2["gb1"]), P(g2["gw2"]), P(g2["gb2"]), P(ws), B, C, Hd, Co, HW, act, be.stream)
    be.sync()
    res.update({"t:preds": be.host(preds2), "t:sums": be.host(sums2), "t:coef": be.host(coef2)})
    res.update({"t:" + k: be.host(v) for k, v in g2.items()})
    return res
