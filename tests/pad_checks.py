"""Checks of the FNO with domain padding (cfd_fno_shape.pad > 0: the reference's Fno2d(padding=p), src/models/fno/fno2d.py:219-226;
cfdbench_amd/csrc/pad.hip and the pad paths of fno.cpp): the padded fp64 oracle, the whole model and the fused training step against it, the
band written on every call, one misaligned run, the crop offset, the refusals.  Used by tests/test_emul_fno_pad.py (CPU, SIMT emulator) and
tests/test_gpu_fno_pad.py (MI355X).

The oracle is a composition of oracle/fno_oracle.py's building blocks only -- conv1x1 on assemble_features, np.pad, [spectral_conv2d_fwd +
conv1x1, gelu] per block on the padded grid, the crop, the head -- and of their adjoints in reverse; the CPU test of
tests/test_emul_fno_pad.py pins it against two fixtures of the reference itself (tools/make_golden_pad.py)."""
from __future__ import annotations

import ctypes

import numpy as np

from cfdbench_amd._capi import CfdError, FnoShape
from oracle import fno_oracle as O
from tests import chan_checks as CK
from tests import fno_checks as F
from tests import kernel_checks as K
from tests.backends import POISON_WORD

nm = K.nm
WHICH = {"mse": 0, "nmse": 1, "mae": 2}

# (H, W, pad, m1, m2): each the smallest that reaches its hazard
SHAPES = [
    (8, 8, 1, 2, 3),         # smallest band, 9 x 9 odd grid
    (12, 10, 5, 8, 7),       # modes valid only on the padded grid (17 x 15)
    (16, 20, 3, 4, 5),       # W a multiple of 4, W + pad not: the vector-form gate
    (60, 60, 4, 12, 12),     # lands on the 64 x 64 plan: every fused kernel and deferral must step aside
    (62, 61, 4, 12, 12),     # lands on 66 x 65: the general fused block
    (64, 64, 8, 12, 12),     # the usual case, 72 rows: the fp32 fall-back transforms
    (70, 76, 12, 12, 12),    # data grid narrow, padded W = 88: the many-modes route
    (120, 120, 8, 12, 12),   # upper edge, 128 x 128
]
DEFERRAL_SHAPES = [SHAPES[3], SHAPES[4]]


# ---- the padded fp64 oracle ----------------------------------------------------------------------------------------------------
def oracle_forward(params, inputs, case_params, mask, label, L, pad):
    """Fno2d(padding=pad).forward (fno2d.py:178-242) from oracle.fno_oracle's pieces; returns preds, loss and what the backward needs."""
    H, W = inputs.shape[2:]
    feats = O.assemble_features(inputs, case_params, mask)
    h = O.conv1x1(feats, params["fc0.weight"], params["fc0.bias"])                 # :217
    h = np.pad(h, [(0, 0), (0, 0), (0, pad), (0, pad)]) if pad else h              # :219-221 (zeros AFTER fc0: no bias in the band)
    acts, pres = [], []
    for l in range(L):                                                             # :223, FnoBlock.forward :106-112
        acts.append(h)
        pre = O.spectral_conv2d_fwd(h, params[f"blocks.{l}.conv0.weights1"], params[f"blocks.{l}.conv0.weights2"]) + O.conv1x1(
            h, params[f"blocks.{l}.w0.weight"], params[f"blocks.{l}.w0.bias"])
        pres.append(pre)
        h = O.gelu(pre)
    hL = h[..., :H, :W] if pad else h                                              # :224-226
    z1 = O.conv1x1(hL, params["fc1.weight"], params["fc1.bias"])
    a1 = O.gelu(z1)
    preds = O.conv1x1(a1, params["fc2.weight"], params["fc2.bias"]) * mask
    out = dict(preds=preds, cache=dict(feats=feats, acts=acts, pres=pres, hL=hL, z1=z1, a1=a1, mask=mask, preds=preds, pad=pad))
    if label is not None:
        out["cache"]["label"] = label * mask
        out["loss"] = O.mse_loss(preds, label * mask, True)
    return out


def oracle_backward(params, cache, gpreds, L, in_chan):
    """Reverse pass of oracle_forward: the adjoint of the crop embeds d loss / d a_L with a zero band, the adjoint of np.pad crops g_0."""
    g = {}
    pad, e = cache["pad"], "bohw,bihw->oi"
    graw = gpreds * cache["mask"]
    w2 = params["fc2.weight"].reshape(params["fc2.weight"].shape[0], -1)
    g["fc2.weight"] = np.einsum(e, graw, cache["a1"], optimize=True).reshape(params["fc2.weight"].shape)
    g["fc2.bias"] = graw.sum(axis=(0, 2, 3))
    gz1 = np.einsum("oi,bohw->bihw", w2, graw, optimize=True) * O.gelu_grad(cache["z1"])
    w1 = params["fc1.weight"].reshape(params["fc1.weight"].shape[0], -1)
    g["fc1.weight"] = np.einsum(e, gz1, cache["hL"], optimize=True).reshape(params["fc1.weight"].shape)
    g["fc1.bias"] = gz1.sum(axis=(0, 2, 3))
    gh = np.einsum("oi,bohw->bihw", w1, gz1, optimize=True)
    if pad:
        gh = np.pad(gh, [(0, 0), (0, 0), (0, pad), (0, pad)])
    for l in reversed(range(L)):
        gpre = gh * O.gelu_grad(cache["pres"][l])
        h_in = cache["acts"][l]
        kw = f"blocks.{l}.w0.weight"
        w0 = params[kw].reshape(params[kw].shape[0], -1)
        g[kw] = np.einsum(e, gpre, h_in, optimize=True).reshape(params[kw].shape)
        g[f"blocks.{l}.w0.bias"] = gpre.sum(axis=(0, 2, 3))
        gx_s, gw1, gw2 = O.spectral_conv2d_bwd(gpre, h_in, params[f"blocks.{l}.conv0.weights1"], params[f"blocks.{l}.conv0.weights2"])
        g[f"blocks.{l}.conv0.weights1"], g[f"blocks.{l}.conv0.weights2"] = gw1, gw2
        gh = gx_s + np.einsum("oi,bohw->bihw", w0, gpre, optimize=True)
    feats = cache["feats"]
    if pad:
        gh = gh[..., :feats.shape[2], :feats.shape[3]]
    g["fc0.weight"] = np.einsum(e, gh, feats, optimize=True).reshape(params["fc0.weight"].shape)
    g["fc0.bias"] = gh.sum(axis=(0, 2, 3))
    w_fc0 = params["fc0.weight"].reshape(params["fc0.weight"].shape[0], -1)
    g["__inputs__"] = np.einsum("oi,bohw->bihw", w_fc0[:, :in_chan], gh, optimize=True)
    return g


def oracle_run(params, batch, L, pad, which="nmse"):
    p64, b64 = CK._to64(params, batch)
    ref = oracle_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L, pad)
    gp = O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], which)
    return ref, oracle_backward(p64, ref["cache"], gp, L, batch["inputs"].shape[1])


def check_oracle_golden(g):
    """The padded oracle in fp64 against a fixture of the reference's Fno2d(padding=pad) (tools/make_golden_pad.py)."""
    from oracle import synth
    pseed, bseed, B, C, L, H, W, p, border, m1, m2, pad = [int(v) for v in g["meta"]]
    params = synth.make_fno_params(pseed, C, L, m1, m2, p, spectral_gain=float(g["gain"]))
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=bool(border))
    ref, rg = oracle_run(params, batch, L, pad)
    res = {"preds": nm(ref["preds"], g["preds"]), "g_inputs": nm(rg["__inputs__"], g["g_inputs"])}
    for k in ("mse", "rmse", "mae", "nmse"):
        res["loss_" + k] = abs(ref["loss"][k] - float(g[f"loss_{k}"])) / abs(float(g[f"loss_{k}"]))
    n = 0
    for key in g.files:
        if key.startswith("gsum::") and key.endswith("::vals"):
            k = key.split("::")[1]
            res["gsum:" + k] = nm(np.ascontiguousarray(rg[k]).reshape(-1)[g[f"gsum::{k}::idx"]], g[key])
            nrm = np.sqrt(np.sum(np.abs(rg[k]) ** 2))
            res["gnorm:" + k] = abs(nrm - abs(g[f"gsum::{k}::norm"])) / nrm
            n += 1
    assert n == len(params)
    return res, pad


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def _shape(B, H, W, cin, cout, p, C, L, m1, m2, pad):
    return FnoShape(B, H, W, cin, cout, p, C, L, m1, m2, 128, pad)


_CASES, _REFS = {}, {}


def _case(B, C, L, H, W, pad, m1, m2, p, cin, cout, gain, pseed, bseed):
    """(params, batch) of a shape, made once per process and shared by the checks (treat as read-only)."""
    key = (B, C, L, H, W, m1, m2, p, cin, cout, gain, pseed, bseed)
    if key not in _CASES:
        _CASES[key] = (CK.make_params(pseed, C, L, m1, m2, p, cin, cout, gain), CK.make_batch(bseed, B, H, W, p, cin, cout, border=True))
    return _CASES[key]


def _reference(case_key, which="nmse"):
    """oracle_run of _case(*case_key), computed once per (case, loss) and shared by the checks (treat as read-only)."""
    if (case_key, which) not in _REFS:
        params, batch = _case(*case_key)
        _REFS[(case_key, which)] = oracle_run(params, batch, case_key[2], case_key[5], which)
    return _REFS[(case_key, which)]


def check_fno_pad_vs_oracle(be, B, C, L, H, W, pad, m1, m2, p=5, cin=2, cout=2, gain=4.0, pseed=7, bseed=8):
    """Whole padded model against the padded oracle: predictions under the training and the inference workspace, the nMSE loss, every
    parameter gradient."""
    key = (B, C, L, H, W, pad, m1, m2, p, cin, cout, gain, pseed, bseed)
    params, batch = _case(*key)
    out = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2, pad)
    ref, rg = _reference(key)
    res = {"preds": nm(out["preds"], ref["preds"]), "preds_infer": nm(out["preds_infer"], ref["preds"])}
    res["nmse_loss"] = abs(out["scores"][3] - ref["loss"]["nmse"]) / ref["loss"]["nmse"]
    for k in params:
        res["g:" + k] = nm(out["grads"][k], rg[k])
    return res


def accept_vs_oracle(res):
    """What check 1 asserts: predictions K.TOL, the loss 1e-5 relative, every parameter gradient 1e-9."""
    res = dict(res)
    assert res.pop("nmse_loss") < 1e-5, res
    for k in ("preds", "preds_infer"):
        v = res.pop(k)
        assert v < K.TOL, (k, v)
    bad = {k: v for k, v in res.items() if not (v < 1e-9)}
    assert not bad, f"gradient parity failures (tol 1e-9): {bad}; all: {res}"


def check_pad_train_step(be, B, C, L, H, W, pad, m1, m2, p=5, cin=2, cout=2, which="mse", flags=7, steps=2, pseed=7, bseed=8):
    """The fused training step (cfd_fno_forward_train_f, phases 1 .. L + 1, cfd_fno_adam_step) on a padded shape with the CFD_TRAIN_DEFER_*
    flags `flags` against flags = 0: a padded shape ignores them, so the two are bitwise equal ("bitwise" == 0.0); the first step's flat
    gradient against the padded oracle."""
    key = (B, C, L, H, W, pad, m1, m2, p, cin, cout, 4.0, pseed, bseed)
    params, batch = _case(*key)
    out, layout = F.run_fused_steps(be, params, batch, L, C, H, W, p, m1, m2, pad, which=which, flags=flags, steps=steps)
    a, b = out[0], out[flags]
    res = {"bitwise": K.nan_max(*[np.max(np.abs(a[k] - b[k])) for k in ("flat", "g1", "sums1", "preds1")])}
    _ref, rg = _reference(key, which)
    for k in layout:
        res["oracle:" + k] = nm(F.flat_slice(b["g1"], layout, k), F.flat_view(rg[k]))
    return res


def _diff(a, b):
    """Largest absolute difference over predictions, scores and every gradient of two run_fno results; NaN if any value is NaN."""
    vals = [np.max(np.abs(a[k] - b[k])) for k in ("preds", "scores")] + [np.max(np.abs(a["grads"][k] - b["grads"][k])) for k in a["grads"]]
    return K.nan_max(*vals)


def check_pad_dirty(be, B, C, L, H, W, pad, m1, m2, p=5, pseed=7, bseed=8):
    """Forward + backward twice on one NaN-poisoned workspace and outputs without re-poisoning: the second result bitwise the first; and a
    run whose workspace held a large finite constant bitwise the same again -- a band that is assumed instead of written shows in either."""
    key = (B, C, L, H, W, pad, m1, m2, p, 2, 2, 4.0, pseed, bseed)
    params, batch = _case(*key)
    first, second = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2, pad, infer=False, repeat=2)
    third = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2, pad, infer=False, ws_fill=3.0e30)
    ref, _rg = _reference(key)
    return {"second_run": _diff(first, second), "finite_fill": _diff(first, third), "preds": nm(first["preds"], ref["preds"])}


def check_pad_misaligned(be, B=1, C=6, L=2, shift=4):
    """Check 1 at (16, 20, 3) with every buffer `shift` bytes past a 16-byte boundary, through tests/align_checks.py's runner (guard bands
    verified there); returns the number of shifted buffers."""
    from tests import align_checks as AC
    H, W, pad, m1, m2 = SHAPES[2]
    row = AC.Row("fno_pad_vs_oracle", check_fno_pad_vs_oracle, (B, C, L, H, W, pad, m1, m2), accept_vs_oracle)
    return AC._run(be, row, shift)


def check_pad_zero_spectral(be, B, C, L, H, W, pad, m1, m2, p=5, pseed=7, bseed=8):
    """With every spectral weight zero the blocks are pointwise and cropping commutes with them: the padded model's predictions equal the
    unpadded model's on the same inputs (plan of the data grid, an 11-field shape).  Independent of the padded oracle; finds a wrong
    interior offset."""
    params, batch = _case(B, C, L, H, W, pad, m1, m2, p, 2, 2, 4.0, pseed, bseed)
    params = {k: (np.zeros_like(v) if "conv0.weights" in k else v) for k, v in params.items()}
    # the unpadded plan takes the modes its own grid admits: the weights are zero, only their shape is read
    padded = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2, pad)
    um1, um2 = min(m1, H // 2), min(m2, W // 2 + 1)
    uparams = {k: (np.zeros(v.shape[:2] + (um1, um2), v.dtype) if "conv0.weights" in k else v) for k, v in params.items()}
    plain = F.run_fno(be, uparams, batch, L, C, H, W, p, um1, um2, 0)
    return {"preds": nm(padded["preds"], plain["preds"]), "preds_infer": nm(padded["preds_infer"], plain["preds_infer"])}


def _still_poisoned(be, bufs):
    return all(bool((be.host(b).reshape(-1).view(np.uint32) == POISON_WORD).all()) for b in bufs)


def check_pad_refusals(be, C=6, L=1, p=5):
    """Every refusal of a padded shape by status, with every output handed over still all poison afterwards, and the accepted edges."""
    api, P = be.api, be.ptr
    res = {}

    def status(fn, *args):
        try:
            api.call(fn, *args)
        except CfdError as e:
            s = str(e)
            return int(s.split("(status ")[1].split(")")[0])
        return 0

    def attempt(name, want, H, W, pad, plan_hw, m1=2, m2=2, act=0):
        """forward_ex, forward_train_f, backward_phase_f and adam_step with shape (H, W, pad) on a plan of grid plan_hw: all four `want`."""
        B = 1
        params = CK.make_params(3, C, L, m1, m2, p)
        batch = CK.make_batch(4, B, max(H, 1), max(W, 1), p, border=False)
        plan = api.plan_create(plan_hw[0], plan_hw[1], m1, m2)
        try:
            shape = _shape(B, H, W, 2, 2, p, C, L, m1, m2, pad)
            sh = ctypes.byref(shape)
            pd = {k: be.dev(v) for k, v in params.items()}
            gd = {k: be.out(v.shape, np.complex64 if np.iscomplexobj(v) else np.float32) for k, v in params.items()}
            pr, gr = ctypes.byref(F.make_param_struct(be, pd, L)), ctypes.byref(F.make_param_struct(be, gd, L))
            di, dc, dm, dl = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask", "label"))
            ws = be.scratch(1 << 20)
            preds, sums, coef = be.out(batch["label"].shape), be.out((4,)), be.out((2,))
            m, v = be.out((16,)), be.out((16,))
            got = [status("cfd_fno_forward_ex", plan, sh, pr, P(di), P(dc), P(dm), None, P(preds), None, P(ws), 0, act, be.stream),
                   status("cfd_fno_forward_train_f", plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), P(sums), P(coef), P(ws), 1, 1.0,
                          act, 0, be.stream),
                   status("cfd_fno_backward_phase_f", plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), None, P(coef), P(sums), P(ws),
                          1, 1, act, 0, be.stream),
                   status("cfd_fno_adam_step", plan, sh, pr, gr, P(di), P(dc), P(dm), P(sums), P(ws), P(gd["fc0.weight"]),
                          P(gd["fc0.weight"]), P(m), P(v), 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 1, act, 0, be.stream)]
            be.sync()
            res[name] = got == [want] * 4 and _still_poisoned(be, [preds, sums, coef, m, v, *gd.values()])
            if not res[name]:
                res[name + ":statuses"] = got
        finally:
            api.plan_destroy(plan)

    INVALID, UNSUPPORTED = -1, -2
    attempt("pad<0", INVALID, 8, 8, -1, (8, 8))
    attempt("pad>0 with H<2", INVALID, 1, 8, 3, (4, 11))
    attempt("pad>0 with W<2", INVALID, 8, 1, 3, (11, 4))
    attempt("plan of the data grid", INVALID, 8, 8, 2, (8, 8))
    attempt("bf16 storage", UNSUPPORTED, 8, 8, 2, (10, 10), act=1)
    res["121x121 + 8 refused at plan creation"] = _plan_refused(be, 129, 129, 12, 12)
    res["120x120 + 8 plan accepted"] = not _plan_refused(be, 128, 128, 12, 12)
    return res


def _plan_refused(be, H, W, m1, m2):
    try:
        plan = be.api.plan_create(H, W, m1, m2)
    except CfdError:
        return True
    be.api.plan_destroy(plan)
    return False


def check_pad_zero_is_unpadded(be, B=1, C=6, L=2, H=16, W=20, m1=4, m2=5, p=5):
    """pad = 0 with an unpadded plan runs and is bitwise the same call through an 11-field FnoShape; cfd_fno_workspace_bytes agrees too."""
    api = be.api
    params, batch = _case(B, C, L, H, W, 0, m1, m2, p, 2, 2, 4.0, 57, 58)
    a = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2, 0)
    out = {}
    plan = api.plan_create(H, W, m1, m2)
    try:
        s11 = FnoShape(B, H, W, 2, 2, p, C, L, m1, m2, 128)
        s12 = FnoShape(B, H, W, 2, 2, p, C, L, m1, m2, 128, 0)
        out["workspace_bytes"] = all(api.size("cfd_fno_workspace_bytes", plan, ctypes.byref(s11), t) ==
                                     api.size("cfd_fno_workspace_bytes", plan, ctypes.byref(s12), t) > 0 for t in (0, 1))
    finally:
        api.plan_destroy(plan)
    b = F.run_fno(be, params, batch, L, C, H, W, p, m1, m2)  # (no pad argument: the route a caller of the 11-field shape takes)
    out["bitwise"] = K.nan_max(_diff(a, b), np.max(np.abs(a["preds_infer"] - b["preds_infer"]))) == 0.0
    return out
