"""Checks of gradient-norm clipping inside the fused FNO step's optimiser call (cfd_fno_params.clip / max_grad_norm of the grads struct, ABI
604; k_gradsq and the clip prologue of k_adam_f in cfdbench_amd/csrc/optim.hip).  Used by tests/test_emul_fno_clip.py (CPU, SIMT
emulator), tests/test_gpu_fno_clip.py (MI355X) and tests/test_cpu_clip.py (the restatement against torch).

The rule, restated in NumPy fp64 (clip_rule; torch.nn.utils.clip_grad_norm_ with norm_type 2):
    norm = |s| * sqrt(sum_i g_i^2)      coef = min(1, max_norm / (norm + 1e-6))      the optimiser sees g_i * (s * coef)
with s the scale the optimiser call applies anyway (grad_scale, times sums[3] / sums[2] where the nMSE normaliser is deferred).

What is compared (check_clipped): at Adam step 1 with zero moments the update is lr * g / (|g| + eps) ~ lr * sign(g), so the PARAMETERS after one
step do not see the coefficient -- the moments are compared after every step, the parameter deltas after three."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from cfdbench_amd._capi import CFD_CLIP_FLOATS, CfdError
from oracle import fno_oracle as O
from oracle import synth
from tests import chan_checks as CK
from tests import fno_checks as F
from tests.backends import POISON_WORD

f64 = np.float64
WHICH = F.WHICH
CLIP_TOL = 2.5e-7   # clip[0], clip[1] against fp64: one fp32 rounding (2^-24) of a double result, times four
ADAM_TOL = 1e-9     # moments and parameter deltas against oracle.adam_step (tests/test_emul_kernels.py holds cfd_adam_flat to it)
LR = 1e-3

# name -> B, C, L, H, W, which, flags, grad_scale, (m1, m2, pad, P = 5 case parameters); each the smallest that reaches its path
CASES = {
    "job_and_deferred_scale": dict(B=2, C=20, L=2, H=64, W=64, which="nmse", flags=7, job=True),   # lifting-layer job in k_gradsq, sums[3]/sums[2] in s
    "job_mae": dict(B=1, C=8, L=1, H=64, W=64, which="mae", flags=7, job=True),                    # the job without the scale deferral
    "flags0_grad_scale": dict(B=2, C=20, L=1, H=64, W=64, which="mse", flags=0, grad_scale=0.5),  # no job, grad_scale inside the norm
    "general_grid": dict(B=1, C=20, L=1, H=66, W=65, which="nmse", flags=7),
    "wide": dict(B=1, C=40, L=1, H=64, W=64, which="mse", flags=7),                       # the wide route defers nothing
    "padded": dict(B=1, C=6, L=1, H=8, W=8, which="nmse", flags=7, m1=2, m2=2, pad=2),    # tests/pad_checks.py's smallest padded shape
    "misaligned": dict(B=2, C=20, L=2, H=64, W=64, which="nmse", flags=7, job=True, misalign=True),  # scalar forms of both kernels
    # hidden 5 with 4 case parameters: fc0.weight is [0, 45), fc0.bias [48, 53) of the flat buffer, so the units of four at 44 and at 52 are
    # half the job's and half the flat walk's (the edge rule of the walk every optimiser kernel shares)
    "odd_ranges": dict(B=1, C=5, L=1, H=64, W=64, which="nmse", flags=7, job=True, P=4),
    "odd_ranges_misaligned": dict(B=1, C=5, L=1, H=64, W=64, which="nmse", flags=7, job=True, P=4, misalign=True),
}
_DATA, _RUNS = {}, {}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def clip_rule(grads, max_norm, scale=1.0):
    """(norm, coef, [scale * coef * g]) in fp64 for a list of real or complex arrays; a complex element counts re^2 + im^2."""
    gs = [np.asarray(g).astype(np.complex128 if np.iscomplexobj(g) else f64) for g in grads]
    sq = sum(float(np.sum(g.real ** 2 + g.imag ** 2)) if np.iscomplexobj(g) else float(np.sum(g * g)) for g in gs)
    norm = abs(float(scale)) * float(np.sqrt(sq))
    coef = min(1.0, float(max_norm) / (norm + 1e-6))
    return norm, coef, [g * (float(scale) * coef) for g in gs]


def scale_defers(c):
    """Whether cfd_fno_adam_step applies sums[3] / sums[2] (include/cfdbench_amd.h, CFD_TRAIN_DEFER_SCALE: nmse on a narrow, unpadded shape)."""
    return bool(c["flags"] & 1) and c["which"] == "nmse" and c["C"] <= 32 and c.get("pad", 0) == 0


def step_scale(c, sums):
    """The fp32 scale s of a step, formed as k_adam_f forms it."""
    s = np.float32(c.get("grad_scale", 1.0))
    if scale_defers(c):
        s = np.float32(s * np.float32(np.float32(sums[3]) / np.float32(sums[2])))
    return s


def case_data(name):
    c = CASES[name]
    key = tuple((k, v) for k, v in sorted(c.items()) if k not in ("misalign", "job"))
    if key not in _DATA:
        m1, m2, p = c.get("m1", 12), c.get("m2", 12), c.get("P", 5)
        if c.get("pad", 0):
            _DATA[key] = (CK.make_params(3, c["C"], c["L"], m1, m2, p), CK.make_batch(4, c["B"], c["H"], c["W"], p, border=True))
        else:
            _DATA[key] = (synth.make_fno_params(27, c["C"], c["L"], m1, m2, p, spectral_gain=4.0),
                          synth.make_batch(28, c["B"], c["H"], c["W"], p, border_mask=True))
    return _DATA[key]


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def same_bits(a, b):
    return bool(np.array_equal(_bits(a), _bits(b)))


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
def run_steps(be, name, max_norm, steps=3, again=0):
    """`steps` fused training steps of case `name` through the C ABI (cfd_fno_forward_train_f, phases 1 .. L + 1, cfd_fno_adam_step with
    Adam(1e-3, 0.9, 0.999, 1e-8)) on hostile memory; max_norm = None: grads->clip = NULL, otherwise a NaN-poisoned clip buffer.  Returns one
    dict per step: flat, m, v, grad (the buffer after the call), sums, clip (the first two floats), job (whether the pass left the fc0 rows
    to the optimiser call).  `again` > 0: after the last step the
    optimiser call is repeated `again` times on copies of that step's parameters and moments with a fresh poisoned clip buffer each;
    the clip pairs come back as the last dict's "again"."""
    c = CASES[name]
    api, P = be.api, be.ptr
    B, C, L, H, W = c["B"], c["C"], c["L"], c["H"], c["W"]
    m1, m2, pad, p = c.get("m1", 12), c.get("m2", 12), c.get("pad", 0), c.get("P", 5)
    wid, flags, gs_ = WHICH[c["which"]], c["flags"], float(c.get("grad_scale", 1.0))
    params, batch = case_data(name)
    layout, numel, flat0 = F.flat_layout(params, L)
    plan = api.plan_create(H + pad, W + pad, m1, m2)
    try:
        shape = F.fno_shape(batch, L, C, H, W, p, m1, m2, pad)
        sh = ctypes.byref(shape)
        di, dc, dm, dl = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask", "label"))

        def placed():  # "misaligned": the flat buffers and clip 4 bytes past a 16-byte boundary (the scalar forms of both kernels)
            return be.misaligned(4) if c.get("misalign") else contextlib.nullcontext()

        def state(flat_h, m_h, v_h):
            with placed():
                return be.dev(flat_h), be.dev(m_h), be.dev(v_h), (be.out((CFD_CLIP_FLOATS,)) if max_norm is not None else None)

        with placed():
            grad = F.flat_grad_buffer(be, layout, numel)
        # cfdbench_amd.h, cfd_adam_flat: the caller zeroes the moments before step 1
        flat, m, v, clip = state(flat0, np.zeros(numel, np.float32), np.zeros(numel, np.float32))
        ws = be.scratch(api.size("cfd_fno_workspace_bytes", plan, sh, 1))
        preds, sums, coef = be.out(batch["label"].shape), be.out((4,)), be.out((2,))

        def structs(flat_, clip_):
            ps, gs = F._flat_struct(be, flat_, layout, L), F._flat_struct(be, grad, layout, L)
            if clip_ is not None:
                gs.clip, gs.max_grad_norm = P(clip_), float(max_norm)
            return ps, gs

        def adam(ps, gs, flat_, m_, v_, step):
            api.call("cfd_fno_adam_step", plan, sh, ctypes.byref(ps), ctypes.byref(gs), P(di), P(dc), P(dm), P(sums), P(ws), P(flat_), P(grad),
                     P(m_), P(v_), numel, LR, 0.9, 0.999, 1e-8, 0.0, step, gs_, wid, 0, flags, be.stream)

        ps, gs = structs(flat, clip)
        pr, gr = ctypes.byref(ps), ctypes.byref(gs)
        out = []
        for step in range(1, steps + 1):
            api.call("cfd_fno_forward_train_f", plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), P(sums), P(coef), P(ws), wid, 1.0, 0, flags,
                     be.stream)
            for phase in range(1, L + 2):
                api.call("cfd_fno_backward_phase_f", plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), None, P(coef), P(sums), P(ws), phase,
                         wid, 0, flags, be.stream)
            if step == 1:  # whether the pass left the fc0 rows to the optimiser call (CFD_TRAIN_DEFER_STEM honoured): still poison
                be.sync()
                w_off = layout["fc0.weight"][0]
                deferred = bool((_bits(be.host(grad[w_off:w_off + 4])) == POISON_WORD).all())
            adam(ps, gs, flat, m, v, step)
            be.sync()
            out.append(dict(job=deferred, flat=be.host(flat).copy(), m=be.host(m).copy(), v=be.host(v).copy(), grad=be.host(grad).copy(),
                            sums=be.host(sums).copy(), clip=None if clip is None else be.host(clip)[:2].copy()))
        pairs = []
        for _ in range(again):  # (the workspace still holds the last pass's records: the call redoes the deferred work on the same inputs)
            f2, m2_, v2, clip2 = state(out[-2]["flat"], out[-2]["m"], out[-2]["v"])
            ps2, gs2 = structs(f2, clip2)
            adam(ps2, gs2, f2, m2_, v2, steps)
            be.sync()
            pairs.append(be.host(clip2)[:2].copy())
            assert same_bits(be.host(f2), out[-1]["flat"]), "the repeated optimiser call gives other parameters"
        out[-1]["again"] = pairs
        return out
    finally:
        api.plan_destroy(plan)


def cached_run(be, name, tag, max_norm, **kw):
    """run_steps once per (backend, case, tag); treat the result as read-only."""
    key = (be.name, name, tag)
    if key not in _RUNS:
        _RUNS[key] = run_steps(be, name, max_norm, **kw)
    return _RUNS[key]


def fc0_rows(name, g):
    params, _ = case_data(name)
    layout, _, _ = F.flat_layout(params, CASES[name]["L"])
    return np.concatenate([F.flat_slice(g, layout, "fc0.weight"), F.flat_slice(g, layout, "fc0.bias")])


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def check_coef_one_is_bitwise(be, name, tag, max_norm):
    """(a) / (f): with a threshold that does not bite -- +inf, or a finite one far above the norm -- every step's parameters, moments and
    gradient buffer are bitwise those of the run without `clip`, and clip[1] == 1.  Returns the step-1 norm."""
    base = cached_run(be, name, "none", None)
    run = cached_run(be, name, tag, max_norm)
    for k, (a, b) in enumerate(zip(base, run), 1):
        for key in ("flat", "m", "v", "grad", "sums"):
            assert same_bits(a[key], b[key]), f"{name} step {k}: {key} differs from the call without clip"
        assert float(b["clip"][1]) == 1.0 and np.isfinite(b["clip"][0]) and b["clip"][0] > 0, (name, k, b["clip"])
    return float(run[0]["clip"][0])


def check_clipped(be, name):
    """(b), (c), (d) with max_grad_norm = half the norm measured at step 1.  Returns the figures it asserted on."""
    c = CASES[name]
    base = cached_run(be, name, "none", None)
    norm1 = float(cached_run(be, name, "inf", float("inf"))[0]["clip"][0])
    max_norm = float(np.float32(0.5 * norm1))
    run = cached_run(be, name, "half", max_norm, again=2)
    params, _ = case_data(name)
    _, numel, flat0 = F.flat_layout(params, c["L"])
    p64, m64, v64 = flat0.astype(f64), np.zeros(numel, f64), np.zeros(numel, f64)
    res = {}
    for k, r in enumerate(run, 1):
        s = step_scale(c, r["sums"])
        norm, coef, (g_eff,) = clip_rule([r["grad"]], max_norm, float(s))
        res[f"norm{k}"] = abs(float(r["clip"][0]) - norm) / norm
        res[f"coef{k}"] = abs(float(r["clip"][1]) - coef) / coef
        O.adam_step(p64, g_eff, m64, v64, k, LR)
        res[f"m{k}"], res[f"v{k}"] = O.rel_nmse(r["m"], m64), O.rel_nmse(r["v"], v64)
        if k == 1:
            assert coef < 0.51, (name, coef)  # the threshold bites
            assert r["job"] or not c.get("job"), f"{name}: the lifting layer's rows were not left to the optimiser call"
            # (c) the gradient buffer is left unclipped: step 1 runs on the same parameters as the unclipped step, so every bit agrees
            assert same_bits(r["grad"], base[0]["grad"]), f"{name}: the gradient buffer differs from the unclipped step's"
            assert same_bits(fc0_rows(name, r["grad"]), fc0_rows(name, base[0]["grad"]))
            assert not same_bits(r["m"], base[0]["m"]), f"{name}: the coefficient did not reach Adam"
    res["delta"] = O.rel_nmse(run[-1]["flat"].astype(f64) - flat0, p64 - flat0)
    print(name, "max_grad_norm", max_norm, res)
    for k, val in res.items():
        assert val <= (CLIP_TOL if k[:4] in ("norm", "coef") else ADAM_TOL), (name, k, val, res)
    # (d) two calls give the same bits
    a, b = run[-1]["again"]
    assert same_bits(a, b) and same_bits(a, run[-1]["clip"]), (name, a, b, run[-1]["clip"])
    return res


def check_refusals(be, name="job_mae"):
    """(e) max_grad_norm = 0, -1, NaN with clip set: CFD_ERR_INVALID_ARG before any launch, every output still poison."""
    c = CASES[name]
    api, P = be.api, be.ptr
    params, batch = case_data(name)
    L = c["L"]
    layout, numel, _ = F.flat_layout(params, L)
    plan = api.plan_create(c["H"], c["W"], 12, 12)
    try:
        shape = F.fno_shape(batch, L, c["C"], c["H"], c["W"], 5, 12, 12, 0)
        sh = ctypes.byref(shape)
        di, dc, dm = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask"))
        ws = be.scratch(api.size("cfd_fno_workspace_bytes", plan, sh, 1))
        got = {}
        for bad in (0.0, -1.0, float("nan")):
            flat, grad, m, v = (be.out((numel,)) for _ in range(4))
            clip, sums = be.out((CFD_CLIP_FLOATS,)), be.out((4,))
            ps, gs = F._flat_struct(be, flat, layout, L), F._flat_struct(be, grad, layout, L)
            gs.clip, gs.max_grad_norm = P(clip), bad
            try:
                api.call("cfd_fno_adam_step", plan, sh, ctypes.byref(ps), ctypes.byref(gs), P(di), P(dc), P(dm), P(sums), P(ws), P(flat), P(grad),
                         P(m), P(v), numel, LR, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, WHICH[c["which"]], 0, c["flags"], be.stream)
                status = 0
            except CfdError as e:
                status = int(str(e).split("(status ")[1].split(")")[0])
            be.sync()
            poison = all(bool((_bits(be.host(b)) == POISON_WORD).all()) for b in (flat, grad, m, v, clip, sums))
            got[repr(bad)] = (status, poison)
        return got
    finally:
        api.plan_destroy(plan)


def check_empty(be):
    """n == 0: clip[0] = 0, clip[1] = 1, nothing else touched."""
    c = CASES["job_mae"]
    api, P = be.api, be.ptr
    params, batch = case_data("job_mae")
    L = c["L"]
    layout, numel, flat0 = F.flat_layout(params, L)
    plan = api.plan_create(c["H"], c["W"], 12, 12)
    try:
        shape = F.fno_shape(batch, L, c["C"], c["H"], c["W"], 5, 12, 12, 0)
        sh = ctypes.byref(shape)
        di, dc, dm = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask"))
        ws = be.scratch(api.size("cfd_fno_workspace_bytes", plan, sh, 1))
        flat, grad, m, v = (be.out((numel,)) for _ in range(4))
        clip, sums = be.out((CFD_CLIP_FLOATS,)), be.out((4,))
        ps, gs = F._flat_struct(be, flat, layout, L), F._flat_struct(be, grad, layout, L)
        gs.clip, gs.max_grad_norm = P(clip), 1.0
        api.call("cfd_fno_adam_step", plan, sh, ctypes.byref(ps), ctypes.byref(gs), P(di), P(dc), P(dm), P(sums), P(ws), P(flat), P(grad), P(m), P(v),
                 0, LR, 0.9, 0.999, 1e-8, 0.0, 1, 1.0, 0, 0, 0, be.stream)
        be.sync()
        untouched = all(bool((_bits(be.host(b)) == POISON_WORD).all()) for b in (flat, grad, m, v))
        return be.host(clip)[:2].copy(), untouched
    finally:
        api.plan_destroy(plan)
