"""Checks of gradient accumulation over micro-batches in the fused FNO step (CFD_STEP_ACCUMULATE / CFD_STEP_ACCUM_INIT of cfd_fno_adam_step's
`flags`; k_grad_accum in cfdbench_amd/csrc/optim.hip).  Used by tests/test_emul_fno_accum.py (CPU, SIMT emulator) and
tests/test_gpu_fno_accum.py (MI355X).  Everything runs through the C ABI on tests/backends.py's hostile memory.

The rule (include/cfdbench_amd.h): with CFD_STEP_ACCUMULATE the call finishes the pass's gradient as the optimiser call does and then
    acc[i] = s * g[i]  (CFD_STEP_ACCUM_INIT: acc is never read)      or      acc[i] = fmaf(s, g[i], acc[i])
with s = grad_scale, times sums[3] / sums[2] where the nMSE normaliser is deferred, formed in fp32.  The optimiser step on the accumulated
gradient is the call without the two bits, flags = 0, with the accumulator as its gradient buffer.

Shapes: tests/clip_checks.py's CASES (each the smallest that reaches its path), among them "odd_ranges", whose lifting-layer ranges do not
end on a multiple of four floats -- hidden 5 with 4 case parameters: fc0.weight is [0, 45), fc0.bias [48, 53) of the flat buffer, so the
units of four at 44 and at 52 are half the job's and half the flat loop's.

Bounds: one fp32 rounding per element is a relative error of at most 2^-24, i.e. at most 3.6e-15 of relative nMSE (1e-13 asked); a sum of
three such terms rounds three times (1e-12 asked).  Gradients against the fp64 oracle at the bounds the fused step's own tests hold them to:
1e-11 (tests/test_emul_kernels.py::test_fused_train_step_with_deferred_launches), 1e-9 on the padded shape (tests/test_emul_fno_pad.py)."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from cfdbench_amd._capi import CFD_CLIP_FLOATS, CFD_STEP_ACCUM_INIT, CFD_STEP_ACCUMULATE, CfdError
from oracle import fno_oracle as O
from oracle import synth
from tests import chan_checks as CK
from tests import clip_checks as CC
from tests import fno_checks as F
from tests.backends import POISON_WORD

f64, c128 = np.float64, np.complex128
ACC, INIT = CFD_STEP_ACCUMULATE, CFD_STEP_ACCUM_INIT
WHICH = F.WHICH
LR = CC.LR
INIT_TOL = 1e-13   # acc against fp32(s) * g: one rounding per element
SUM_TOL = 1e-12    # acc against the fp64 sum of three terms
GRAD_TOL, GRAD_TOL_PAD = 1e-11, 1e-9
N_MICRO, N_STEPS = 3, 3

# (odd_ranges' misaligned twin is clipping's: here check_misaligned_gives_the_aligned_bits places whole cases off the boundary)
CASES = {k: v for k, v in CC.CASES.items() if k != "odd_ranges_misaligned"}
_DATA, _RUNS = {}, {}

same_bits, _bits = CC.same_bits, CC._bits


def is_poison(a):
    return bool((_bits(a) == POISON_WORD).all())


def case_data(name, k=0):
    """(params, micro-batch k) of a case; k = 0 of a clip_checks case is clip_checks' own batch."""
    c = CASES[name]
    key = (tuple((q, v) for q, v in sorted(c.items()) if q not in ("misalign", "job")), k)
    if key not in _DATA:
        P, m1, m2 = c.get("P", 5), c.get("m1", 12), c.get("m2", 12)
        if c.get("pad", 0):
            _DATA[key] = (CK.make_params(3, c["C"], c["L"], m1, m2, P), CK.make_batch(4 + 10 * k, c["B"], c["H"], c["W"], P, border=True))
        else:
            _DATA[key] = (synth.make_fno_params(27, c["C"], c["L"], m1, m2, P, spectral_gain=4.0),
                          synth.make_batch(28 + 10 * k, c["B"], c["H"], c["W"], P, border_mask=True))
    return _DATA[key]


def oracle_grad(name, k, which):
    """The flat fp64 gradient of micro-batch k's loss, per tensor: {name: flat array}."""
    c = CASES[name]
    key = ("oracle", name if not c.get("misalign") else "job_and_deferred_scale", k, which)
    if key not in _DATA:
        params, batch = case_data(name, k)
        L = c["L"]
        if c.get("pad", 0):
            from tests import pad_checks as PC
            _ref, rg = PC.oracle_run(params, batch, L, c["pad"], which)
        else:
            p64 = {q: v.astype(c128 if np.iscomplexobj(v) else f64) for q, v in params.items()}
            b64 = {q: v.astype(f64) for q, v in batch.items()}
            ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
            rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], which), L)
        _DATA[key] = {q: F.flat_view(rg[q]) for q in F.param_names(L)}
    return _DATA[key]


def scale_of(c, weight, sums):
    """The fp32 scale of an accumulate call, formed as k_adam_f forms its gscale."""
    s = np.float32(weight)
    if CC.scale_defers(c):
        s = np.float32(s * np.float32(np.float32(sums[3]) / np.float32(sums[2])))
    return s


# ---- the rig: one case's buffers and calls ------------------------------------------------------------------------------------------
class Rig:
    """Plan, shape, device copies of `n_batches` micro-batches, flat parameters, the hostile flat gradient buffer, workspace and outputs of
    a case; `over` overrides entries of the case (flags, which).  The flat buffers obey the case's placement ("misaligned": 4 bytes past a
    16-byte boundary -- the scalar forms)."""

    def __init__(self, be, name, n_batches=1, **over):
        self.be, self.name = be, name
        self.c = c = dict(CASES[name], **over)
        self.api = be.api
        self.L, self.P = c["L"], c.get("P", 5)
        m1, m2, pad = c.get("m1", 12), c.get("m2", 12), c.get("pad", 0)
        self.wid, self.flags = WHICH[c["which"]], c["flags"]
        self.params, batch0 = case_data(name, 0)
        self.layout, self.numel, self.flat0 = F.flat_layout(self.params, self.L)
        self.plan = self.api.plan_create(c["H"] + pad, c["W"] + pad, m1, m2)
        self.shape = F.fno_shape(batch0, self.L, c["C"], c["H"], c["W"], self.P, m1, m2, pad)
        self.sh = ctypes.byref(self.shape)
        self.batches = [tuple(be.dev(case_data(name, k)[1][q]) for q in ("inputs", "case_params", "mask", "label")) for k in range(n_batches)]
        with self.placed():
            self.grad = F.flat_grad_buffer(be, self.layout, self.numel)
            self.flat = be.dev(self.flat0)
        self.ws = be.scratch(self.api.size("cfd_fno_workspace_bytes", self.plan, self.sh, 1))
        self.preds, self.sums, self.coef = be.out(batch0["label"].shape), be.out((4,)), be.out((2,))
        self.ps, self.gs = self.struct(self.flat), self.struct(self.grad)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.plan_destroy(self.plan)

    def placed(self):
        return self.be.misaligned(4) if self.c.get("misalign") else contextlib.nullcontext()

    def struct(self, buf, clip=None, max_norm=0.0):
        s = F._flat_struct(self.be, buf, self.layout, self.L)
        if clip is not None:
            s.clip, s.max_grad_norm = self.be.ptr(clip), float(max_norm)
        return s

    def out(self, n=None):
        with self.placed():
            return self.be.out((self.numel if n is None else n,))

    def dev(self, a):
        with self.placed():
            return self.be.dev(a)

    def host(self, a):
        return self.be.host(a).copy()

    def backward(self, k=0):
        """Forward + backward of micro-batch k into the flat gradient buffer (the case's CFD_TRAIN_DEFER_* flags)."""
        P, (di, dc, dm, dl) = self.be.ptr, self.batches[k]
        pr, gr = ctypes.byref(self.ps), ctypes.byref(self.gs)
        self.api.call("cfd_fno_forward_train_f", self.plan, self.sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(self.preds), P(self.sums), P(self.coef),
                      P(self.ws), self.wid, 1.0, 0, self.flags, self.be.stream)
        for phase in range(1, self.L + 2):
            self.api.call("cfd_fno_backward_phase_f", self.plan, self.sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(self.preds), None, P(self.coef),
                          P(self.sums), P(self.ws), phase, self.wid, 0, self.flags, self.be.stream)
        self.be.sync()

    def step_call(self, k, params, grads, param, grad, m, v, flags, grad_scale, step=1, n=None, hyper=(LR, 0.9, 0.999, 1e-8, 0.0)):
        P, (di, dc, dm, _dl) = self.be.ptr, self.batches[k]
        self.api.call("cfd_fno_adam_step", self.plan, self.sh, ctypes.byref(params), ctypes.byref(grads), P(di), P(dc), P(dm), P(self.sums),
                      P(self.ws), P(param), P(grad), P(m), P(v), self.numel if n is None else n, *hyper, step, float(grad_scale), self.wid, 0,
                      flags, self.be.stream)
        self.be.sync()

    def accumulate(self, k, acc, weight, first, m=None, v=None, clip=None, grad=None):
        """The accumulate call behind backward(k): hyper-parameters that would wreck an Adam step, step = 0."""
        grad = self.grad if grad is None else grad
        gs = self.struct(grad, clip, 1.0)
        self.step_call(k, self.struct(acc), gs, acc, grad, m, v, self.flags | ACC | (INIT if first else 0), weight, step=0,
                       hyper=(float("nan"),) * 5)

    def adam(self, k, flat, acc, m, v, step, clip=None, max_norm=0.0):
        """The optimiser step on the accumulated gradient: flags = 0, grad = the accumulator."""
        self.step_call(k, self.struct(flat), self.struct(acc, clip, max_norm), flat, acc, m, v, 0, 1.0, step=step)


# ---- 1. INIT with an exact scale ------------------------------------------------------------------------------------------------------
def check_init_exact(be, name):
    """flags = 0, mse, grad_scale = 1: a poisoned accumulator equals the gradient buffer bit for bit afterwards; the moments are NULL."""
    with Rig(be, name, flags=0, which="mse") as r:
        acc = r.out()
        r.backward()
        g_before = r.host(r.grad)
        r.accumulate(0, acc, 1.0, True)
        g, a = r.host(r.grad), r.host(acc)
        assert np.isfinite(g).all() and np.any(g != 0.0), name
        assert same_bits(g, g_before), f"{name}: the gradient buffer changed although nothing was deferred"
        assert same_bits(a, g), f"{name}: accumulator != gradient with scale 1"


# ---- 2. / 4. INIT with the case's deferrals; nothing else is touched -------------------------------------------------------------------
def check_init_deferred(be, name, weight=1.0 / 3.0):
    c = CASES[name]
    with Rig(be, name) as r:
        acc, m, v, clip = r.out(), r.out(), r.out(), r.out(CFD_CLIP_FLOATS)
        r.backward()
        g_before = r.host(r.grad)
        w_off, w_n = r.layout["fc0.weight"]
        b_off, b_n = r.layout["fc0.bias"]
        deferred = is_poison(g_before[w_off:w_off + w_n]) and is_poison(g_before[b_off:b_off + b_n])
        assert deferred or not c.get("job"), f"{name}: the lifting layer's rows were not left to the optimiser call"
        if not deferred:
            assert np.isfinite(g_before).all(), name
        r.accumulate(0, acc, weight, True, m, v, clip)
        g, a, sums = r.host(r.grad), r.host(acc), r.host(r.sums)
        # (4) nothing else is touched
        for what, buf in (("exp_avg", m), ("exp_avg_sq", v), ("clip", clip)):
            assert is_poison(r.host(buf)), f"{name}: the accumulate call wrote {what}"
        assert same_bits(r.host(r.flat), r.flat0), f"{name}: the weights changed"
        # the gradient buffer afterwards: what the ABI-604 optimiser call leaves on the same pass (the workspace still holds its records)
        g2 = r.dev(g_before)
        f2, m2, v2 = r.dev(r.flat0), r.dev(np.zeros(r.numel, np.float32)), r.dev(np.zeros(r.numel, np.float32))
        r.step_call(0, r.struct(f2), r.struct(g2), f2, g2, m2, v2, r.flags, 1.0)
        g_ref = r.host(g2)
        assert np.isfinite(g).all(), name
        assert same_bits(g, g_ref), f"{name}: the gradient buffer differs from the one the optimiser call leaves"
        rows = np.r_[w_off:w_off + w_n, b_off:b_off + b_n]
        assert same_bits(g[rows], g_ref[rows])
        s = scale_of(c, weight, sums)
        err = O.rel_nmse(a.astype(f64), float(s) * g.astype(f64))
        print(name, "scale", float(s), "acc vs fp32(s) * grad:", err)
        assert err <= INIT_TOL, (name, err)
        return err


# ---- 3. / 5. the sum over micro-batches, then Adam on the accumulator -------------------------------------------------------------------
def run_groups(be, name):
    """N_STEPS optimiser steps of N_MICRO micro-batches with weights 1 / N_MICRO (first INIT, then add), Adam(1e-3) on the accumulator.
    Two optimiser states see the same accumulated gradients: the unclipped one, whose parameters the passes run on, and a clipped one
    (max_grad_norm = half the first step's norm, a NaN-poisoned clip buffer per step).  Returns one dict per step: grads / sums (per
    micro-batch, the buffer after its accumulate call), acc, and flat / m / v / clip of both states; the first dict also has `twice`: the
    add call of micro-batch 1 repeated on a copy of the accumulator."""
    key = (be.name, name)
    if key in _RUNS:
        return _RUNS[key]
    w = 1.0 / N_MICRO
    with Rig(be, name, N_MICRO) as r:
        zeros = np.zeros(r.numel, np.float32)
        acc = r.out()
        state = {"plain": (r.flat, r.dev(zeros), r.dev(zeros)), "clipped": (r.dev(r.flat0), r.dev(zeros), r.dev(zeros))}
        max_norm, out = None, []
        for step in range(1, N_STEPS + 1):
            rec = dict(grads=[], sums=[])
            for k in range(N_MICRO):
                r.backward(k)
                if step == 1 and k == 1:  # (5) the same call on a copy of the accumulator
                    acc2, g2 = r.dev(r.host(acc)), r.dev(r.host(r.grad))
                    r.accumulate(k, acc2, w, False, grad=g2)
                    rec["twice"] = r.host(acc2)
                r.accumulate(k, acc, w, k == 0)
                if "twice" in rec and k == 1:
                    assert same_bits(rec["twice"], r.host(acc)), f"{name}: two accumulate calls on the same operands differ"
                rec["grads"].append(r.host(r.grad))
                rec["sums"].append(r.host(r.sums))
            rec["acc"] = r.host(acc)
            if max_norm is None:
                max_norm = float(np.float32(0.5 * np.sqrt(np.sum(rec["acc"].astype(f64) ** 2))))
            rec["max_norm"] = max_norm
            for tag, (flat, m, v) in state.items():
                clip = r.out(CFD_CLIP_FLOATS) if tag == "clipped" else None
                r.adam(N_MICRO - 1, flat, acc, m, v, step, clip, max_norm)
                rec[tag] = dict(flat=r.host(flat), m=r.host(m), v=r.host(v), clip=None if clip is None else r.host(clip)[:2])
            assert same_bits(r.host(acc), rec["acc"]), f"{name}: the optimiser call changed the accumulator"
            out.append(rec)
        out[0]["flat0"] = r.flat0
    _RUNS[key] = out
    return out


def check_sum_and_adam(be, name):
    c = CASES[name]
    run = run_groups(be, name)
    L = c["L"]
    params, _ = case_data(name)
    layout, numel, flat0 = F.flat_layout(params, L)
    res = {}
    st = {tag: (flat0.astype(f64), np.zeros(numel, f64), np.zeros(numel, f64)) for tag in ("plain", "clipped")}
    for step, rec in enumerate(run, 1):
        want = np.zeros(numel, f64)
        for k, (g, sums) in enumerate(zip(rec["grads"], rec["sums"])):
            want += float(scale_of(c, 1.0 / N_MICRO, sums)) * g.astype(f64)
            if step == 1:  # the passes of step 1 run on the initial weights: each micro-batch's gradient against the fp64 oracle
                ref = oracle_grad(name, k, c["which"])
                unit = float(np.float32(sums[3]) / np.float32(sums[2])) if CC.scale_defers(c) else 1.0
                for q in layout:
                    res[f"oracle{k}:{q}"] = O.rel_nmse(F.flat_slice(g, layout, q).astype(f64) * unit, ref[q])
        res[f"sum{step}"] = O.rel_nmse(rec["acc"].astype(f64), want)
        for tag, (p64, m64, v64) in st.items():
            got = rec[tag]
            if tag == "clipped":
                norm, coef, (g_eff,) = CC.clip_rule([rec["acc"]], rec["max_norm"], 1.0)
                res[f"norm{step}"] = abs(float(got["clip"][0]) - norm) / norm
                res[f"coef{step}"] = abs(float(got["clip"][1]) - coef) / coef
                if step == 1:
                    assert coef < 0.51, (name, coef)  # the threshold bites
            else:
                g_eff = rec["acc"].astype(f64)
            O.adam_step(p64, g_eff, m64, v64, step, LR)
            res[f"{tag}:m{step}"], res[f"{tag}:v{step}"] = O.rel_nmse(got["m"], m64), O.rel_nmse(got["v"], v64)
    for tag, (p64, _m, _v) in st.items():
        res[f"{tag}:delta"] = O.rel_nmse(run[-1][tag]["flat"].astype(f64) - flat0, p64 - flat0)
    assert not same_bits(run[0]["plain"]["m"], run[0]["clipped"]["m"]), f"{name}: the coefficient did not reach Adam"
    print(name, {q: v for q, v in res.items() if not q.startswith("oracle")}, "worst oracle",
          max(v for q, v in res.items() if q.startswith("oracle")))
    gtol = GRAD_TOL_PAD if c.get("pad", 0) else GRAD_TOL
    for q, val in res.items():
        tol = gtol if q.startswith("oracle") else SUM_TOL if q.startswith("sum") else CC.CLIP_TOL if q[:4] in ("norm", "coef") else CC.ADAM_TOL
        assert val <= tol, (name, q, val, tol)
    return res


def check_misaligned_gives_the_aligned_bits(be):
    """(5) the placement 4 bytes off a 16-byte boundary (scalar forms) gives the aligned run's bits: accumulator, parameters and moments."""
    a, b = run_groups(be, "job_and_deferred_scale"), run_groups(be, "misaligned")
    for step, (x, y) in enumerate(zip(a, b), 1):
        assert same_bits(x["acc"], y["acc"]), f"step {step}: accumulator"
        for tag in ("plain", "clipped"):
            for q in ("flat", "m", "v"):
                assert same_bits(x[tag][q], y[tag][q]), (step, tag, q)
        assert same_bits(x["clipped"]["clip"], y["clipped"]["clip"]), step


# ---- 6. refusals, the empty buffer ----------------------------------------------------------------------------------------------------
def check_refusals(be, name="job_mae"):
    """CFD_STEP_ACCUM_INIT without CFD_STEP_ACCUMULATE, and a NULL `param` or `grad` with it: CFD_ERR_INVALID_ARG before any launch, every
    buffer still poison.  No pass has run: workspace, sums and gradient buffer are poison on entry."""
    got = {}
    with Rig(be, name) as r:
        for what in ("init_alone", "null_param", "null_grad"):
            acc, grad, m, v, clip = r.out(), r.out(), r.out(), r.out(), r.out(CFD_CLIP_FLOATS)
            flags = r.flags | (INIT if what == "init_alone" else ACC)
            try:
                r.step_call(0, r.struct(acc), r.struct(grad, clip, 1.0), None if what == "null_param" else acc,
                            None if what == "null_grad" else grad, m, v, flags, 1.0)
                status = 0
            except CfdError as e:
                status = int(str(e).split("(status ")[1].split(")")[0])
            be.sync()
            got[what] = (status, all(is_poison(r.host(b)) for b in (acc, grad, m, v, clip, r.sums)))
    return got


def check_empty(be, name="job_mae"):
    """n == 0: CFD_OK, nothing launched, nothing touched."""
    with Rig(be, name) as r:
        acc, grad = r.out(), r.out()
        r.step_call(0, r.struct(acc), r.struct(grad), acc, grad, None, None, r.flags | ACC | INIT, 1.0, n=0)
        return all(is_poison(r.host(b)) for b in (acc, grad, r.sums))
