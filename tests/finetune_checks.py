"""Checks of fine-tuning on the fused FNO step: decoupled weight decay inside the optimiser launch (CFD_STEP_DECOUPLED_WD of cfd_fno_adam_step's
`flags`; k_adam_f<VEC, true> in cfdbench_amd/csrc/optim.hip) and whole steps over a TRAINABLE SUBSET at the C ABI -- compact flat buffers,
frozen tensors in storage of their own, their gradients in a sink, a backward pass that stops behind the shallowest trainable tensor
(cfdbench_amd/engine.py: flatten_layout, last_backward_phase, mask_defer_flags).  Used by tests/test_cpu_finetune.py (the rule against
torch.optim.AdamW), tests/test_emul_finetune.py (CPU, SIMT emulator) and tests/test_gpu_finetune.py (MI355X).

The rule (adamw_rule; torch.optim.AdamW, single-tensor path), per element and step t:
    p *= f,  f = fp32(1 - lr * wd)  formed once in double         then Adam with the UNDECAYED gradient g:
    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Tolerances: ADAM_TOL = 1e-9 is what the flat Adam holds against oracle.adam_step (tests/test_emul_kernels.py, tests/clip_checks.py: moments
and parameter deltas, rel_nmse); the gradient of a step against the fp64 oracle holds 1e-11, 1e-9 on the head's channel route (out_chan > 2:
tests/test_emul_fno_chan.py).  A parameter delta after two steps is a smooth function of the two gradients (|d update / d g| * |g| <= lr),
so it inherits the gradient's relative error and is held to the Adam bound."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np

from cfdbench_amd._capi import CFD_CLIP_FLOATS, CFD_STEP_DECOUPLED_WD, FnoParams
from cfdbench_amd.engine import last_backward_phase, mask_defer_flags, match_prefixes
from oracle import fno_oracle as O
from tests import accum_checks as AC
from tests import chan_checks as CK
from tests import clip_checks as CC
from tests import fno_checks as F
from tests.backends import POISON_WORD, poison

f64, c128, f32 = np.float64, np.complex128, np.float32
DW = CFD_STEP_DECOUPLED_WD
ADAM_TOL = CC.ADAM_TOL
GRAD_TOL, GRAD_TOL_CHAN = 1e-11, 1e-9
LR, B1, B2, EPS, WD = float(f32(1e-3)), float(f32(0.9)), float(f32(0.999)), float(f32(1e-8)), float(f32(0.1))  # (what the fp32 ABI receives)
FLAT_NS = (1, 3, 4, 5, 1027)
same_bits, _bits = CC.same_bits, CC._bits
_DATA = {}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def adamw_rule(p, g, m, v, step, lr=LR, b1=B1, b2=B2, eps=EPS, wd=WD, round_factor=True):
    """In place, fp64 arrays.  round_factor: the factor 1 - lr * wd rounded to fp32 (what a float32 tensor's mul_ by a Python scalar sees);
    False keeps the double, which is torch.optim.AdamW on float64 tensors."""
    fac = 1.0 - float(lr) * float(wd)
    p *= float(f32(fac)) if round_factor else fac
    m *= b1
    m += (1 - b1) * g
    v *= b2
    v += (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** step) + eps
    p -= (lr / (1 - b1 ** step)) * m / denom


def flat_case(n, seed=11):
    """(p0, [g1, g2, g3]) of n floats: parameters 0.1 * N(0, 1) -- their fp32 rounding stays well below a 1e-3 step, as for the weights of
    a model -- and gradients over seven decades, as tests/kernel_checks.py's Adam check draws them."""
    rng = np.random.default_rng(seed + n)
    p0 = (0.1 * rng.standard_normal(n)).astype(f32)
    gs = [(rng.standard_normal(n).astype(f32) * (10.0 ** rng.integers(-6, 1, size=n))).astype(f32) for _ in range(3)]
    return p0, gs


# ---- 1. the bit on a bare flat buffer (flags = 0 besides it) --------------------------------------------------------------------------
def check_adamw_flat(be, misalign, clip, ns=FLAT_NS):
    """cfd_fno_adam_step on flat buffers of n floats, three steps, structs that point nowhere (flags = 0: nothing of them is read but
    grads->clip).  Per n: (a) the bit with wd != 0 against adamw_rule -- with `clip` the gradient the rule sees is clip_rule's, at half the
    measured norm; (b) the bit with wd = 0 is bitwise the call without it; (c) without the bit, wd != 0 is the coupled form: against
    oracle.adam_step, and without clip bitwise cfd_adam_flat.  Returns {n: figures}."""
    res = {}
    with AC.Rig(be, "job_mae", flags=0) as r:
        place = (lambda: be.misaligned(4)) if misalign else contextlib.nullcontext
        P = be.ptr

        def run(n, p0, gs, flags, wd, max_norms):
            with place():
                p, m, v = be.dev(p0), be.dev(np.zeros(n, f32)), be.dev(np.zeros(n, f32))
            clips = []
            for step, g in enumerate(gs, 1):
                with place():
                    dg = be.dev(g)
                    cb = be.out((CFD_CLIP_FLOATS,)) if clip else None
                gstruct = FnoParams()
                if clip:
                    gstruct.clip, gstruct.max_grad_norm = P(cb), float(max_norms[step - 1])
                r.step_call(0, FnoParams(), gstruct, p, dg, m, v, flags, 1.0, step=step, n=n, hyper=(LR, B1, B2, EPS, wd))
                assert same_bits(be.host(dg), g), "the optimiser call changed the gradient buffer"
                clips.append(None if cb is None else be.host(cb)[:2].copy())
            return be.host(p).copy(), be.host(m).copy(), be.host(v).copy(), clips

        for n in ns:
            p0, gs = flat_case(n)
            # thresholds that bite: half of each step's own norm
            max_norms = [float(f32(0.5 * np.sqrt(np.sum(g.astype(f64) ** 2)))) for g in gs]
            got = run(n, p0, gs, DW, WD, max_norms)
            p64, m64, v64 = p0.astype(f64), np.zeros(n, f64), np.zeros(n, f64)
            c64 = (p0.astype(f64), np.zeros(n, f64), np.zeros(n, f64))
            for step, g in enumerate(gs, 1):
                g_eff = g.astype(f64)
                if clip:
                    norm, coef, (g_eff,) = CC.clip_rule([g], max_norms[step - 1], 1.0)
                    assert coef < 0.51 and abs(float(got[3][step - 1][1]) - coef) / coef <= CC.CLIP_TOL, (n, step, coef, got[3][step - 1])
                adamw_rule(p64, g_eff, m64, v64, step)
                O.adam_step(c64[0], g_eff, c64[1], c64[2], step, LR, B1, B2, EPS, WD)
            fig = dict(delta=O.rel_nmse(got[0].astype(f64) - p0, p64 - p0), m=O.rel_nmse(got[1], m64), v=O.rel_nmse(got[2], v64))
            # (b) wd = 0: the factor is 1 and the bits are plain Adam's
            zero_bit, zero_plain = run(n, p0, gs, DW, 0.0, max_norms), run(n, p0, gs, 0, 0.0, max_norms)
            for a, b, what in zip(zero_bit[:3], zero_plain[:3], ("parameters", "exp_avg", "exp_avg_sq")):
                assert same_bits(a, b), f"n = {n}: {what} with the bit and weight_decay = 0 differ from plain Adam"
            # (c) without the bit: coupled L2, the call of before the bit
            coupled = run(n, p0, gs, 0, WD, max_norms)
            fig["coupled_delta"] = O.rel_nmse(coupled[0].astype(f64) - p0, c64[0] - p0)
            assert not same_bits(coupled[0], got[0]), f"n = {n}: the bit changed nothing"
            if not clip:
                with place():
                    p, m, v = be.dev(p0), be.dev(np.zeros(n, f32)), be.dev(np.zeros(n, f32))
                    for step, g in enumerate(gs, 1):
                        be.api.call("cfd_adam_flat", P(p), P(be.dev(g)), P(m), P(v), n, LR, B1, B2, EPS, WD, step, 1.0, be.stream)
                be.sync()
                for a, b in zip(coupled[:3], (p, m, v)):
                    assert same_bits(a, be.host(b)), f"n = {n}: without the bit the call is not cfd_adam_flat"
            print("adamw flat", "misaligned" if misalign else "aligned", "clip" if clip else "no clip", n, fig)
            res[n] = fig
    for n, fig in res.items():
        for k, val in fig.items():
            assert val <= ADAM_TOL, (n, k, val, fig)
    return res


# ---- 2. the bit beside the deferral flags, on a shape that honours them ------------------------------------------------------------------
def check_adamw_deferred(be, misalign, clip, name="job_and_deferred_scale", steps=3):
    """Three whole steps of clip_checks' deferring case (64 x 64, C = 20, L = 2, nmse, flags = 7: the normaliser in the scale, the fc0 rows
    finished by the optimiser launch) with the bit: moments after every step and parameter deltas after three against adamw_rule on the
    gradient buffer the call leaves, scaled (and clipped) as clip_checks restates it.  The lifting layer's rows must have been deferred."""
    c = dict(AC.CASES[name], misalign=misalign)
    with AC.Rig(be, name, misalign=misalign) as r:
        zeros = np.zeros(r.numel, f32)
        m, v = r.dev(zeros), r.dev(zeros)
        p64, m64, v64 = r.flat0.astype(f64), np.zeros(r.numel, f64), np.zeros(r.numel, f64)
        res, max_norm = {}, None
        w_off, w_n = r.layout["fc0.weight"]
        for step in range(1, steps + 1):
            r.backward()
            if step == 1:
                assert AC.is_poison(r.host(r.grad)[w_off:w_off + w_n]), "the lifting layer's rows were not left to the optimiser call"
            if clip and max_norm is None:  # half the norm of the first gradient (the rows of fc0 missing: any threshold that bites will do)
                g_ = r.host(r.grad)
                g_[w_off:w_off + w_n] = 0
                b_off, b_n = r.layout["fc0.bias"]
                g_[b_off:b_off + b_n] = 0
                s_ = CC.step_scale(c, r.host(r.sums))
                max_norm = float(f32(0.5 * abs(float(s_)) * np.sqrt(np.sum(g_.astype(f64) ** 2))))
            cb = r.out(CFD_CLIP_FLOATS) if clip else None
            r.step_call(0, r.ps, r.struct(r.grad, cb, max_norm or 0.0), r.flat, r.grad, m, v, r.flags | DW, 1.0, step=step,
                        hyper=(LR, B1, B2, EPS, WD))
            g, s = r.host(r.grad), CC.step_scale(c, r.host(r.sums))
            assert np.isfinite(g).all()
            if clip:
                norm, coef, (g_eff,) = CC.clip_rule([g], max_norm, float(s))
                got = r.host(cb)[:2]
                res[f"norm{step}"], res[f"coef{step}"] = abs(float(got[0]) - norm) / norm, abs(float(got[1]) - coef) / coef
                if step == 1:
                    assert coef < 0.75, coef
            else:
                g_eff = float(s) * g.astype(f64)
            adamw_rule(p64, g_eff, m64, v64, step)
            res[f"m{step}"], res[f"v{step}"] = O.rel_nmse(r.host(m), m64), O.rel_nmse(r.host(v), v64)
        res["delta"] = O.rel_nmse(r.host(r.flat).astype(f64) - r.flat0, p64 - r.flat0)
    print("adamw deferred", "misaligned" if misalign else "aligned", "clip" if clip else "no clip", res)
    for k, val in res.items():
        assert val <= (CC.CLIP_TOL if k[:4] in ("norm", "coef") else ADAM_TOL), (k, val, res)
    return res


# ---- 3. whole steps over a trainable subset ------------------------------------------------------------------------------------------
# name -> shape; each the smallest that reaches its route.  `defers`: the shape is there FOR the deferrals -- the fc0 rows must be left to
# the optimiser launch when fc0 is trainable (the others may or may not defer; the checks hold either way).
SHAPES = {
    "small": dict(B=2, H=16, W=16, C=4, L=2, m1=3, m2=3, P=1, cin=2, cout=2, defers=False),
    "deferring": dict(B=2, H=64, W=64, C=20, L=2, m1=12, m2=12, P=5, cin=2, cout=2, defers=True),
    "wide": dict(B=2, H=16, W=16, C=33, L=2, m1=3, m2=3, P=1, cin=2, cout=2, defers=False),
    "chan": dict(B=2, H=16, W=16, C=4, L=2, m1=3, m2=3, P=1, cin=3, cout=3, defers=False),
}


def subsets(L):
    """name -> state_dict key prefixes of the trainable tensors."""
    return {"head": ["fc1", "fc2"], "last_block_head": [f"blocks.{L - 1}", "fc1", "fc2"], "fc0_head": ["fc0", "fc1", "fc2"],
            "spectral": [f"blocks.{l}.conv0" for l in range(L)]}


def shape_data(shape):
    if shape not in _DATA:
        c = SHAPES[shape]
        _DATA[shape] = (CK.make_params(41, c["C"], c["L"], c["m1"], c["m2"], c["P"], c["cin"], c["cout"], 4.0),
                        CK.make_batch(42, c["B"], c["H"], c["W"], c["P"], c["cin"], c["cout"], border=True))
    return _DATA[shape]


def compact_layout(params, names, trainable):
    """({name: (offset, floats)} of the trainable tensors, total floats, initial buffer): fno_checks.flat_layout over the subset -- ABI
    order, every tensor on a 4-float boundary."""
    layout, off = {}, 0
    for k, t in zip(names, trainable):
        if t:
            n = params[k].size * (2 if np.iscomplexobj(params[k]) else 1)
            layout[k] = (off, n)
            off += (n + 3) // 4 * 4
    flat0 = np.zeros(off, f32)
    for k, (o, n) in layout.items():
        flat0[o:o + n] = F.flat_view(params[k])
    return layout, off, flat0


def oracle_train(params, batches, L, trainable_names, first_grad=None, lr=1e-3, weight_decay=None):
    """One fp64 step per batch of `batches` (forward, nmse, backward; oracle.adam_step on the trainable tensors, or with `weight_decay`
    adamw_rule with an unrounded factor) -> (first gradient, final parameters).  `first_grad`: the first pass's gradient when the caller
    has it already (it runs on the initial weights whatever is trainable)."""
    p64 = {k: v.astype(c128 if np.iscomplexobj(v) else f64) for k, v in params.items()}
    st = {k: (np.zeros(F.flat_view(p64[k]).size, f64), np.zeros(F.flat_view(p64[k]).size, f64)) for k in trainable_names}
    g1 = first_grad
    for step, batch in enumerate(batches, 1):
        if step == 1 and first_grad is not None:
            rg = first_grad
        else:
            b64 = {k: v.astype(f64) for k, v in batch.items()}
            ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
            rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], "nmse"), L)
        if step == 1:
            g1 = rg
        for k in trainable_names:
            flat = F.flat_view(p64[k]).astype(f64)
            if weight_decay is None:
                O.adam_step(flat, F.flat_view(rg[k]).astype(f64), st[k][0], st[k][1], step, lr)
            else:
                adamw_rule(flat, F.flat_view(rg[k]).astype(f64), st[k][0], st[k][1], step, lr, 0.9, 0.999, 1e-8, weight_decay, round_factor=False)
            p64[k] = (flat.reshape(-1, 2) @ np.array([1.0, 1j])).reshape(p64[k].shape) if np.iscomplexobj(p64[k]) else flat.reshape(p64[k].shape)
    return g1, p64


def oracle_steps(shape, trainable_names, steps):
    """oracle_train on a shape's own batch; the first pass's gradient is computed once per shape."""
    params, batch = shape_data(shape)
    g1, p64 = oracle_train(params, [batch] * steps, SHAPES[shape]["L"], trainable_names, _DATA.get(("oracle1", shape)))
    _DATA[("oracle1", shape)] = g1
    return g1, p64


def run_subset_steps(be, shape, subset, steps=2):
    """`steps` fused steps of `shape` with only `subset` trainable, as FnoTrainEngine issues them: the flat parameter / gradient / moment
    buffers hold the trainable tensors only (compact_layout), `params` points at each frozen tensor's own storage and `grads` at a poisoned
    sink for it; cfd_fno_forward_train_f, cfd_fno_backward_phase_f(1 .. last phase), cfd_fno_adam_step with Adam(1e-3) over the compact
    length, flags = mask_defer_flags(7, ...).  Everything sits in hostile memory between guard bands.  Returns a dict of host arrays."""
    c = SHAPES[shape]
    api, P = be.api, be.ptr
    L = c["L"]
    params, batch = shape_data(shape)
    names = F.param_names(L)
    trainable = match_prefixes(names, subsets(L)[subset])
    last = last_backward_phase(trainable, L)
    flags = mask_defer_flags(7, trainable[0], last)
    layout, numel, flat0 = compact_layout(params, names, trainable)
    plan = api.plan_create(c["H"], c["W"], c["m1"], c["m2"])
    try:
        shp = F.fno_shape(batch, L, c["C"], c["H"], c["W"], c["P"], c["m1"], c["m2"], 0)
        sh = ctypes.byref(shp)
        di, dc, dm, dl = (P(be.dev(batch[k])) for k in ("inputs", "case_params", "mask", "label"))
        flat = be.dev(flat0)
        g0 = poison((numel,)).copy()  # hostile where the contract allows: the tensors poisoned, the alignment padding zero
        used = np.zeros(numel, bool)
        for off, n in layout.values():
            used[off:off + n] = True
        g0[~used] = 0.0
        grad, m, v = be.dev(g0), be.zeros((numel,)), be.zeros((numel,))
        frozen = {k: be.dev(params[k]) for k, t in zip(names, trainable) if not t}
        sink = {k: be.out(params[k].shape, np.complex64 if np.iscomplexobj(params[k]) else f32) for k in frozen}
        ps = F._param_struct(lambda k: P(flat) + 4 * layout[k][0] if k in layout else P(frozen[k]), L)
        gs = F._param_struct(lambda k: P(grad) + 4 * layout[k][0] if k in layout else P(sink[k]), L)
        pr, gr = ctypes.byref(ps), ctypes.byref(gs)
        ws = be.scratch(api.size("cfd_fno_workspace_bytes", plan, sh, 1))
        preds, sums, coef = be.out(batch["label"].shape), be.out((4,)), be.out((2,))
        out = dict(layout=layout, numel=numel, flat0=flat0, trainable=trainable, names=names, last=last, flags=flags, calls=[])
        for step in range(1, steps + 1):
            api.call("cfd_fno_forward_train_f", plan, sh, pr, gr, di, dc, dm, dl, P(preds), P(sums), P(coef), P(ws), 1, 1.0, 0, flags, be.stream)
            for phase in range(1, last + 1):
                api.call("cfd_fno_backward_phase_f", plan, sh, pr, gr, di, dc, dm, dl, P(preds), None, P(coef), P(sums), P(ws), phase, 1, 0,
                         flags, be.stream)
            if step == 1 and "fc0.weight" in layout:
                be.sync()
                o, n = layout["fc0.weight"]
                out["stem_deferred"] = bool((_bits(be.host(grad[o:o + n])) == POISON_WORD).all())
            api.call("cfd_fno_adam_step", plan, sh, pr, gr, di, dc, dm, P(sums), P(ws), P(flat), P(grad), P(m), P(v), numel, 1e-3, 0.9, 0.999,
                     1e-8, 0.0, step, 1.0, 1, 0, flags, be.stream)
            be.sync()
            if step == 1:
                out.update(g1=be.host(grad).copy(), sums1=be.host(sums).copy())
        out.update(flat=be.host(flat).copy(), m=be.host(m).copy(), v=be.host(v).copy(),
                   frozen={k: be.host(t).copy() for k, t in frozen.items()})
        return out
    finally:
        api.plan_destroy(plan)


def check_subset(be, shape, subset, steps=2):
    c = SHAPES[shape]
    params, _ = shape_data(shape)
    run = run_subset_steps(be, shape, subset, steps)
    layout, names = run["layout"], run["names"]
    tnames = [k for k, t in zip(names, run["trainable"]) if t]
    # frozen tensors: bit for bit what they were (nothing steps them, and no gradient lands in them)
    for k, got in run["frozen"].items():
        assert same_bits(got, params[k]), f"{shape}/{subset}: the frozen tensor {k} changed"
    assert len(run["frozen"]) + len(tnames) == len(names) and run["numel"] == sum((n + 3) // 4 * 4 for _, n in layout.values())
    assert run["m"].size == run["numel"] and run["v"].size == run["numel"]
    if "fc0.weight" in layout and c["defers"]:  # the shape's claim about its route: the fc0 rows were left to the optimiser launch
        assert run["stem_deferred"], f"{shape}: the route did not defer the lifting layer's rows"
    g1, p64 = oracle_steps(shape, tnames, steps)
    # where the normaliser is deferred (nmse, narrow, two output channels) the buffer lacks n / sum (label * mask)^2
    unit = float(f32(run["sums1"][3]) / f32(run["sums1"][2])) if (c["C"] <= 32 and c["cout"] <= 2) else 1.0
    gtol = GRAD_TOL_CHAN if c["cout"] > 2 else GRAD_TOL
    res = {}
    for k in tnames:
        res["g:" + k] = O.rel_nmse(F.flat_slice(run["g1"], layout, k).astype(f64) * unit, F.flat_view(g1[k]))
    got = np.concatenate([F.flat_slice(run["flat"], layout, k).astype(f64) - F.flat_view(params[k]) for k in tnames])
    want = np.concatenate([F.flat_view(p64[k]) - F.flat_view(params[k]).astype(f64) for k in tnames])
    res["delta"] = O.rel_nmse(got, want)
    assert np.any(got != 0.0)
    print(shape, subset, "last phase", run["last"], "flags", run["flags"], {k: v for k, v in res.items()})
    for k, val in res.items():
        assert val <= (ADAM_TOL if k == "delta" else gtol), (shape, subset, k, val, res)
    return res
