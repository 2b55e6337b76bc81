"""Checks of skipping non-finite steps inside the fused FNO step's optimiser call (CFD_STEP_SKIP_NONFINITE of cfd_fno_adam_step's `flags`;
k_adam_f<VEC, DW, true> in cfdbench_amd/csrc/optim.hip).  Used by tests/test_emul_fno_guard.py (CPU, SIMT emulator) and
tests/test_gpu_fno_guard.py (MI355X).  Everything runs through the C ABI on tests/backends.py's hostile memory.

The rule (include/cfdbench_amd.h): with the bit, norm = |s| * sqrt(sum_i grad[i]^2) in fp64 -- the quantity clipping defines, s = grad_scale
times the deferred normaliser where it applies.  A norm that is not finite makes the call a SKIPPED STEP: param, exp_avg, exp_avg_sq keep
their bits, the gradient buffer is left as the pass left it (the deferred fc0 rows are still finished into it), clip[0] = the norm,
clip[1] = 0, and the clip buffer's last two floats count: [CFD_CLIP_SKIPPED] += 1, [CFD_CLIP_CONSECUTIVE] += 1; an applied call stores 0
to the latter.  `step` stays the caller's: the bias corrections after a skip are those of t.  With a finite norm the call is bitwise the
call without the bit.

Bounds: the one comparison that is not bitwise (check_sequence) is held to finetune_checks.ADAM_TOL, the bound check_adamw_flat applies
to its own three-step comparison against the same fp64 rule."""
from __future__ import annotations

import contextlib

import numpy as np

from cfdbench_amd._capi import (CFD_CLIP_CONSECUTIVE, CFD_CLIP_FLOATS, CFD_CLIP_SKIPPED, CFD_STEP_ACCUM_INIT, CFD_STEP_ACCUMULATE,
                                CFD_STEP_DECOUPLED_WD, CFD_STEP_SKIP_NONFINITE, CfdError, FnoParams)
from oracle import fno_oracle as O
from tests import accum_checks as AC
from tests import clip_checks as CC
from tests import finetune_checks as FT
from tests import fno_checks as F
from tests.backends import POISON_WORD, poison

f64, f32 = np.float64, np.float32
SKIP, DW, ACC, INIT = CFD_STEP_SKIP_NONFINITE, CFD_STEP_DECOUPLED_WD, CFD_STEP_ACCUMULATE, CFD_STEP_ACCUM_INIT
INF = float("inf")
FLAT_NS = (1, 7, 1028)    # the scalar form (n < 4), an n % 4 tail, the 16-byte form over several threads
FLAT_N_CAPPED = 300003    # 293 workgroups of four floats per thread: k_gradsq runs at its cap of 256 records; n % 4 = 3
BAD_VALUES = (float("nan"), INF, -INF)
HYPER = (FT.LR, FT.B1, FT.B2, FT.EPS, FT.WD)
DEFERRING = "job_and_deferred_scale"  # clip_checks' case: 64 x 64, C = 20, L = 2, nmse, flags = 7
same_bits, _bits, is_poison = CC.same_bits, CC._bits, AC.is_poison


def clip_buffer(skipped=0.0, consecutive=0.0):
    """Host image of a clip buffer as the contract asks for it with the bit: NaN poison, the two counters set by the caller."""
    c = poison((CFD_CLIP_FLOATS,)).copy()
    c[CFD_CLIP_SKIPPED], c[CFD_CLIP_CONSECUTIVE] = skipped, consecutive
    return c


def counters(clip_host):
    return float(clip_host[CFD_CLIP_SKIPPED]), float(clip_host[CFD_CLIP_CONSECUTIVE])


def bad_positions(n):
    """Element 0, the last element, and one inside the n % 4 tail where the 16-byte form has one."""
    pos = {0, n - 1}
    if n >= 4 and n % 4:
        pos.add(n - n % 4 + (n % 4) // 2)
    return sorted(pos)


def _status(call):
    try:
        call()
        return 0
    except CfdError as e:
        return int(str(e).split("(status ")[1].split(")")[0])


def _grad_struct(be, clip, max_norm):
    g = FnoParams()
    if clip is not None:
        g.clip, g.max_grad_norm = be.ptr(clip), float(max_norm)
    return g


def _moments(n, seed=5):
    """Moments of a run under way (exp_avg_sq >= 0): a skipped step must keep every bit of them."""
    rng = np.random.default_rng(seed + n)
    return (1e-2 * rng.standard_normal(n)).astype(f32), (1e-4 * rng.random(n)).astype(f32)


# ---- (a) a non-finite gradient on flat buffers: nothing is written ------------------------------------------------------------------------
def check_skip_flat(be, misalign, ns=FLAT_NS):
    """cfd_fno_adam_step on flat buffers of n floats, structs that point nowhere, flags = the bit (with and without CFD_STEP_DECOUPLED_WD),
    max_grad_norm = +inf and = 1: one NaN / +inf / -inf at element 0, at the last element or in the n % 4 tail, and one call with a finite
    gradient and grad_scale = NaN.  Returns the number of skipped calls it looked at."""
    seen = 0
    with AC.Rig(be, "job_mae", flags=0) as r:
        place = (lambda: be.misaligned(4)) if misalign else contextlib.nullcontext
        for n in ns:
            p0, gs = FT.flat_case(n)
            m0, v0 = _moments(n)
            cases = [(val, pos, 1.0) for val in BAD_VALUES for pos in bad_positions(n)] + [(None, None, float("nan"))]
            for val, pos, scale in cases:
                g0 = gs[0].copy()
                if val is not None:
                    g0[pos] = val
                for flags in (SKIP, SKIP | DW):
                    for max_norm in (INF, 1.0):
                        with place():
                            p, m, v, dg = be.dev(p0), be.dev(m0), be.dev(v0), be.dev(g0)
                            cb = be.dev(clip_buffer(5.0, 2.0))
                        r.step_call(0, FnoParams(), _grad_struct(be, cb, max_norm), p, dg, m, v, flags, scale, step=3, n=n, hyper=HYPER)
                        what = (n, val, pos, scale, flags, max_norm)
                        for name, buf, ref in (("param", p, p0), ("exp_avg", m, m0), ("exp_avg_sq", v, v0), ("grad", dg, g0)):
                            assert same_bits(be.host(buf), ref), f"{what}: a skipped step changed {name}"
                        c = be.host(cb)
                        assert not np.isfinite(c[0]) and _bits(c[1:2])[0] == 0, (what, c[:2])
                        assert counters(c) == (6.0, 3.0), (what, counters(c))
                        seen += 1
    return seen


# ---- (b) finite gradients: the bit changes no bit ------------------------------------------------------------------------------------------
def check_finite_is_bitwise(be, misalign, ns=FLAT_NS):
    """Three steps on flat buffers with `clip` set, with and without the bit (and each with and without CFD_STEP_DECOUPLED_WD, with
    max_grad_norm = +inf and = half each step's norm): parameters, moments, gradient buffer and clip[0..1] agree bit for bit after every
    step; the counters are 0 after every step with the bit and untouched poison without it."""
    with AC.Rig(be, "job_mae", flags=0) as r:
        place = (lambda: be.misaligned(4)) if misalign else contextlib.nullcontext

        def run(n, p0, gs, flags, max_norms):
            with place():
                p, m, v = be.dev(p0), be.dev(np.zeros(n, f32)), be.dev(np.zeros(n, f32))
                cb = be.dev(clip_buffer()) if flags & SKIP else be.out((CFD_CLIP_FLOATS,))
            out = []
            for step, g in enumerate(gs, 1):
                with place():
                    dg = be.dev(g)
                r.step_call(0, FnoParams(), _grad_struct(be, cb, max_norms[step - 1]), p, dg, m, v, flags, 1.0, step=step, n=n, hyper=HYPER)
                out.append(dict(p=be.host(p).copy(), m=be.host(m).copy(), v=be.host(v).copy(), g=be.host(dg).copy(), clip=be.host(cb).copy()))
            return out

        for n in ns:
            p0, gs = FT.flat_case(n)
            half = [float(f32(0.5 * np.sqrt(np.sum(g.astype(f64) ** 2)))) for g in gs]
            for dw in (0, DW):
                for max_norms in ([INF] * 3, half):
                    plain, guarded = run(n, p0, gs, dw, max_norms), run(n, p0, gs, dw | SKIP, max_norms)
                    for step, (a, b) in enumerate(zip(plain, guarded), 1):
                        what = (n, dw, max_norms[0], step)
                        for k in ("p", "m", "v", "g"):
                            assert same_bits(a[k], b[k]), f"{what}: {k} differs between the calls with and without the bit"
                        assert same_bits(a["clip"][:2], b["clip"][:2]) and np.isfinite(b["clip"][:2]).all(), (what, a["clip"][:2], b["clip"][:2])
                        assert (float(b["clip"][1]) < 0.51) == (max_norms[0] != INF), (what, b["clip"][:2])
                        assert counters(b["clip"]) == (0.0, 0.0), (what, counters(b["clip"]))
                        assert is_poison(a["clip"][CFD_CLIP_CONSECUTIVE:]), f"{what}: the call without the bit touched the counters"
                    assert not same_bits(guarded[-1]["p"], p0)


# ---- (c) finite, non-finite, finite ----------------------------------------------------------------------------------------------------------
def check_sequence(be, misalign, ns=FLAT_NS):
    """t = 1, 2, 3 with gradients g1, g2 (one NaN), g3: the result is the fp64 rule applied at t = 1 to g1 and at t = 3 to g3 -- the bias
    corrections of t = 3, not of the second applied step -- with step 2 changing nothing.  AdamW against finetune_checks.adamw_rule,
    coupled Adam against oracle.adam_step.  Returns {(n, flags): figures}."""
    res = {}
    with AC.Rig(be, "job_mae", flags=0) as r:
        place = (lambda: be.misaligned(4)) if misalign else contextlib.nullcontext
        for n in ns:
            p0, gs = FT.flat_case(n)
            gs = [g.copy() for g in gs]
            gs[1][n // 2] = float("nan")
            for dw in (0, DW):
                with place():
                    p, m, v = be.dev(p0), be.dev(np.zeros(n, f32)), be.dev(np.zeros(n, f32))
                    cb = be.dev(clip_buffer())
                p64, m64, v64 = p0.astype(f64), np.zeros(n, f64), np.zeros(n, f64)
                for step, g in enumerate(gs, 1):
                    before = [be.host(b).copy() for b in (p, m, v)]
                    with place():
                        dg = be.dev(g)
                    r.step_call(0, FnoParams(), _grad_struct(be, cb, INF), p, dg, m, v, SKIP | dw, 1.0, step=step, n=n, hyper=HYPER)
                    c = be.host(cb)
                    if step == 2:
                        for b, ref in zip((p, m, v), before):
                            assert same_bits(be.host(b), ref), (n, dw, "the skipped step wrote")
                        assert float(c[1]) == 0.0 and np.isnan(c[0]), c[:2]
                    elif dw:
                        FT.adamw_rule(p64, g.astype(f64), m64, v64, step)
                    else:
                        O.adam_step(p64, g.astype(f64), m64, v64, step, FT.LR, FT.B1, FT.B2, FT.EPS, FT.WD)
                    assert counters(c) == ((0.0, 0.0), (1.0, 1.0), (1.0, 0.0))[step - 1], (n, dw, step, counters(c))
                fig = dict(delta=O.rel_nmse(be.host(p).astype(f64) - p0, p64 - p0), m=O.rel_nmse(be.host(m), m64), v=O.rel_nmse(be.host(v), v64))
                # the same two gradients at t = 1, 2 (a step count that stood still over the skip) are another result, in this measure too
                q64, qm, qv = p0.astype(f64), np.zeros(n, f64), np.zeros(n, f64)
                for step, g in ((1, gs[0]), (2, gs[2])):
                    FT.adamw_rule(q64, g.astype(f64), qm, qv, step) if dw else O.adam_step(q64, g.astype(f64), qm, qv, step, FT.LR, FT.B1, FT.B2,
                                                                                           FT.EPS, FT.WD)
                fig["other_rule"] = O.rel_nmse(q64 - p0, p64 - p0)
                print("guard sequence", "misaligned" if misalign else "aligned", n, "adamw" if dw else "adam", fig)
                res[(n, dw)] = fig
    for key, fig in res.items():
        for k in ("delta", "m", "v"):
            assert fig[k] <= FT.ADAM_TOL, (key, k, fig)
        assert fig["other_rule"] > FT.ADAM_TOL, (key, fig)  # (the comparison tells the two step-count rules apart)
    return res


# ---- (d) whole steps with deferrals ----------------------------------------------------------------------------------------------------------
def bad_label(label, kind):
    """A label that makes the step non-finite: "inf" -- one +inf at an interior point; "zero" -- all zero, so that nMSE's deferred
    normaliser n / sum (label * mask)^2 is inf."""
    bad = np.zeros_like(label) if kind == "zero" else label.copy()
    if kind == "inf":
        bad[0, 0, label.shape[2] // 2, label.shape[3] // 2] = INF
    return bad


def check_deferred_steps(be, kind, misalign=False, name=DEFERRING):
    """Clean batch (t = 1), bad batch (t = 2), clean batch (t = 3) on clip_checks' deferring case with flags = 7 | the bit and
    max_grad_norm = +inf; beside it an UNGUARDED state (flags = 7, no clip buffer at all) takes the two clean steps on the same gradient
    buffers.  The skipped step touches no parameter and no moment, the fc0 rows included, but finishes the fc0 rows of the gradient buffer;
    the steps at t = 1 and t = 3 are bitwise the unguarded state's."""
    with AC.Rig(be, name, misalign=misalign) as r:
        di, dc, dm, dl = r.batches[0]
        r.batches.append((di, dc, dm, be.dev(bad_label(be.host(dl), kind))))
        zeros = np.zeros(r.numel, f32)
        m, v, cb = r.dev(zeros), r.dev(zeros), r.dev(clip_buffer())
        f2, m2, v2 = r.dev(r.flat0), r.dev(zeros), r.dev(zeros)
        rows = np.r_[slice(*np.cumsum(r.layout["fc0.weight"])), slice(*np.cumsum(r.layout["fc0.bias"]))]
        for step, k in ((1, 0), (2, 1), (3, 0)):
            with r.placed():  # a gradient buffer of its own per step, so that the fc0 rows are poison again in front of every optimiser call
                r.grad = F.flat_grad_buffer(be, r.layout, r.numel)
            r.gs, guarded = r.struct(r.grad), r.struct(r.grad, cb, INF)
            r.backward(k)
            g_pass = r.host(r.grad)
            assert is_poison(g_pass[rows]), f"{name}: the lifting layer's rows were not left to the optimiser call"
            before = [r.host(b) for b in (r.flat, m, v)]
            r.step_call(k, r.ps, guarded, r.flat, r.grad, m, v, r.flags | SKIP, 1.0, step=step)
            g, c = r.host(r.grad), r.host(cb)
            assert not (_bits(g[rows]) == POISON_WORD).any(), f"step {step}: the fc0 rows of the gradient buffer were not written"
            keep = np.ones(r.numel, bool)
            keep[rows] = False
            assert same_bits(g[keep], g_pass[keep]), f"step {step}: the optimiser call changed the gradient buffer outside the fc0 rows"
            if k == 1:
                for b, ref, what in zip((r.flat, m, v), before, ("parameters", "exp_avg", "exp_avg_sq")):
                    assert same_bits(r.host(b), ref), f"{kind}: the skipped step changed {what}"
                    assert same_bits(r.host(b)[rows], ref[rows])
                assert not np.isfinite(c[0]) and float(c[1]) == 0.0 and counters(c) == (1.0, 1.0), (kind, c[:2], counters(c))
                if kind == "zero":  # the gradient itself is finite: it is the normaliser that is not
                    assert np.isfinite(g).all() and r.host(r.sums)[2] == 0.0 and r.host(r.sums)[3] > 0.0
                continue
            g2 = r.dev(g_pass)
            r.step_call(k, r.struct(f2), r.struct(g2), f2, g2, m2, v2, r.flags, 1.0, step=step)
            for a, b, what in ((r.flat, f2, "parameters"), (m, m2, "exp_avg"), (v, v2, "exp_avg_sq"), (r.grad, g2, "gradient buffer")):
                assert same_bits(r.host(a), r.host(b)), f"{kind}, t = {step}: {what} differ from the unguarded step's"
            assert np.isfinite(c[:2]).all() and float(c[1]) == 1.0 and counters(c) == ((0.0, 0.0) if step == 1 else (1.0, 0.0)), (step, c[:2])
        assert not same_bits(r.host(r.flat), r.flat0) and np.isfinite(r.host(r.flat)).all()


# ---- (e) the bit beside CFD_STEP_ACCUMULATE ---------------------------------------------------------------------------------------------------
def check_accumulate_ignores_the_bit(be, name=DEFERRING):
    """A pass on a label with one +inf, then the accumulate call with and without the bit on copies of the gradient buffer: accumulator and
    gradient buffer agree bit for bit, NaNs included, and the clip buffer handed along stays poison (no norm is taken there).  The
    optimiser call on that accumulator with the bit is a skip."""
    with AC.Rig(be, name) as r:
        di, dc, dm, dl = r.batches[0]
        r.batches.append((di, dc, dm, be.dev(bad_label(be.host(dl), "inf"))))
        r.backward(1)
        g_pass = r.host(r.grad)
        got = {}
        for bit in (0, SKIP):
            acc, grad, clip = r.out(), r.dev(g_pass), r.out(CFD_CLIP_FLOATS)
            r.step_call(1, r.struct(acc), r.struct(grad, clip, 1.0), acc, grad, None, None, r.flags | ACC | INIT | bit, 0.5, step=0,
                        hyper=(float("nan"),) * 5)
            assert is_poison(r.host(clip)), "the accumulate call touched the clip buffer"
            got[bit] = (r.host(acc), r.host(grad), acc)
        assert same_bits(got[0][0], got[SKIP][0]) and same_bits(got[0][1], got[SKIP][1]), "the bit changed the accumulate call"
        acc_h, acc = got[SKIP][0], got[SKIP][2]
        assert not np.isfinite(acc_h).all() and not (_bits(acc_h) == POISON_WORD).any()
        zeros = np.zeros(r.numel, f32)
        m, v, cb = r.dev(zeros), r.dev(zeros), r.dev(clip_buffer())
        r.step_call(1, r.struct(r.flat), r.struct(acc, cb, INF), r.flat, acc, m, v, SKIP, 1.0, step=1)
        c = r.host(cb)
        assert same_bits(r.host(r.flat), r.flat0) and same_bits(r.host(m), zeros) and same_bits(r.host(v), zeros)
        assert same_bits(r.host(acc), acc_h), "the skipped optimiser call changed the accumulator"
        assert not np.isfinite(c[0]) and float(c[1]) == 0.0 and counters(c) == (1.0, 1.0), (c[:2], counters(c))


# ---- (f) the refusal, the empty buffer ----------------------------------------------------------------------------------------------------
def check_refusal(be, name="job_mae"):
    """The bit with grads->clip = NULL: (status, every buffer still poison).  No pass has run: everything is poison on entry."""
    with AC.Rig(be, name) as r:
        flat, grad, m, v = r.out(), r.out(), r.out(), r.out()
        status = _status(lambda: r.step_call(0, r.struct(flat), r.struct(grad), flat, grad, m, v, r.flags | SKIP, 1.0))
        be.sync()
        return status, all(is_poison(r.host(b)) for b in (flat, grad, m, v, r.sums))


def check_empty(be, name="job_mae"):
    """n == 0 with the bit, as without it: clip[0] = 0, clip[1] = 1; the counters and everything else untouched.  Returns
    (clip[0..1], counters, untouched)."""
    with AC.Rig(be, name, flags=0) as r:
        flat, grad, m, v = r.out(), r.out(), r.out(), r.out()
        cb = r.dev(clip_buffer(4.0, 3.0))
        r.step_call(0, r.struct(flat), r.struct(grad, cb, 1.0), flat, grad, m, v, SKIP, 1.0, n=0)
        c = r.host(cb)
        return c[:2].tolist(), counters(c), all(is_poison(r.host(b)) for b in (flat, grad, m, v)) and is_poison(c[2:CFD_CLIP_CONSECUTIVE])
