"""Checks of the exponential moving average of the weights inside the fused FNO step's optimiser call (cfd_fno_adam_step_ema;
k_adam_f<VEC, DW, GUARD, true> in cfdbench_amd/csrc/optim.hip).  Used by tests/test_emul_fno_ema.py (CPU, SIMT emulator),
tests/test_gpu_fno_ema.py (MI355X) and, through the row "adam_step_ema" it adds to tests/align_checks.py's table, by
tests/test_gpu_alignment.py.  Everything runs through the C ABI on tests/backends.py's hostile memory.

The alignment table: tests/test_emul_alignment.py asks that every exported entry point with a tensor argument has a row in
tests/align_checks.py's ROWS.  The new entry's row is added to that table from here (register_alignment_row, called by the two test
files of this feature when they are imported, i.e. while pytest collects), and `python -m tests.ema_checks [--sanitize] adam_step_ema`
is the child process of tests/align_checks.py with that row in its table.

The rule (include/cfdbench_amd.h): behind the Adam update of element i, with d = ema_decay as the fp32 the ABI receives,
    ema[i] = fmaf(d, ema[i], fp32((1.f - d) * p_new[i]))
Bound (rule_error): two fp32 roundings of a convex combination -- the product is off by at most 2^-24 |p|, the fmaf by at most 2^-24 of a
result no larger than max(|e|, |p|) -- so every element lies within 2^-23 * max(|e|, |p_new|) of the fp64 value of d e + (1 - d) p_new taken
with the fp32 d and the fp32 1.f - d.  Derived, not measured.  d = 0: ema == p_new bit for bit.  Everything else is compared bit for bit
with cfd_fno_adam_step on the same inputs."""
from __future__ import annotations

import contextlib
import ctypes
import sys

import numpy as np

from cfdbench_amd._capi import CFD_CLIP_FLOATS, CfdError, FnoParams
from tests import accum_checks as AC
from tests import clip_checks as CC
from tests import finetune_checks as FT
from tests import guard_checks as GC
from tests.backends import POISON_WORD

f64, f32 = np.float64, np.float32
SKIP, DW, ACC, INIT = GC.SKIP, GC.DW, GC.ACC, GC.INIT
INF = float("inf")
FLAT_NS = GC.FLAT_NS + (GC.FLAT_N_CAPPED,)  # 1: scalar form; 7: n % 4 tail; 1028: 16-byte form, several threads; 300003: several trips
DECAYS = (0.0, 0.5, 0.999)
HYPER = GC.HYPER
DEFERRING = GC.DEFERRING  # clip_checks' case: 64 x 64, C = 20, L = 2, nmse, flags = 7
BAD_DECAYS = (1.0, -0.1, float("nan"))
same_bits, _bits, is_poison = CC.same_bits, CC._bits, AC.is_poison
_RUNS = {}


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
def rule_error(ema_new, ema_prev, p_new, decay):
    """max over the elements of |ema_new - (d e + (1 - d) p)| / (2^-23 max(|e|, |p|)) with the fp32 d and 1.f - d, in fp64: <= 1 holds the
    bound of the module docstring.  An element whose e and p are both 0 must be 0."""
    d = f32(decay)
    omd = f32(f32(1.0) - d)
    e, p, got = ema_prev.astype(f64), p_new.astype(f64), ema_new.astype(f64)
    want = float(d) * e + float(omd) * p
    bound = 2.0 ** -23 * np.maximum(np.abs(e), np.abs(p))
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err[bound == 0.0] == 0.0).all()
    return float(np.max(err[bound > 0.0] / bound[bound > 0.0], initial=0.0))


def ema_start(n):
    """An average under way: not the parameters themselves, so that both terms of the rule show."""
    return FT.flat_case(n, seed=12)[0]


def step_call(r, k, params, grads, param, grad, m, v, flags, grad_scale, ema, decay, step=1, n=None, hyper=HYPER, old_entry=False):
    """accum_checks.Rig.step_call through the new entry point (old_entry: cfd_fno_adam_step, which has no last two arguments)."""
    P, (di, dc, dm, _dl) = r.be.ptr, r.batches[k]
    args = (r.plan, r.sh, ctypes.byref(params), ctypes.byref(grads), P(di), P(dc), P(dm), P(r.sums), P(r.ws), P(param), P(grad), P(m), P(v),
            r.numel if n is None else n, *hyper, step, float(grad_scale), r.wid, 0, flags, r.be.stream)
    if old_entry:
        r.api.call("cfd_fno_adam_step", *args)
    else:
        r.api.call("cfd_fno_adam_step_ema", *args, P(ema), float(decay))
    r.be.sync()


def _status(call):
    try:
        call()
        return 0
    except CfdError as e:
        return int(str(e).split("(status ")[1].split(")")[0])


def _place(be, place, for_ema=False):
    """None: the placement policy in force; "aligned" / "all4": every buffer on / 4 bytes off the 16-byte grid; "ema4": the EMA alone off it."""
    if place is None:
        return contextlib.nullcontext()
    return be.misaligned(4 if place == "all4" or (place == "ema4" and for_ema) else 0)


def run_flat(be, r, n, flags, decay, clip, mode, place="aligned", steps=3):
    """`steps` optimiser steps on flat buffers of n floats (finetune_checks.flat_case; structs that point nowhere, so r's flags are 0) with
    hyper-parameters HYPER; clip: a NaN-poisoned clip buffer per step, max_grad_norm = half that step's norm.  mode "on": the new entry with
    an EMA that starts at ema_start(n); "null": the new entry with ema = NULL; "old": cfd_fno_adam_step.  One dict per step."""
    p0, gs = FT.flat_case(n)
    with _place(be, place):
        p, m, v = be.dev(p0), be.dev(np.zeros(n, f32)), be.dev(np.zeros(n, f32))
    with _place(be, place, True):
        ema = be.dev(ema_start(n)) if mode == "on" else None
    out = []
    for step, g in enumerate(gs[:steps], 1):
        with _place(be, place):
            dg = be.dev(g)
            cb = be.out((CFD_CLIP_FLOATS,)) if clip else None
        gstruct = FnoParams()
        if clip:
            gstruct.clip, gstruct.max_grad_norm = be.ptr(cb), float(f32(0.5 * np.sqrt(np.sum(g.astype(f64) ** 2))))
        prev = None if ema is None else be.host(ema).copy()
        step_call(r, 0, FnoParams(), gstruct, p, dg, m, v, flags, 1.0, ema, decay, step=step, n=n, old_entry=mode == "old")
        out.append(dict(p=be.host(p).copy(), m=be.host(m).copy(), v=be.host(v).copy(), g=be.host(dg).copy(),
                        clip=None if cb is None else be.host(cb).copy(), ema=None if ema is None else be.host(ema).copy(), ema_prev=prev))
    return out


def assert_same_step(a, b, what, with_ema=False, records=True):
    """records = False: the gradient buffer lies elsewhere -- the 16-byte and the scalar form of k_gradsq cut the sum of squares into other
    partial records (fp64, so clip[0..1] agree all the same): only clip[0..1] are compared.  Where the average alone is off the grid
    k_gradsq runs the form of the call without it and the whole clip buffer is compared."""
    for k in ("p", "m", "v", "g") + (("ema",) if with_ema else ()):
        assert same_bits(a[k], b[k]), f"{what}: {k} differs"
    assert (a["clip"] is None) == (b["clip"] is None)
    if a["clip"] is not None:
        # (records: clip[0..1], the partial records, and the poison behind them)
        assert same_bits(a["clip"][:None if records else 2], b["clip"][:None if records else 2]), f"{what}: the clip buffer differs"
        assert np.isfinite(a["clip"][:2]).all() and float(a["clip"][1]) < 0.51, (what, a["clip"][:2])


# ---- (a) the rule, (b) no other bit moves -------------------------------------------------------------------------------------------
def flat_runs(be, n):
    """Every variant of (a) / (b) at size n, once per backend: {(dw, clip, decay or "old" / "null"): run_flat's list}."""
    key = (be.name, n)
    if key not in _RUNS:
        runs = {}
        with AC.Rig(be, "job_mae", flags=0) as r:
            for dw in (0, DW):
                for clip in (False, True):
                    runs[(dw, clip, "old")] = run_flat(be, r, n, dw, 0.0, clip, "old")
                    runs[(dw, clip, "null")] = run_flat(be, r, n, dw, 0.5, clip, "null")
                    for decay in DECAYS:
                        runs[(dw, clip, decay)] = run_flat(be, r, n, dw, decay, clip, "on")
        _RUNS[key] = runs
    return _RUNS[key]


def check_rule_flat(be, n):
    """(a) with and without DW, with and without clip, decays 0, 0.5, 0.999, three steps: every EMA element within the bound of the value
    the rule gives from the parameters read back after the step and the EMA read back before it; decay 0: the parameters' bits.  Returns
    the worst figure (in units of the bound)."""
    worst = 0.0
    for (dw, clip, decay), run in flat_runs(be, n).items():
        if isinstance(decay, str):
            continue
        for step, s in enumerate(run, 1):
            err = rule_error(s["ema"], s["ema_prev"], s["p"], decay)
            print("ema rule", be.name, n, "adamw" if dw else "adam", "clip" if clip else "no clip", decay, step, err)
            assert err <= 1.0, (n, dw, clip, decay, step, err)
            if decay == 0.0:
                assert same_bits(s["ema"], s["p"]), (n, dw, clip, step, "decay 0 is not a copy of the parameters")
            else:
                assert not same_bits(s["ema"], s["ema_prev"]) and not same_bits(s["ema"], s["p"]), (n, dw, clip, decay, step)
            worst = max(worst, err)
    return worst


def check_no_other_bit_moves(be, n):
    """(b) parameters, both moments, gradient buffer and clip buffer after every step: the new entry with an EMA == the new entry with
    ema = NULL == cfd_fno_adam_step, bit for bit."""
    runs = flat_runs(be, n)
    for dw in (0, DW):
        for clip in (False, True):
            old = runs[(dw, clip, "old")]
            assert not same_bits(old[-1]["p"], FT.flat_case(n)[0])
            for tag in ("null",) + DECAYS:
                for step, (a, b) in enumerate(zip(old, runs[(dw, clip, tag)]), 1):
                    assert_same_step(a, b, f"n = {n}, dw = {dw}, clip = {clip}, {tag}, step {step}")


# ---- (c) placement ------------------------------------------------------------------------------------------------------------------
def check_placement(be, n=1028, decay=0.5):
    """AdamW with clipping, three steps, under the placement policy in force against the same run with every buffer on the 16-byte grid:
    the number of steps in which any buffer, the EMA included, differs in a bit.  (The row "adam_step_ema" of tests/align_checks.py: all
    buffers shifted by 4 and by 8 bytes, and each buffer alone -- the EMA among them -- shifted by 4.)"""
    with AC.Rig(be, "job_mae", flags=0) as r:
        ref = run_flat(be, r, n, DW, decay, True, "on", place="aligned")
        got = run_flat(be, r, n, DW, decay, True, "on", place=None)
    bad = 0
    for a, b in zip(ref, got):
        bad += not (all(same_bits(a[k], b[k]) for k in ("p", "m", "v", "g", "ema")) and same_bits(a["clip"][:2], b["clip"][:2]))
    assert rule_error(got[-1]["ema"], got[-1]["ema_prev"], got[-1]["p"], decay) <= 1.0
    return bad


def check_misplaced(be, ns=FLAT_NS[:3]):
    """All buffers 4 bytes off the 16-byte grid, and the EMA alone off it while the others are aligned: both the aligned run's bits."""
    with AC.Rig(be, "job_mae", flags=0) as r:
        for n in ns:
            for dw, clip in ((0, False), (DW, True)):
                ref = flat_runs(be, n)[(dw, clip, 0.5)]
                for place in ("all4", "ema4"):
                    got = run_flat(be, r, n, dw, 0.5, clip, "on", place=place)
                    for step, (a, b) in enumerate(zip(ref, got), 1):
                        assert_same_step(a, b, f"n = {n}, dw = {dw}, clip = {clip}, {place}, step {step}", with_ema=True, records=place == "ema4")


# ---- (d) the lifting layer's rows -----------------------------------------------------------------------------------------------------
def check_stem_rows(be, clip, decay=0.5, name=DEFERRING):
    """One pass of the deferring case, then the optimiser call with an EMA on a copy of the pass's gradient buffer -- without `clip` the
    job's workgroups of k_adam_f finish the fc0 rows (stem_row), with it k_gradsq takes the job and the flat walk covers them -- beside
    cfd_fno_adam_step on another copy.  The whole EMA, the fc0 ranges looked at on their own, obeys the rule; nothing else moves a bit."""
    with AC.Rig(be, name) as r:
        r.backward(0)
        g_pass = r.host(r.grad)
        rows = np.r_[slice(*np.cumsum(r.layout["fc0.weight"])), slice(*np.cumsum(r.layout["fc0.bias"]))]
        assert is_poison(g_pass[rows]), f"{name}: the lifting layer's rows were not left to the optimiser call"
        zeros = np.zeros(r.numel, f32)
        ema0 = (r.flat0 + f32(0.01)).astype(f32)
        got = {}
        for tag in ("old", "ema"):
            flat, grad, m, v = r.dev(r.flat0), r.dev(g_pass), r.dev(zeros), r.dev(zeros)
            cb = r.out(CFD_CLIP_FLOATS) if clip else None
            ema = r.dev(ema0) if tag == "ema" else None
            step_call(r, 0, r.struct(flat), r.struct(grad, cb, 1.0), flat, grad, m, v, r.flags, 1.0, ema, decay, old_entry=tag == "old")
            got[tag] = dict(p=r.host(flat), m=r.host(m), v=r.host(v), g=r.host(grad), clip=None if cb is None else r.host(cb),
                            ema=None if ema is None else r.host(ema))
        a, b = got["old"], got["ema"]
        for k in ("p", "m", "v", "g"):
            assert same_bits(a[k], b[k]), f"clip = {clip}: {k} differs from cfd_fno_adam_step's"
        if clip:
            assert same_bits(a["clip"], b["clip"]) and np.isfinite(b["clip"][:2]).all(), b["clip"][:2]
        assert np.isfinite(b["g"]).all() and not same_bits(b["p"][rows], r.flat0[rows]), "the fc0 rows were not stepped"
        errs = (rule_error(b["ema"][rows], ema0[rows], b["p"][rows], decay), rule_error(b["ema"], ema0, b["p"], decay))
        print("ema stem rows", be.name, "clip" if clip else "no clip", errs)
        assert max(errs) <= 1.0, errs
        assert not (_bits(b["ema"][rows]) == _bits(ema0[rows])).all()
        return errs


# ---- (e) the guard ---------------------------------------------------------------------------------------------------------------------
def check_guard(be, ns=(7, 1028), decay=0.5):
    """One NaN in the gradient with CFD_STEP_SKIP_NONFINITE: the EMA -- one element of it NaN poison -- keeps every bit with parameters and
    moments, the counters go to (1, 1); the next, finite step updates it by the rule (the poisoned element stays NaN) and is bitwise
    cfd_fno_adam_step's."""
    with AC.Rig(be, "job_mae", flags=0) as r:
        for n in ns:
            p0, gs = FT.flat_case(n)
            e0 = ema_start(n).copy()
            _bits(e0)[n // 3] = POISON_WORD
            ok = np.ones(n, bool)
            ok[n // 3] = False
            bad = gs[0].copy()
            bad[n - 1] = float("nan")
            for dw in (0, DW):
                state = {}
                for tag in ("old", "ema"):
                    state[tag] = dict(p=be.dev(p0), m=be.dev(np.zeros(n, f32)), v=be.dev(np.zeros(n, f32)), cb=be.dev(GC.clip_buffer()),
                                      ema=be.dev(e0) if tag == "ema" else None)
                for step, g in ((1, bad), (2, gs[1])):
                    for tag, s in state.items():
                        dg = be.dev(g)
                        gstruct = FnoParams()
                        gstruct.clip, gstruct.max_grad_norm = be.ptr(s["cb"]), INF
                        step_call(r, 0, FnoParams(), gstruct, s["p"], dg, s["m"], s["v"], SKIP | dw, 1.0, s["ema"], decay, step=step, n=n,
                                  old_entry=tag == "old")
                    a, b = state["old"], state["ema"]
                    for k in ("p", "m", "v", "cb"):
                        assert same_bits(be.host(a[k]), be.host(b[k])), (n, dw, step, k)
                    c, e = be.host(b["cb"]), be.host(b["ema"])
                    if step == 1:
                        assert same_bits(e, e0), (n, dw, "the skipped step changed the EMA")
                        assert same_bits(be.host(b["p"]), p0) and float(c[1]) == 0.0 and GC.counters(c) == (1.0, 1.0), (n, dw, c[:2])
                    else:
                        p = be.host(b["p"])
                        assert GC.counters(c) == (1.0, 0.0) and float(c[1]) == 1.0 and not same_bits(p, p0), (n, dw, c[:2])
                        assert np.isnan(e[~ok]).all() and rule_error(e[ok], e0[ok], p[ok], decay) <= 1.0, (n, dw)
                        assert n == 1 or not same_bits(e[ok], e0[ok])


# ---- (f) accumulate, refusals, the empty buffer ---------------------------------------------------------------------------------------------
def check_accumulate_ignores_the_ema(be, name=DEFERRING):
    """The accumulate call through the new entry with a poisoned `ema` and, as nothing of the two arguments is read there, a decay that
    the optimiser call would refuse: the EMA stays poison, accumulator and gradient buffer are bitwise cfd_fno_adam_step's."""
    with AC.Rig(be, name) as r:
        r.backward(0)
        g_pass = r.host(r.grad)
        got = {}
        for tag in ("old", "ema"):
            acc, grad = r.out(), r.dev(g_pass)
            ema = r.out() if tag == "ema" else None
            step_call(r, 0, r.struct(acc), r.struct(grad), acc, grad, None, None, r.flags | ACC | INIT, 0.5, ema, float("nan"), step=0,
                      hyper=(float("nan"),) * 5, old_entry=tag == "old")
            got[tag] = (r.host(acc), r.host(grad))
            assert ema is None or is_poison(r.host(ema)), "the accumulate call touched the EMA"
        assert same_bits(got["old"][0], got["ema"][0]) and same_bits(got["old"][1], got["ema"][1])
        assert np.isfinite(got["ema"][0]).all() and np.any(got["ema"][0] != 0.0)


def check_bad_decay(be, n=1028):
    """ema_decay = 1, -0.1, NaN with an EMA: {decay: (status, every buffer kept its bits)}.  With ema = NULL the same values are not read."""
    res = {}
    with AC.Rig(be, "job_mae", flags=0) as r:
        p0, gs = FT.flat_case(n)
        for decay in BAD_DECAYS:
            p, m, v, dg, ema, cb = be.dev(p0), be.out((n,)), be.out((n,)), be.dev(gs[0]), be.dev(ema_start(n)), be.out((CFD_CLIP_FLOATS,))
            gstruct = FnoParams()
            gstruct.clip, gstruct.max_grad_norm = be.ptr(cb), 1.0
            status = _status(lambda: step_call(r, 0, FnoParams(), gstruct, p, dg, m, v, DW, 1.0, ema, decay, n=n))
            be.sync()
            kept = (same_bits(be.host(p), p0) and same_bits(be.host(dg), gs[0]) and same_bits(be.host(ema), ema_start(n))
                    and all(is_poison(be.host(b)) for b in (m, v, cb)))
            res[str(decay)] = (status, kept)
            m2, v2 = be.dev(np.zeros(n, f32)), be.dev(np.zeros(n, f32))
            assert _status(lambda: step_call(r, 0, FnoParams(), FnoParams(), p, dg, m2, v2, 0, 1.0, None, decay, n=n)) == 0
    return res


def check_empty(be):
    """n == 0 with an EMA: nothing of it is written; with `clip`, clip[0..1] = (0, 1) as without the EMA."""
    with AC.Rig(be, "job_mae", flags=0) as r:
        flat, grad, m, v, ema, cb = r.out(), r.out(), r.out(), r.out(), r.out(), r.out(CFD_CLIP_FLOATS)
        step_call(r, 0, r.struct(flat), r.struct(grad), flat, grad, m, v, 0, 1.0, ema, 0.5, n=0)
        quiet = all(is_poison(r.host(b)) for b in (flat, grad, m, v, ema, cb))
        step_call(r, 0, r.struct(flat), r.struct(grad, cb, 1.0), flat, grad, m, v, 0, 1.0, ema, 0.5, n=0)
        return quiet and all(is_poison(r.host(b)) for b in (flat, grad, m, v, ema)), r.host(cb)[:2].tolist()


# ---- the row of the alignment table -----------------------------------------------------------------------------------------------------
ALIGN_ROW = "adam_step_ema"


def register_alignment_row():
    """The row of cfd_fno_adam_step_ema in tests/align_checks.py's table (module docstring): check_placement, accepted when no step
    differs in a bit; each4 also on the emulator, as the launcher has an alignment gate.  Idempotent.  Returns the row."""
    from tests import align_checks as A
    if ALIGN_ROW not in A.BY_ID:
        row = A.Row(ALIGN_ROW, check_placement, (), A.zero, emul_each=True)
        A.ROWS.append(row)
        A.BY_ID[row.id] = row
    return A.BY_ID[ALIGN_ROW]


if __name__ == "__main__":
    # (the row's check must be the importable module's function, not this script's copy of it: the table looks helpers up by module)
    from tests import align_checks as _A
    from tests import ema_checks as _EC
    _EC.register_alignment_row()
    sys.exit(_A.main(sys.argv[1:]))
