"""Checks of the training objectives beside mse / nmse / mae: cfd_objective_fwd / cfd_objective_bwd (cfdbench_amd/csrc/objective.hip;
include/cfdbench_amd.h, "Training objectives").  Used by tests/test_emul_fno_objective.py (CPU, SIMT emulator), tests/test_gpu_fno_objective.py
(MI355X), tests/test_cpu_objective.py (the golden) and, through the row "objective" it adds to tests/align_checks.py's table, by the
alignment files.  The C-ABI checks run on tests/backends.py's hostile memory: poisoned outputs, guard bands, be.verify().

The alignment table: as tests/ema_checks.py does, the row is added from here (register_alignment_row, called by the test files of this
feature while pytest collects), and `python -m tests.objective_checks [--sanitize] objective` is the child process with that row.

Reference: reference() below, fp64 NumPy on the same fp32 inputs.

Bound, derived for the operation order of objective.hip, with u = 2^-24 (half an fp32 ulp, relative) and 0/1 masks, so that
label * mask is exact:
  d = fp32(preds - label * mask): |d - d*| <= u |d*|, the only fp32 rounding in front of the sums (a difference of nearby numbers is exact).
  d * d and (label * mask)^2 are exact in fp64 (24-bit factors), the sums are fp64 (n 2^-53: nothing on this scale), so
      E = E* (1 + 2u + u^2) at worst, S = S*.
  value:  sqrt(E) / sqrt(S) is off by u, E / S by 2u; the mean of non-negative terms keeps that; one final rounding: u.     -> <= 3u
  batch-global sums in rec: sum d^2 <= 2u, sum (label * mask)^2 exact.                                                      -> <= 2u
  gradient: coef in fp64 from E (rel_l2: 1 / sqrt(E), u; the nMSE kinds: S only, exact), times d (u), rounded once (u).     -> <= 3u
  with gadd: the term is rounded (above), then ONE fp32 addition: u (|gadd| + |term|) more at worst.                        -> <= 4u
            of |gadd| + |term|
UNITS holds these first-order counts; SLACK = 1 + 2^-10 covers the second-order terms and the fp64 roundings.  All stay below the 16 u
above which fp64 accumulation would have been lost.  Derived, not measured."""
from __future__ import annotations

import sys

import numpy as np

from cfdbench_amd._capi import CFD_OBJ_REC_FLOATS, OBJECTIVE_IDS, CfdError
from tests.backends import POISON_WORD

f64, f32 = np.float64, np.float32
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
UNITS = {"value": 3.0, "sums": 2.0, "grad": 3.0, "grad_gadd": 4.0}
assert max(UNITS.values()) * SLACK <= 16.0
KINDS = tuple(OBJECTIVE_IDS)
MAX_PARTS = 8
# (B, Co, HW): one element; a tail of 3 behind one unit; 66 x 65 -- HW % 4 != 0, two parts per slice; several slices of one whole part;
# four parts per slice
SHAPES = ((1, 1, 1), (2, 2, 7), (3, 3, 4290), (5, 8, 4096), (2, 2, 16384))


def n_parts(HW):
    """Parts per slice (objective.hip: obj_split)."""
    return min(-(-HW // 4096), MAX_PARTS)


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def is_poison(a):
    return bool((_bits(a) == POISON_WORD).all())


def load_f64(rec, i):
    """The fp64 stored as two 32-bit words at rec[i], rec[i + 1]."""
    return float(np.ascontiguousarray(rec[i:i + 2]).view(f64)[0])


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def reference(preds, label, mask, kind, gadd=None, upstream=1.0):
    """fp64: dict(value, grad -- gadd included --, term, E, S: the batch-global sums).  preds, label: (B, Co, HW); mask: (B, HW) or None."""
    p, lab = preds.astype(f64), label.astype(f64)
    lm = lab if mask is None else lab * mask.astype(f64)[:, None, :]
    d = p - lm
    E, S = (d * d).sum(-1), (lm * lm).sum(-1)
    B, Co = E.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "rel_l2":
            Eb, Sb = E.sum(1), S.sum(1)
            value = np.mean(np.sqrt(Eb) / np.sqrt(Sb))
            coef = np.where(Eb == 0.0, 0.0, 1.0 / (B * np.sqrt(Eb) * np.sqrt(Sb)))[:, None, None]
        elif kind == "nmse_sample":
            Eb, Sb = E.sum(1), S.sum(1)
            value = np.mean(Eb / Sb)
            coef = (2.0 / (B * Sb))[:, None, None]
        elif kind == "nmse_channel":
            Ec, Sc = E.sum(0), S.sum(0)
            value = np.mean(Ec / Sc)
            coef = (2.0 / (Co * Sc))[None, :, None]
        else:
            raise ValueError(kind)
        term = float(upstream) * coef * d
    grad = term if gadd is None else gadd.astype(f64) + term
    return dict(value=float(value), grad=grad, term=term, E=float(E.sum()), S=float(S.sum()))


def case(B, Co, HW, seed=0, masked=True):
    """Seeded O(1) inputs: preds (carrying the mask), label, a 0/1 mask with about a fifth of zeros (or None), gadd."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * Co + HW)
    mask = (rng.random((B, HW)) > 0.2).astype(f32) if masked else None
    preds = rng.standard_normal((B, Co, HW)).astype(f32)
    if masked:
        preds *= mask[:, None, :]
    label = (rng.standard_normal((B, Co, HW)) * (1.0 + np.arange(B)[:, None, None])).astype(f32)  # (samples of different scale)
    if HW == 1 and masked:
        mask[:] = 1.0
    gadd = rng.standard_normal((B, Co, HW)).astype(f32)
    return preds, label, mask, gadd


# ---- the calls -----------------------------------------------------------------------------------------------------------------------
def call_fwd(be, preds, label, mask, rec, value, B, Co, HW, kind):
    P = be.ptr
    be.api.call("cfd_objective_fwd", P(preds), P(label), P(mask), P(rec), P(value), B, Co, HW, OBJECTIVE_IDS.get(kind, kind), be.stream)


def call_bwd(be, preds, label, mask, rec, gadd, updev, upstream, gpreds, B, Co, HW, kind):
    P = be.ptr
    be.api.call("cfd_objective_bwd", P(preds), P(label), P(mask), P(rec), P(gadd), P(updev), float(upstream), P(gpreds), B, Co, HW,
                OBJECTIVE_IDS.get(kind, kind), be.stream)


def run(be, shape, kind, masked=True, with_gadd=False, upstream=1.0, updev=None, alias=False, seed=0, data=None, twice=False):
    """fwd + bwd on fresh hostile buffers.  updev: a value for the device scalar (None: NULL); alias: gpreds is the gadd buffer; twice:
    both calls once more on the now dirty rec / value / gpreds (with alias, gadd is written back first).  Returns dict(value, rec, gpreds)
    as host arrays and `ref`, the fp64 reference with the fp32 upstream values."""
    B, Co, HW = shape
    preds, label, mask, gadd = data if data is not None else case(B, Co, HW, seed, masked)
    if not with_gadd:
        gadd = None
    dp, dl = be.dev(preds), be.dev(label)
    dm = be.dev(mask) if mask is not None else None
    dg = be.dev(gadd) if gadd is not None else None
    du = be.dev(np.array([updev], f32)) if updev is not None else None
    rec, value = be.out((CFD_OBJ_REC_FLOATS(B, Co),)), be.out((1,))
    gp = dg if alias else be.out((B, Co, HW))
    assert not alias or with_gadd
    for k in range(2 if twice else 1):
        if k and alias:
            if be.name == "gpu":
                gp.copy_(be.torch.from_numpy(gadd))
            else:
                gp[...] = gadd
        call_fwd(be, dp, dl, dm, rec, value, B, Co, HW, kind)
        call_bwd(be, dp, dl, dm, rec, dg, du, upstream, gp, B, Co, HW, kind)
        be.sync()
    up = float(f32(upstream)) * (float(f32(updev)) if updev is not None else 1.0)
    return dict(value=be.host(value).copy(), rec=be.host(rec).copy(), gpreds=be.host(gp).copy(),
                ref=reference(preds, label, mask, kind, gadd, up))


def rel_err(got, want):
    return abs(float(got) - want) / abs(want) if want != 0.0 else abs(float(got))


def errors(res, shape, with_gadd):
    """The figures of one run in units of u: value, the two batch-global sums in rec, the worst gradient element (relative to
    |gadd| + |term|; an element whose scale is 0 must be exactly the reference)."""
    ref, rec = res["ref"], res["rec"]
    got, want = res["gpreds"].astype(f64), ref["grad"]
    scale = np.abs(ref["term"]) + (np.abs(want - ref["term"]) if with_gadd else 0.0)
    err = np.abs(got - want)
    assert np.isfinite(got).all() and (err[scale == 0.0] == 0.0).all()
    out = dict(value=rel_err(res["value"][0], ref["value"]) / U, E=rel_err(load_f64(rec, 0), ref["E"]) / U, S=rel_err(load_f64(rec, 2), ref["S"]) / U,
               grad=float(np.max(err[scale > 0.0] / scale[scale > 0.0], initial=0.0)) / U)
    out["value64"] = rel_err(load_f64(rec, 4), ref["value"]) / U
    return out


def assert_within(figs, with_gadd, what):
    print("objective", what, {k: round(v, 4) for k, v in figs.items()})
    assert figs["value"] <= UNITS["value"] * SLACK and figs["value64"] <= (UNITS["value"] - 1.0) * SLACK, (what, figs)
    assert figs["E"] <= UNITS["sums"] * SLACK and figs["S"] <= 2.0 ** -20, (what, figs)
    assert figs["grad"] <= UNITS["grad_gadd" if with_gadd else "grad"] * SLACK, (what, figs)


def assert_rec_layout(rec, shape):
    """What the header says is not written is still poison: rec[6..7] and everything behind the part records of this shape."""
    B, Co, HW = shape
    used = 8 + 4 * max(B, Co) + 4 * B * Co * n_parts(HW)
    assert rec.size == CFD_OBJ_REC_FLOATS(B, Co) and is_poison(rec[6:8]) and is_poison(rec[used:])
    assert not (_bits(rec[:6]) == POISON_WORD).any() and not (_bits(rec[8 + 4 * max(B, Co):used]) == POISON_WORD).any()


# ---- (a) parity ----------------------------------------------------------------------------------------------------------------------
VARIANTS = {  # masked, with_gadd, upstream, updev, alias
    "plain": (True, False, 1.0, None, False),
    "no_mask": (False, False, 1.0, None, False),
    "gadd": (True, True, 1.0, None, False),
    "gadd_alias": (True, True, 1.0, None, True),
    "upstream": (True, False, 0.37, None, False),
    "upstream_dev": (True, False, 1.0, -1.7, False),
    "upstream_both_gadd_no_mask": (False, True, 0.5, 0.3, True),
}


def check_parity(be, shape, kind):
    """Every variant at one shape and kind: value, batch-global sums and every gradient element within the derived bound; the unwritten
    parts of rec untouched.  Returns {variant: figures}."""
    out = {}
    for name, (masked, with_gadd, upstream, updev, alias) in VARIANTS.items():
        res = run(be, shape, kind, masked, with_gadd, upstream, updev, alias)
        assert_rec_layout(res["rec"], shape)
        out[name] = errors(res, shape, with_gadd)
        assert_within(out[name], with_gadd, (be.name, shape, kind, name))
    return out


# ---- (b) determinism and placement ---------------------------------------------------------------------------------------------------
def _written(res, shape):
    B, Co, HW = shape
    used = 8 + 4 * max(B, Co) + 4 * B * Co * n_parts(HW)
    return [res["value"], res["rec"][:6], res["rec"][8:used], res["gpreds"]]


def check_twice(be, shape, kind):
    """Two calls, the second on the first's dirty buffers: the same bits as one call on poisoned ones."""
    a = run(be, shape, kind, with_gadd=True, alias=True, updev=0.7)
    b = run(be, shape, kind, with_gadd=True, alias=True, updev=0.7, twice=True)
    return sum(not same_bits(x, y) for x, y in zip(_written(a, shape), _written(b, shape)))


def check_placement(be, shapes=((2, 2, 16384), (3, 2, 4100)), kinds=KINDS):
    """Under the placement policy in force against every buffer on the 16-byte grid (the 16-byte form where HW % 4 == 0): the number of
    outputs -- value, the written parts of rec, gpreds -- that differ in a bit.  The runs under the policy must also hold the bound."""
    bad = 0
    for shape in shapes:
        for kind in kinds:
            for name in ("plain", "upstream_both_gadd_no_mask"):
                masked, with_gadd, upstream, updev, alias = VARIANTS[name]
                with be.misaligned(0):
                    ref = run(be, shape, kind, masked, with_gadd, upstream, updev, alias)
                got = run(be, shape, kind, masked, with_gadd, upstream, updev, alias)
                assert_within(errors(got, shape, with_gadd), with_gadd, (be.name, shape, kind, name, "placed"))
                bad += sum(not same_bits(x, y) for x, y in zip(_written(ref, shape), _written(got, shape)))
    return bad


def check_misplaced(be, shape=(2, 2, 16384)):
    """Every buffer 4 and 8 bytes off the grid, and single buffers alone: the aligned bits."""
    bad = 0
    for kind in KINDS:
        with be.misaligned(0):
            ref = run(be, shape, kind, with_gadd=True, updev=0.7)
        for shift, only in ((4, None), (8, None), (4, 0), (4, 2), (4, 3), (4, 5), (4, 7)):
            with be.misaligned(shift, only=only):
                got = run(be, shape, kind, with_gadd=True, updev=0.7)
            bad += sum(not same_bits(x, y) for x, y in zip(_written(ref, shape), _written(got, shape)))
    return bad


# ---- (c) edges -----------------------------------------------------------------------------------------------------------------------
def check_exact_sample(be, shape=(3, 2, 100)):
    """rel_l2 with sample 1's preds == label * mask exactly: its gradient is exactly 0 (with gadd: gadd's bits), the others hold the bound."""
    preds, label, mask, gadd = case(*shape, seed=3)
    preds[1] = label[1] * mask[1][None, :]
    for with_gadd in (False, True):
        res = run(be, shape, "rel_l2", with_gadd=with_gadd, data=(preds, label, mask, gadd))
        g = res["gpreds"]
        assert same_bits(g[1], gadd[1] if with_gadd else np.zeros_like(g[1])), "the exact sample's gradient is not exactly 0"
        assert_within(errors(res, shape, with_gadd), with_gadd, (be.name, "exact sample", with_gadd))
        assert np.any(res["ref"]["term"][0] != 0.0)


def check_zero_label(be, shape=(3, 2, 100)):
    """Sample 1's label all zero (channel 1's for nmse_channel): the value is not finite; every gradient the definition leaves finite is
    finite and within the bound -- the other samples (channels) -- and the zero group's is not."""
    out = {}
    for kind in KINDS:
        preds, label, mask, gadd = case(*shape, seed=4)
        if kind == "nmse_channel":
            label[:, 1] = 0.0
            zero = (slice(None), 1)
            rest = (slice(None), 0)
        else:
            label[1] = 0.0
            zero, rest = (1,), ([0, 2],)
        res = run(be, shape, kind, data=(preds, label, mask, gadd))
        g, want = res["gpreds"], res["ref"]["grad"]
        assert not np.isfinite(res["value"][0]) and not np.isfinite(res["ref"]["value"]), (kind, res["value"])
        assert np.isfinite(g[rest]).all() and not np.isfinite(g[zero]).any(), kind
        err = np.abs(g[rest].astype(f64) - want[rest])
        scale = np.abs(want[rest])
        assert (err[scale == 0.0] == 0.0).all()
        out[kind] = float(np.max(err[scale > 0] / scale[scale > 0])) / U
        assert out[kind] <= UNITS["grad"] * SLACK, (kind, out)
    return out


def _status(call):
    try:
        call()
        return 0
    except CfdError as e:
        return int(str(e).split("(status ")[1].split(")")[0])


def check_refusals(be, shape=(2, 2, 64)):
    """Unknown kind, B / Co / HW < 1 and NULL required pointers: {what: (status, every buffer kept its bits)}; -1 and True throughout."""
    B, Co, HW = shape
    preds, label, mask, gadd = case(B, Co, HW, seed=5)
    dp, dl, dm, dg = be.dev(preds), be.dev(label), be.dev(mask), be.dev(gadd)
    rec, value, gp = be.out((CFD_OBJ_REC_FLOATS(B, Co),)), be.out((1,)), be.out((B, Co, HW))
    good = be.out((CFD_OBJ_REC_FLOATS(B, Co),))
    call_fwd(be, dp, dl, dm, good, be.out((1,)), B, Co, HW, "rel_l2")
    be.sync()
    good0 = be.host(good).copy()

    def kept():
        be.sync()
        return (is_poison(be.host(rec)) and is_poison(be.host(value)) and is_poison(be.host(gp)) and same_bits(be.host(good), good0)
                and same_bits(be.host(dp), preds) and same_bits(be.host(dl), label) and same_bits(be.host(dg), gadd))

    res = {}
    fwd = dict(kind=(dp, dl, dm, rec, value, B, Co, HW, 3), kind_neg=(dp, dl, dm, rec, value, B, Co, HW, -1),
               B=(dp, dl, dm, rec, value, 0, Co, HW, 0), Co=(dp, dl, dm, rec, value, B, 0, HW, 1), HW=(dp, dl, dm, rec, value, B, Co, -4, 2),
               preds=(None, dl, dm, rec, value, B, Co, HW, 0), label=(dp, None, dm, rec, value, B, Co, HW, 0),
               rec=(dp, dl, dm, None, value, B, Co, HW, 0), value=(dp, dl, dm, rec, None, B, Co, HW, 0))
    for k, a in fwd.items():
        res["fwd:" + k] = (_status(lambda: call_fwd(be, *a)), kept())
    bwd = dict(kind=(dp, dl, dm, good, dg, None, 1.0, gp, B, Co, HW, 7), B=(dp, dl, dm, good, dg, None, 1.0, gp, -1, Co, HW, 0),
               Co=(dp, dl, dm, good, dg, None, 1.0, gp, B, 0, HW, 0), HW=(dp, dl, dm, good, dg, None, 1.0, gp, B, Co, 0, 0),
               preds=(None, dl, dm, good, dg, None, 1.0, gp, B, Co, HW, 0), label=(dp, None, dm, good, dg, None, 1.0, gp, B, Co, HW, 0),
               rec=(dp, dl, dm, None, dg, None, 1.0, gp, B, Co, HW, 0), gpreds=(dp, dl, dm, good, dg, None, 1.0, None, B, Co, HW, 0))
    for k, a in bwd.items():
        res["bwd:" + k] = (_status(lambda: call_bwd(be, *a)), kept())
    return res


# ---- (d) the whole model: FnoTrainEngine(objective=) against the fp64 chain --------------------------------------------------------------
# 64 x 64, C = 20: the pair route (out_chan = 2); 66 x 65 with three channels: the head's channel route; C = 40: the wide route; 12 x 12
# padded by 4: the padded shape of tests/window_checks.py.  Bounds: what the fused step's own checks hold their nmse step to on the same
# route -- tests/finetune_checks.py: GRAD_TOL, on the channel route GRAD_TOL_CHAN; tests/accum_checks.py: GRAD_TOL_PAD on a padded shape;
# moments and parameter deltas: tests/clip_checks.py's ADAM_TOL (all rel_nmse, as there).
MODEL_CASES = {
    "pair": dict(B=3, C=20, L=2, H=64, W=64, m1=12, m2=12, p=5, cin=2, cout=2, pad=0),
    "chan": dict(B=2, C=20, L=2, H=66, W=65, m1=12, m2=12, p=5, cin=3, cout=3, pad=0),
    "wide": dict(B=2, C=40, L=2, H=32, W=32, m1=12, m2=12, p=5, cin=2, cout=2, pad=0),
    "padded": dict(B=2, C=6, L=2, H=12, W=12, m1=4, m2=4, p=5, cin=2, cout=2, pad=4),
}
LR = 1e-3
VALUE_TOL = 1e-5  # the objective of the fp32 model against the fp64 model's: the relative bound every loss check of the suite uses


def grad_tol(name):
    from tests import accum_checks as AC
    from tests import finetune_checks as FT
    return {"pair": FT.GRAD_TOL, "wide": FT.GRAD_TOL, "chan": FT.GRAD_TOL_CHAN, "padded": AC.GRAD_TOL_PAD}[name]


def adam_tol():
    from tests import clip_checks as CC
    return CC.ADAM_TOL


def model_case(name, bseed=42):
    """(params, batch, shape record) of a case: tests/ingrad_checks.small_case's seeded weights and batch (a border mask)."""
    from tests import ingrad_checks as IC
    s = MODEL_CASES[name]
    params, batch = IC.small_case(s["B"], s["C"], s["L"], s["H"], s["W"], s["m1"], s["m2"], s["p"], s["cin"], s["pad"], bseed=bseed, cout=s["cout"])
    return params, batch, s


def ref_pass(params, batch, s, kind, label=None, inputs=None, gadd=None, upstream=1.0):
    """One pass in fp64: the model at `inputs` (default: the batch's), the objective against `label` (default: the batch's) on the fp64
    predictions, its gradient times `upstream` plus `gadd` as the gradient on the predictions, and the model's adjoint.  Without padding the
    chain is oracle.fno_forward -> reference() -> oracle.fno_backward; oracle.fno_forward has no domain padding, so a padded shape takes
    tests/ingrad_checks.py's fp64 restatement of the forward pass and autograd as its adjoint.  dict(preds, value, grads, g_inputs)."""
    from oracle import fno_oracle as O
    x = batch["inputs"] if inputs is None else inputs
    lab = batch["label"] if label is None else label
    B, Co = lab.shape[:2]
    mask2 = batch["mask"].reshape(B, -1)

    def objective(preds):
        o = reference(preds.reshape(B, Co, -1), lab.reshape(B, Co, -1), mask2, kind, None if gadd is None else np.asarray(gadd).reshape(B, Co, -1),
                      upstream)
        return o["value"], o["grad"].reshape(preds.shape)

    if s["pad"] == 0:
        p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else f64) for k, v in params.items()}
        fw = O.fno_forward(p64, x.astype(f64), batch["case_params"].astype(f64), batch["mask"].astype(f64), lab.astype(f64), s["L"])
        value, G = objective(fw["preds"])
        g = O.fno_backward(p64, fw["cache"], G, s["L"])
        g_inputs = g.pop("__inputs__")  # (the first two input channels: read only where in_chan == 2)
        return dict(preds=fw["preds"], value=value, grads=g, g_inputs=g_inputs)
    import torch

    from tests import ingrad_checks as IC
    tp, tb = IC._leaves(params, dict(batch, inputs=np.asarray(x)))
    preds = IC.ref_forward(tp, tb["inputs"], tb["case_params"], tb["mask"], s["L"], s["pad"])
    value, G = objective(preds.detach().numpy())
    (preds * torch.from_numpy(G)).sum().backward()
    return dict(preds=preds.detach().numpy(), value=value, grads={k: v.grad.numpy() for k, v in tp.items()}, g_inputs=tb["inputs"].grad.numpy())


def ref_window(params, batch, s, kind, labels_seq):
    """fp64: the gradient of (1 / K) sum_k objective_k with prediction k fed back as the input of step k + 1 -- the passes K .. 1, step k's
    gradient on its predictions being its own objective's (upstream 1 / K) plus step k + 1's gradient of its inputs (gadd)."""
    K_ = len(labels_seq)
    xs, fw = [batch["inputs"]], []
    for k in range(K_):
        fw.append(ref_pass(params, batch, s, kind, labels_seq[k], xs[k]))
        xs.append(fw[k]["preds"])
    total, gadd = None, None
    for k in range(K_ - 1, -1, -1):
        r = ref_pass(params, batch, s, kind, labels_seq[k], xs[k], gadd=gadd, upstream=1.0 / K_)
        gadd = r["g_inputs"]
        total = r["grads"] if total is None else {q: total[q] + r["grads"][q] for q in total}
    return dict(grads=total, values=[f["value"] for f in fw], preds=[f["preds"] for f in fw])


def make_model(params, s, loss="nmse"):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import objective_to_fn
    model = Fno2d(s["cin"], s["cout"], s["p"], objective_to_fn(loss), s["L"], s["m1"], s["m2"], s["C"], padding=s["pad"] or None).cuda()
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model


class Counting:
    """Stands in for the engine's api: the names of the C calls it makes."""

    def __init__(self, api):
        self._api, self.names = api, []

    def __getattr__(self, name):
        return getattr(self._api, name)

    def call(self, name, *args):
        self.names.append(name)
        return self._api.call(name, *args)


def make_engine(params, s, **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    eng = FnoTrainEngine(make_model(params, s), lr=LR, loss_name="nmse", **kw)
    eng.api = Counting(eng.api)
    return eng


def to_dev(batch):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch.items()}


def step_args(tb, label=None):
    return tb["inputs"], tb["label"] if label is None else label, tb["case_params"], tb["mask"]


def engine_tensors(eng, flat):
    """{name: its floats} of the engine's trainable tensors inside a flat buffer laid out like flat.data (compact under a frozen subset)."""
    a = flat.detach().cpu().numpy()
    out = {}
    for k, p_, off, t in zip(eng.param_names, eng.flat.params, eng.flat.offsets, eng.flat.trainable):
        if t:
            out[k] = a[off:off + p_.numel() * (2 if p_.is_complex() else 1)].copy()
    return out


def compare_step(eng, flat0, ref_grads, coef=1.0, step=1):
    """gradients() and both moments of the engine's first optimiser step, tensor by tensor, against `ref_grads` (fp64, by name) and
    oracle.adam_step on coef * ref_grads: {"g:name" | "m:name" | "v:name": rel_nmse}; and "delta", the parameter delta over the whole
    flat buffer -- the quantity tests/clip_checks.py and tests/finetune_checks.py hold to ADAM_TOL.  (Not per tensor: the first Adam update
    is lr g / (|g| + eps), which saturates at +-lr, so an element with |g| near eps carries its gradient's rounding error at full weight
    and a small tensor cannot average that out; the bound was set for the buffer-wide figure.)"""
    from oracle import fno_oracle as O
    from tests import fno_checks as F
    g, m, v, p1 = (engine_tensors(eng, t) for t in (eng.gradients(), eng.exp_avg, eng.exp_avg_sq, eng.flat.data))
    res, got, ref = {}, [], []
    for k in g:
        want = F.flat_view(np.asarray(ref_grads[k])).astype(f64)
        res["g:" + k] = O.rel_nmse(g[k], want)
        p64, m64, v64 = flat0[k].astype(f64), np.zeros(want.size), np.zeros(want.size)
        O.adam_step(p64, coef * want, m64, v64, step, LR)
        res["m:" + k], res["v:" + k] = O.rel_nmse(m[k], m64), O.rel_nmse(v[k], v64)
        got.append(p1[k].astype(f64) - flat0[k])
        ref.append(p64 - flat0[k])
    res["delta"] = O.rel_nmse(np.concatenate(got), np.concatenate(ref))
    return res


def assert_step(res, name, what=""):
    gtol, atol = grad_tol(name), adam_tol()
    print("objective step", name, what, "worst g", max(v for k, v in res.items() if k[0] == "g"), "worst adam", max(v for k, v in res.items() if k[0] != "g"))
    bad = {k: v for k, v in res.items() if not (v <= (gtol if k[0] == "g" else atol))}
    assert not bad, (name, what, gtol, atol, bad)


def ref_norm(ref_grads, names):
    from tests import fno_checks as F
    return float(np.sqrt(sum(float(np.sum(F.flat_view(np.asarray(ref_grads[k])).astype(f64) ** 2)) for k in names)))


# ---- the row of the alignment table --------------------------------------------------------------------------------------------------
ALIGN_ROW = "objective"


def register_alignment_row():
    """The row of cfd_objective_fwd / cfd_objective_bwd in tests/align_checks.py's table (module docstring): check_placement, accepted when
    no output differs in a bit from the aligned run; each4 also on the emulator, as both launchers have an alignment gate.  Idempotent."""
    from tests import align_checks as A
    if ALIGN_ROW not in A.BY_ID:
        row = A.Row(ALIGN_ROW, check_placement, (), A.zero, emul_each=True)
        A.ROWS.append(row)
        A.BY_ID[row.id] = row
    return A.BY_ID[ALIGN_ROW]


if __name__ == "__main__":
    # (the row's check must be the importable module's function, not this script's copy of it: the table looks helpers up by module)
    from tests import align_checks as _A
    from tests import objective_checks as _OC
    _OC.register_alignment_row()
    sys.exit(_A.main(sys.argv[1:]))
