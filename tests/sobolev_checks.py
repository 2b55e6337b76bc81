"""Checks of the Sobolev objective: cfd_sobolev_fwd / cfd_sobolev_bwd (cfdbench_amd/csrc/sobolev.hip; include/cfdbench_amd.h, "Sobolev
objective").  Used by tests/test_emul_sobolev.py (CPU, SIMT emulator), tests/test_gpu_sobolev.py (MI355X), tests/test_cpu_sobolev.py (the
golden) and, through the row "sobolev" it adds to tests/align_checks.py's table, by the alignment files.  The C-ABI checks run on
tests/backends.py's hostile memory: poisoned outputs, guard bands, be.verify().

Reference: reference() below, fp64 NumPy (np.fft) on the same fp32 inputs, the rule of the header restated.

Bound.  The transform is fp32 products accumulated over up to 128 terms per stage, so objective.hip's 3 u does not carry over and no
fixed number is chosen here.  emulate() restates the kernels' arithmetic in NumPy -- the same fp32 tables, every output element as the
kernels form it (_Seg: segments of eight sequential fused multiply-adds in k order from a zero fp32 accumulator, the segments added in
fp64, one rounding to fp32), the same fp64 sums and coefficients, the same roundings of the spectrum's weight and of the term -- and its
error against reference() is what this arithmetic costs on these data.  A run is held to TWICE that figure plus a floor
for the final roundings (u = 2^-24): value 2 u (the fp32 rounding of the value, and the emulation's own), the fp64 quantities 2^-30, a
gradient element 4 u of |term| + |gadd| (the term's rounding and the addition).  Twice: the margin tests/conv_exact_checks.py gives
its kernels, which admits another order inside a chain but not a lost term.  CEILING = 1e-5, the project's parity budget, bounds value,
sums and the gradient however large the emulation's error is, and no shape may come near it.
The gradient figures: "grad", as tests/objective_checks.errors, is the worst element relative to |term| + |gadd|; a transform's error in
an element is proportional to the norm of its chains, not to the element, so for an element whose term nearly vanishes that figure is
unbounded by nature: it is held to twice the emulation's own, not to the ceiling.  "grad_img" is the worst element's error relative to the
largest |term| + |gadd| of its image, and the ceiling applies to it."""
from __future__ import annotations

import sys

import numpy as np

from cfdbench_amd._capi import CFD_HS_REC_FLOATS, CfdError
from tests.backends import POISON_WORD
from tests.objective_checks import VARIANTS, _bits, is_poison, load_f64, rel_err, same_bits

f64, f32 = np.float64, np.float32
U = 2.0 ** -24
CEILING = 1e-5
FLOOR = {"value": 2.0 * U, "value64": 2.0 ** -30, "sums": 2.0 ** -30, "grad": 4.0 * U, "grad_img": 4.0 * U}
# (k, a, group): the golden's three
SETTINGS = {"k1": (1, (1.0,), False), "k2": (2, (0.5, 0.25), False), "k2_grouped": (2, (1.0, 1.0), True)}
# (B, Co, H, W): the smallest grid; odd / odd; exactly one tile; one past a tile in both directions, odd; two 16-byte-unit-free sizes past
# four tiles; the FNO's default grid with 8 channels; the LDS maximum; an odd height below it
SHAPES = ((1, 1, 2, 2), (3, 2, 5, 7), (2, 3, 16, 16), (2, 2, 17, 33), (2, 2, 66, 65), (1, 8, 64, 64), (1, 2, 128, 128), (1, 1, 127, 128))
# (the emulator takes about four seconds for the seven variants at 128 x 128: every shape runs on both backends)
EMUL_SHAPES = SHAPES


def wave_r(H, W):
    """r(i, j) = kx(i)^2 + ky(j)^2 with the reference's wave numbers."""
    kx = np.array([i if i < H // 2 else H - i for i in range(H)], f64)
    ky = np.array([j if j < W // 2 else W - j for j in range(W)], f64)
    return kx[:, None] ** 2 + ky[None, :] ** 2


def coeffs(k, a):
    a = [1.0] * k if a is None else [float(f32(x)) for x in a]
    return [1.0, a[0] ** 2, (a[1] ** 2 if k >= 2 else 0.0)]


def _finish(Et, St, k, A, group, B):
    """value and, per sample, (scale, g0, g1, g2): the filter is scale (g0 + g1 r + g2 r^2).  Et, St: (3, B) fp64."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if group:
            terms = [np.sqrt(A[t] * Et[t]) / np.sqrt(A[t] * St[t]) for t in range(k + 1)]
            value = float(np.mean(sum(terms) / (k + 1)))
            den = B * (k + 1)
            c = [np.where(Et[t] == 0.0, 0.0, 1.0 / (den * np.sqrt(Et[t]) * np.sqrt(St[t]))) for t in range(3)]
            scale = c[0]
            g = [np.ones(B)] + [np.where((Et[t] == 0.0) | (scale == 0.0), 0.0, c[t] / scale) if t <= k else np.zeros(B) for t in (1, 2)]
        else:
            E = sum(A[t] * Et[t] for t in range(k + 1))
            S = sum(A[t] * St[t] for t in range(k + 1))
            value = float(np.mean(np.sqrt(E) / np.sqrt(S)))
            scale = np.where(E == 0.0, 0.0, 1.0 / (B * np.sqrt(E) * np.sqrt(S)))
            g = [np.full(B, A[t] if t <= k else 0.0) for t in range(3)]
    return value, scale, g


# ---- the reference -------------------------------------------------------------------------------------------------------------------
def reference(preds, label, mask, k=1, a=None, group=False, gadd=None, upstream=1.0):
    """fp64: dict(value, grad -- gadd included --, term, E, S: (3, B) each).  preds, label: (B, Co, H, W); mask: (B, H, W) or None."""
    p, lab = preds.astype(f64), label.astype(f64)
    lm = lab if mask is None else lab * mask.astype(f64)[:, None]
    d = p - lm
    B, Co, H, W = d.shape
    r = wave_r(H, W)
    Dh, Yh = np.fft.fft2(d), np.fft.fft2(lm)
    Et = np.stack([(r ** t * np.abs(Dh) ** 2).sum((1, 2, 3)) for t in range(3)])
    St = np.stack([(r ** t * np.abs(Yh) ** 2).sum((1, 2, 3)) for t in range(3)])
    A = coeffs(k, a)
    value, scale, g = _finish(Et, St, k, A, group, B)
    with np.errstate(invalid="ignore", over="ignore"):
        q = scale[:, None, None] * (g[0][:, None, None] + g[1][:, None, None] * r + g[2][:, None, None] * r * r)
        term = float(upstream) * (H * W) * np.real(np.fft.ifft2(q[:, None] * Dh))
    grad = term if gadd is None else gadd.astype(f64) + term
    return dict(value=value, grad=grad, term=term, E=Et, S=St)


# ---- the kernels' arithmetic in NumPy ------------------------------------------------------------------------------------------------
def _fma(x, y, acc):
    """fmaf: the product of two fp32 is exact in fp64; one rounding of the sum to fp32 (the rare double rounding aside)."""
    return (x.astype(f64) * y.astype(f64) + acc.astype(f64)).astype(f32)


class _Seg:
    """An output element of a stage as sobolev.hip holds it: an fp32 accumulator that takes a segment of eight fused multiply-adds from
    zero, and an fp64 sum of the segments; one rounding to fp32 at the end."""

    def __init__(self, shape):
        self.acc, self.sum = np.zeros(shape, f32), np.zeros(shape, f64)

    def fma(self, x, y):
        self.acc = _fma(x, y, self.acc)

    def flush(self):
        self.sum, self.acc = self.sum + self.acc.astype(f64), np.zeros_like(self.acc)

    def result(self):
        self.flush()
        return self.sum.astype(f32)


def _table(N):
    ang = 2.0 * np.pi * np.arange(N, dtype=f64) / N
    return np.cos(ang).astype(f32), np.sin(ang).astype(f32)


def _half_weights(H, W):
    """(n, r1, q1, paired) over the half spectrum (H, Wf): multiplicity, r of the element and of its mirror image (-i, W - l)."""
    Wf = W // 2 + 1
    r = wave_r(H, W)
    col = np.arange(Wf)
    paired = ~((col == 0) | (2 * col == W))
    r1 = r[:, :Wf]
    mi, ml = (-np.arange(H)) % H, (W - col) % W
    q1 = np.where(paired[None, :], r[mi][:, ml], 0.0)
    return np.where(paired, 2.0, 1.0)[None, :], r1, q1, paired[None, :]


def _spectrum(x):
    """Half spectrum of real images x (n, H, W) fp32 by the two stages of sobolev.hip: (re, im), fp32 (n, H, Wf)."""
    n, H, W = x.shape
    Wf = W // 2 + 1
    cw, sw = _table(W)
    ch, sh = _table(H)
    l = np.arange(Wf)
    pr, pi = _Seg((n, H, Wf)), _Seg((n, H, Wf))
    for y in range(W):  # stage W: y ascending, a segment of eight terms per flush
        idx = (y * l) % W
        xv = x[:, :, y][:, :, None]
        pr.fma(xv, cw[idx][None, None, :]), pi.fma(xv, -sw[idx][None, None, :])
        if y % 8 == 7:
            pr.flush(), pi.flush()
    pr, pi = pr.result(), pi.result()
    re, im = _Seg((n, H, Wf)), _Seg((n, H, Wf))
    rr = np.arange(H)
    for x0 in range(0, H, 4):  # stage H: per block of four x, cos P_re, then sin P_im (re); cos P_im, then -sin P_re (im); then the flush
        blk = range(x0, min(x0 + 4, H))
        for xx in blk:
            re.fma(ch[(rr * xx) % H][None, :, None], pr[:, xx, :][:, None, :])
        for xx in blk:
            re.fma(sh[(rr * xx) % H][None, :, None], pi[:, xx, :][:, None, :])
        for xx in blk:
            im.fma(ch[(rr * xx) % H][None, :, None], pi[:, xx, :][:, None, :])
        for xx in blk:
            im.fma(-sh[(rr * xx) % H][None, :, None], pr[:, xx, :][:, None, :])
        re.flush(), im.flush()
    return re.result(), im.result()


def _adjoint(zr, zi, W):
    """Re F^H of a weighted half spectrum (n, H, Wf) fp32 by the two stages backwards: fp32 (n, H, W)."""
    n, H, Wf = zr.shape
    cw, sw = _table(W)
    ch, sh = _table(H)
    ur, ui = _Seg((n, H, Wf)), _Seg((n, H, Wf))
    xs = np.arange(H)
    for r0 in range(0, H, 4):
        blk = range(r0, min(r0 + 4, H))
        for r in blk:
            ur.fma(ch[(xs * r) % H][None, :, None], zr[:, r, :][:, None, :])
        for r in blk:
            ur.fma(-sh[(xs * r) % H][None, :, None], zi[:, r, :][:, None, :])
        for r in blk:
            ui.fma(ch[(xs * r) % H][None, :, None], zi[:, r, :][:, None, :])
        for r in blk:
            ui.fma(sh[(xs * r) % H][None, :, None], zr[:, r, :][:, None, :])
        ur.flush(), ui.flush()
    ur, ui = ur.result(), ui.result()
    out = _Seg((n, H, W))
    ys = np.arange(W)
    for l in range(Wf):
        out.fma(ur[:, :, l][:, :, None], cw[(l * ys) % W][None, None, :])
        if l % 8 == 7:
            out.flush()
    out.flush()
    for l in range(Wf):
        out.fma(ui[:, :, l][:, :, None], -sw[(l * ys) % W][None, None, :])
        if l % 8 == 7:
            out.flush()
    return out.result()


def emulate(preds, label, mask, k=1, a=None, group=False, gadd=None, upstream=1.0):
    """The kernels' arithmetic (module docstring): dict(value -- fp64 --, value32, grad -- fp32 --, E, S)."""
    B, Co, H, W = preds.shape
    lm = label if mask is None else (label * mask[:, None]).astype(f32)
    d = (preds - lm).astype(f32)
    n, r1, q1, paired = _half_weights(H, W)
    dre, dim = _spectrum(d.reshape(B * Co, H, W))
    yre, yim = _spectrum(lm.reshape(B * Co, H, W))

    def sums(re, im):
        p = (re.astype(f64) ** 2 + im.astype(f64) ** 2).reshape(B, Co, H, -1)
        return np.stack([(n * p).sum((1, 2, 3)), ((r1 + q1) * p).sum((1, 2, 3)), ((r1 ** 2 + q1 ** 2) * p).sum((1, 2, 3))])

    Et, St = sums(dre, dim), sums(yre, yim)
    A = coeffs(k, a)
    value, scale, g = _finish(Et, St, k, A, group, B)
    gb = [np.repeat(x, Co)[:, None, None] for x in g]
    with np.errstate(invalid="ignore", over="ignore"):
        w = (gb[0] + gb[1] * r1 + gb[2] * r1 ** 2) + np.where(paired, gb[0] + gb[1] * q1 + gb[2] * q1 ** 2, 0.0)
        zr, zi = (w * dre.astype(f64)).astype(f32), (w * dim.astype(f64)).astype(f32)
        out = _adjoint(zr, zi, W).reshape(B, Co, H, W)
        term = (float(upstream) * scale[:, None, None, None] * out.astype(f64)).astype(f32)
    grad = term if gadd is None else (gadd + term).astype(f32)
    return dict(value=value, value32=f32(value), grad=grad, E=Et, S=St)


def case(B, Co, H, W, seed=0, masked=True):
    """Seeded inputs: a smooth field plus noise, so that every wave number carries energy, samples of different scale; preds (carrying
    the mask), label, a 0/1 mask with about a fifth of zeros (or None), gadd."""
    rng = np.random.default_rng(1000 * seed + 7 * B + 3 * Co + 131 * H + W)
    yy, xx = np.meshgrid(np.linspace(0, 1, H), np.linspace(0, 1, W), indexing="ij")
    smooth = np.sin(2 * np.pi * (xx + 0.3 * yy))[None, None] + 0.5 * np.cos(3 * np.pi * yy * xx)[None, None]
    scale = (1.0 + np.arange(B))[:, None, None, None]
    label = ((smooth + 0.3 * rng.standard_normal((B, Co, H, W))) * scale).astype(f32)
    preds = (label.astype(f64) + 0.2 * scale * (0.5 * smooth + rng.standard_normal((B, Co, H, W)))).astype(f32)
    mask = (rng.random((B, H, W)) > 0.2).astype(f32) if masked else None
    if masked:
        preds *= mask[:, None]
    gadd = rng.standard_normal((B, Co, H, W)).astype(f32)
    return preds, label, mask, gadd


# ---- the calls -----------------------------------------------------------------------------------------------------------------------
def _hs(setting):
    k, a, group = SETTINGS[setting] if isinstance(setting, str) else setting
    a = [1.0] * k if a is None else list(a)
    return int(k), float(a[0]), float(a[1]) if k >= 2 else 1.0, int(bool(group))


def call_fwd(be, preds, label, mask, rec, value, B, Co, H, W, k, a1, a2, balanced):
    P = be.ptr
    be.api.call("cfd_sobolev_fwd", P(preds), P(label), P(mask), P(rec), P(value), B, Co, H, W, k, a1, a2, balanced, be.stream)


def call_bwd(be, preds, label, mask, rec, gadd, updev, upstream, gpreds, B, Co, H, W, k, a1, a2, balanced):
    P = be.ptr
    be.api.call("cfd_sobolev_bwd", P(preds), P(label), P(mask), P(rec), P(gadd), P(updev), float(upstream), P(gpreds), B, Co, H, W, k, a1, a2,
                balanced, be.stream)


def run(be, shape, setting, masked=True, with_gadd=False, upstream=1.0, updev=None, alias=False, seed=0, data=None, twice=False, refs=True):
    """fwd + bwd on fresh hostile buffers; the arguments of tests/objective_checks.run.  Returns dict(value, rec, gpreds) as host arrays,
    `ref` (reference()) and `emu` (emulate()), both with the fp32 upstream values."""
    B, Co, H, W = shape
    hs = _hs(setting)
    preds, label, mask, gadd = data if data is not None else case(B, Co, H, W, seed, masked)
    if not with_gadd:
        gadd = None
    dp, dl = be.dev(preds), be.dev(label)
    dm = be.dev(mask) if mask is not None else None
    dg = be.dev(gadd) if gadd is not None else None
    du = be.dev(np.array([updev], f32)) if updev is not None else None
    rec, value = be.out((CFD_HS_REC_FLOATS(B, Co),)), be.out((1,))
    gp = dg if alias else be.out((B, Co, H, W))
    assert not alias or with_gadd
    for it in range(2 if twice else 1):
        if it and alias:
            if be.name == "gpu":
                gp.copy_(be.torch.from_numpy(gadd))
            else:
                gp[...] = gadd
        call_fwd(be, dp, dl, dm, rec, value, B, Co, H, W, *hs)
        call_bwd(be, dp, dl, dm, rec, dg, du, upstream, gp, B, Co, H, W, *hs)
        be.sync()
    up = float(f32(upstream)) * (float(f32(updev)) if updev is not None else 1.0)
    out = dict(value=be.host(value).copy(), rec=be.host(rec).copy(), gpreds=be.host(gp).copy())
    if refs:
        k, a, group = hs[0], hs[1:3][:hs[0]], bool(hs[3])
        out["ref"] = reference(preds, label, mask, k, a, group, gadd, up)
        out["emu"] = emulate(preds, label, mask, k, a, group, gadd, up)
    return out


def rec_sums(rec, B):
    """(E, S), (3, B) each, of the samples' records in rec."""
    E = np.array([[load_f64(rec, 2 + 12 * b + 2 * t) for b in range(B)] for t in range(3)])
    S = np.array([[load_f64(rec, 2 + 12 * b + 6 + 2 * t) for b in range(B)] for t in range(3)])
    return E, S


def _figures(value32, value64, E, S, grad, ref, with_gadd):
    want, term = ref["grad"], ref["term"]
    scale = np.abs(term) + (np.abs(want - term) if with_gadd else 0.0)
    err = np.abs(grad.astype(f64) - want)
    assert np.isfinite(grad).all() and (err[scale == 0.0] == 0.0).all()
    sums = max(max(rel_err(x, y) for x, y in zip(np.ravel(E), np.ravel(ref["E"]))), max(rel_err(x, y) for x, y in zip(np.ravel(S), np.ravel(ref["S"]))))
    top = scale.max(axis=(2, 3), keepdims=True)
    return dict(value=rel_err(value32, ref["value"]), value64=rel_err(value64, ref["value"]), sums=sums,
                grad=float(np.max(err[scale > 0.0] / scale[scale > 0.0], initial=0.0)),
                grad_img=float(np.max(np.where(top > 0.0, err / np.where(top > 0.0, top, 1.0), 0.0))))


def errors(res, shape, with_gadd):
    """(figures of the run, figures of the emulation), both against reference(): value, the fp64 value, the worst per-sample sum, the worst
    gradient element relative to |term| + |gadd|, and relative to the largest |term| + |gadd| of its image."""
    E, S = rec_sums(res["rec"], shape[0])
    got = _figures(res["value"][0], load_f64(res["rec"], 0), E, S, res["gpreds"], res["ref"], with_gadd)
    emu = res["emu"]
    return got, _figures(emu["value32"], emu["value"], emu["E"], emu["S"], emu["grad"], res["ref"], with_gadd)


def assert_within(figs, what):
    got, emu = figs
    print("sobolev", what, "run", {k: f"{v / U:.3g}u" for k, v in got.items()}, "emulation", {k: f"{v / U:.3g}u" for k, v in emu.items()})
    for key, v in got.items():
        assert v <= 2.0 * emu[key] + FLOOR[key], (what, key, v, emu[key])
        if key != "grad":
            assert v <= CEILING and 2.0 * emu[key] + FLOOR[key] <= CEILING, (what, key, v, emu[key])


def assert_rec_layout(rec, shape):
    B, Co = shape[:2]
    assert rec.size == CFD_HS_REC_FLOATS(B, Co) == 2 + 12 * B + 12 * B * Co and not (_bits(rec) == POISON_WORD).any()


# ---- (a) parity ----------------------------------------------------------------------------------------------------------------------
def check_parity(be, shape, setting, variants=None):
    """Every variant of tests/objective_checks.VARIANTS at one shape and setting: value, per-sample sums and every gradient element within
    the bound of the module docstring.  Returns {variant: (figures, the emulation's)}."""
    out = {}
    for name in variants or VARIANTS:
        masked, with_gadd, upstream, updev, alias = VARIANTS[name]
        res = run(be, shape, setting, masked, with_gadd, upstream, updev, alias)
        assert_rec_layout(res["rec"], shape)
        out[name] = errors(res, shape, with_gadd)
        assert_within(out[name], (be.name, shape, setting, name))
    return out


# ---- (b) determinism and placement ---------------------------------------------------------------------------------------------------
def _written(res):
    return [res["value"], res["rec"], res["gpreds"]]


def check_twice(be, shape, setting):
    """Two calls, the second on the first's dirty buffers: the same bits as one call on poisoned ones."""
    a = run(be, shape, setting, with_gadd=True, alias=True, updev=0.7, refs=False)
    b = run(be, shape, setting, with_gadd=True, alias=True, updev=0.7, twice=True, refs=False)
    return sum(not same_bits(x, y) for x, y in zip(_written(a), _written(b)))


def check_placement(be, shapes=((2, 2, 16, 20), (1, 2, 17, 33)), settings=("k1", "k2_grouped")):
    """Under the placement policy in force against every buffer on the 16-byte grid (the 16-byte loads where W % 4 == 0): the number of
    outputs -- value, rec, gpreds -- that differ in a bit.  The runs under the policy must also hold the bound."""
    bad = 0
    for shape in shapes:
        for setting in settings:
            for name in ("plain", "upstream_both_gadd_no_mask"):
                masked, with_gadd, upstream, updev, alias = VARIANTS[name]
                with be.misaligned(0):
                    ref = run(be, shape, setting, masked, with_gadd, upstream, updev, alias, refs=False)
                got = run(be, shape, setting, masked, with_gadd, upstream, updev, alias)
                assert_within(errors(got, shape, with_gadd), (be.name, shape, setting, name, "placed"))
                bad += sum(not same_bits(x, y) for x, y in zip(_written(ref), _written(got)))
    return bad


def check_misplaced(be, shape=(2, 2, 16, 20)):
    """Every buffer 4 and 8 bytes off the grid, and single buffers alone: the aligned bits."""
    bad = 0
    for setting in SETTINGS:
        with be.misaligned(0):
            ref = run(be, shape, setting, with_gadd=True, updev=0.7, refs=False)
        for shift, only in ((4, None), (8, None), (4, 0), (4, 1), (4, 2), (4, 3), (4, 5), (4, 7)):
            with be.misaligned(shift, only=only):
                got = run(be, shape, setting, with_gadd=True, updev=0.7, refs=False)
            bad += sum(not same_bits(x, y) for x, y in zip(_written(ref), _written(got)))
    return bad


# ---- (c) edges -----------------------------------------------------------------------------------------------------------------------
def check_exact_sample(be, shape=(3, 2, 9, 12)):
    """Sample 1's preds == label * mask exactly: its gradient is exactly 0 (with gadd: gadd's bits), the others hold the bound."""
    preds, label, mask, gadd = case(*shape, seed=3)
    preds[1] = label[1] * mask[1][None]
    for setting in SETTINGS:
        for with_gadd in (False, True):
            res = run(be, shape, setting, with_gadd=with_gadd, data=(preds, label, mask, gadd))
            g = res["gpreds"]
            assert same_bits(g[1], gadd[1] if with_gadd else np.zeros_like(g[1])), "the exact sample's gradient is not exactly 0"
            assert_within(errors(res, shape, with_gadd), (be.name, "exact sample", setting, with_gadd))
            assert np.any(res["ref"]["term"][0] != 0.0)


def check_zero_label(be, shape=(3, 2, 9, 12)):
    """Sample 1's label all zero: the value is not finite; the other samples' gradients are finite and within the bound, the zero
    sample's is not finite anywhere."""
    out = {}
    for setting in SETTINGS:
        preds, label, mask, gadd = case(*shape, seed=4)
        label[1] = 0.0
        res = run(be, shape, setting, data=(preds, label, mask, gadd))
        g, want, emu = res["gpreds"], res["ref"]["grad"], res["emu"]["grad"]
        assert not np.isfinite(res["value"][0]) and not np.isfinite(res["ref"]["value"]), (setting, res["value"])
        rest = [0, 2]
        assert np.isfinite(g[rest]).all() and not np.isfinite(g[1]).any(), setting
        top = np.abs(want[rest]).max(axis=(2, 3), keepdims=True)
        fig = float(np.max(np.abs(g[rest].astype(f64) - want[rest]) / top))
        bound = 2.0 * float(np.max(np.abs(emu[rest].astype(f64) - want[rest]) / top)) + FLOOR["grad_img"]
        assert fig <= bound <= CEILING, (setting, fig, bound)
        out[setting] = fig
    return out


def _status(call):
    try:
        call()
        return 0
    except CfdError as e:
        return int(str(e).split("(status ")[1].split(")")[0])


def check_refusals(be, shape=(2, 2, 8, 8)):
    """{what: (status, every buffer kept its bits)}: k outside {1, 2}, balanced outside {0, 1}, B / Co < 1, NULL required pointers: -1
    (CFD_ERR_INVALID_ARG); a grid outside 2 .. 128: -2 (CFD_ERR_UNSUPPORTED)."""
    B, Co, H, W = shape
    preds, label, mask, gadd = case(B, Co, H, W, seed=5)
    dp, dl, dm, dg = be.dev(preds), be.dev(label), be.dev(mask), be.dev(gadd)
    rec, value, gp = be.out((CFD_HS_REC_FLOATS(B, Co),)), be.out((1,)), be.out((B, Co, H, W))
    good = be.out((CFD_HS_REC_FLOATS(B, Co),))
    call_fwd(be, dp, dl, dm, good, be.out((1,)), B, Co, H, W, 1, 1.0, 1.0, 0)
    be.sync()
    good0 = be.host(good).copy()

    def kept():
        be.sync()
        return (is_poison(be.host(rec)) and is_poison(be.host(value)) and is_poison(be.host(gp)) and same_bits(be.host(good), good0)
                and same_bits(be.host(dp), preds) and same_bits(be.host(dl), label) and same_bits(be.host(dg), gadd))

    res = {}
    hs = (1, 1.0, 1.0, 0)
    fwd = dict(k0=(dp, dl, dm, rec, value, B, Co, H, W, 0, 1.0, 1.0, 0), k3=(dp, dl, dm, rec, value, B, Co, H, W, 3, 1.0, 1.0, 0),
               balanced=(dp, dl, dm, rec, value, B, Co, H, W, 1, 1.0, 1.0, 2), B=(dp, dl, dm, rec, value, 0, Co, H, W, *hs),
               Co=(dp, dl, dm, rec, value, B, 0, H, W, *hs), preds=(None, dl, dm, rec, value, B, Co, H, W, *hs),
               label=(dp, None, dm, rec, value, B, Co, H, W, *hs), rec=(dp, dl, dm, None, value, B, Co, H, W, *hs),
               value=(dp, dl, dm, rec, None, B, Co, H, W, *hs), H1=(dp, dl, dm, rec, value, B, Co, 1, W, *hs),
               W129=(dp, dl, dm, rec, value, B, Co, H, 129, *hs), H_neg=(dp, dl, dm, rec, value, B, Co, -8, W, *hs))
    for name, a in fwd.items():
        res["fwd:" + name] = (_status(lambda: call_fwd(be, *a)), kept())
    b0 = (dp, dl, dm, good, dg, None, 1.0, gp)
    bwd = dict(k0=(*b0, B, Co, H, W, 0, 1.0, 1.0, 0), balanced=(*b0, B, Co, H, W, 2, 1.0, 1.0, -1), B=(*b0, -1, Co, H, W, *hs),
               Co=(*b0, B, 0, H, W, *hs), preds=(None, dl, dm, good, dg, None, 1.0, gp, B, Co, H, W, *hs),
               label=(dp, None, dm, good, dg, None, 1.0, gp, B, Co, H, W, *hs), rec=(dp, dl, dm, None, dg, None, 1.0, gp, B, Co, H, W, *hs),
               gpreds=(dp, dl, dm, good, dg, None, 1.0, None, B, Co, H, W, *hs), H129=(*b0, B, Co, 129, W, *hs), W1=(*b0, B, Co, H, 1, *hs))
    for name, a in bwd.items():
        res["bwd:" + name] = (_status(lambda: call_bwd(be, *a)), kept())
    return res


def expected_refusals(res):
    """The statuses check_refusals must report."""
    return {name: (-2 if name.split(":")[1] in ("H1", "W129", "H_neg", "H129", "W1") else -1, True) for name in res}


def check_parseval(be, shape=(3, 2, 17, 33)):
    """a1 = 0, k = 1, not grouped is rel_l2 (Parseval): cfd_sobolev_fwd's value against cfd_objective_fwd's on the same buffers, within
    the Sobolev bound of that shape plus rel_l2's own 3 u.  Returns (figure, bound)."""
    from cfdbench_amd._capi import CFD_OBJ_REC_FLOATS, OBJECTIVE_IDS
    B, Co, H, W = shape
    preds, label, mask, gadd = case(B, Co, H, W, seed=6)
    dp, dl, dm = be.dev(preds), be.dev(label), be.dev(mask)
    rec, value = be.out((CFD_HS_REC_FLOATS(B, Co),)), be.out((1,))
    orec, ovalue = be.out((CFD_OBJ_REC_FLOATS(B, Co),)), be.out((1,))
    call_fwd(be, dp, dl, dm, rec, value, B, Co, H, W, 1, 0.0, 1.0, 0)
    P = be.ptr
    be.api.call("cfd_objective_fwd", P(dp), P(dl), P(dm), P(orec), P(ovalue), B, Co, H * W, OBJECTIVE_IDS["rel_l2"], be.stream)
    be.sync()
    hs, l2 = float(be.host(value)[0]), float(be.host(ovalue)[0])
    ref = reference(preds, label, mask, 1, (0.0,), False)
    emu = emulate(preds, label, mask, 1, (0.0,), False)
    bound = 2.0 * rel_err(emu["value32"], ref["value"]) + FLOOR["value"] + 3.0 * U
    return rel_err(hs, l2), bound


# ---- (e) the whole model: FnoTrainEngine(objective="hs") against the fp64 chain -----------------------------------------------------------
# The cases, the tolerances (grad_tol, adam_tol, VALUE_TOL) and compare_step / assert_step are tests/objective_checks.py's: the Sobolev
# gradient enters the same backward pass through the same argument, so the routes hold what they hold there.
def hs_kwargs(setting):
    k, a, group = SETTINGS[setting]
    return dict(k=k, a=tuple(a), group=group)


def ref_pass(params, batch, s, setting, label=None, inputs=None, gadd=None, upstream=1.0):
    """tests/objective_checks.ref_pass with reference() of this module as the objective: oracle.fno_forward -> reference() ->
    oracle.fno_backward; a padded shape takes tests/ingrad_checks.py's fp64 forward pass and autograd as its adjoint."""
    from oracle import fno_oracle as O
    x = batch["inputs"] if inputs is None else inputs
    lab = batch["label"] if label is None else label
    B = lab.shape[0]
    mask3 = batch["mask"].reshape(B, *lab.shape[2:])
    k, a, group = SETTINGS[setting]

    def objective(preds):
        o = reference(preds, lab, mask3, k, a, group, None if gadd is None else np.asarray(gadd), upstream)
        return o["value"], o["grad"]

    if s["pad"] == 0:
        p64 = {q: v.astype(np.complex128 if np.iscomplexobj(v) else f64) for q, v in params.items()}
        fw = O.fno_forward(p64, x.astype(f64), batch["case_params"].astype(f64), batch["mask"].astype(f64), lab.astype(f64), s["L"])
        value, G = objective(fw["preds"])
        g = O.fno_backward(p64, fw["cache"], G, s["L"])
        g_inputs = g.pop("__inputs__")
        return dict(preds=fw["preds"], value=value, grads=g, g_inputs=g_inputs)
    import torch

    from tests import ingrad_checks as IC
    tp, tb = IC._leaves(params, dict(batch, inputs=np.asarray(x)))
    preds = IC.ref_forward(tp, tb["inputs"], tb["case_params"], tb["mask"], s["L"], s["pad"])
    value, G = objective(preds.detach().numpy())
    (preds * torch.from_numpy(G)).sum().backward()
    return dict(preds=preds.detach().numpy(), value=value, grads={q: v.grad.numpy() for q, v in tp.items()}, g_inputs=tb["inputs"].grad.numpy())


def ref_window(params, batch, s, setting, labels_seq):
    """tests/objective_checks.ref_window on ref_pass of this module."""
    K_ = len(labels_seq)
    xs, fw = [batch["inputs"]], []
    for i in range(K_):
        fw.append(ref_pass(params, batch, s, setting, labels_seq[i], xs[i]))
        xs.append(fw[i]["preds"])
    total, gadd = None, None
    for i in range(K_ - 1, -1, -1):
        r = ref_pass(params, batch, s, setting, labels_seq[i], xs[i], gadd=gadd, upstream=1.0 / K_)
        gadd = r["g_inputs"]
        total = r["grads"] if total is None else {q: total[q] + r["grads"][q] for q in total}
    return dict(grads=total, values=[f["value"] for f in fw], preds=[f["preds"] for f in fw])


def make_model(params, s, setting=None):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import objective_to_fn
    loss = objective_to_fn("nmse") if setting is None else objective_to_fn("hs", **hs_kwargs(setting))
    model = Fno2d(s["cin"], s["cout"], s["p"], loss, s["L"], s["m1"], s["m2"], s["C"], padding=s["pad"] or None).cuda()
    model.load_state_dict({q: torch.from_numpy(np.ascontiguousarray(v)) for q, v in params.items()})
    return model


def make_engine(params, s, setting, **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    from tests.objective_checks import LR, Counting
    eng = FnoTrainEngine(make_model(params, s), lr=LR, loss_name="nmse", objective="hs", **{"hs_" + q: v for q, v in hs_kwargs(setting).items()}, **kw)
    eng.api = Counting(eng.api)
    return eng


# ---- the row of the alignment table --------------------------------------------------------------------------------------------------
ALIGN_ROW = "sobolev"


def register_alignment_row():
    """The row of cfd_sobolev_fwd / cfd_sobolev_bwd in tests/align_checks.py's table: check_placement, accepted when no output differs
    in a bit from the aligned run; each4 also on the emulator, as both launchers have an alignment gate.  Idempotent."""
    from tests import align_checks as A
    if ALIGN_ROW not in A.BY_ID:
        row = A.Row(ALIGN_ROW, check_placement, (), A.zero, emul_each=True)
        A.ROWS.append(row)
        A.BY_ID[row.id] = row
    return A.BY_ID[ALIGN_ROW]


if __name__ == "__main__":
    # (the row's check must be the importable module's function, not this script's copy of it: the table looks helpers up by module)
    from tests import align_checks as _A
    from tests import sobolev_checks as _SC
    _SC.register_alignment_row()
    sys.exit(_A.main(sys.argv[1:]))
