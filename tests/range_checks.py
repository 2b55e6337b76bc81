"""Checks of the FNO over the whole range of grids and mode counts cfd_plan_create accepts (2 <= H, W <= 128, 1 <= m1, 2 m1 <= H,
1 <= m2 <= W/2 + 1), at the shapes where cfdbench_amd/csrc/spectral.hip changes kernel: one table (SHAPES) with a row for every
kernel family and the edge it is there for, and a seeded sweep over the range.  Built on the shared helpers of tests/kernel_checks.py,
tests/modes_checks.py and tests/fno_checks.py; every figure is against the fp64 oracle, at the bound the existing tests of the same
kernel family use (EXACT_TOL on the three-piece split-bf16 kernels, K.TOL on the generic exact-fp32 ones and on dft_many.hip).  Used by tests/test_emul_range.py (CPU, SIMT
emulator) and tests/test_gpu_range.py (MI355X).

What a narrow plan (m1 <= 15, m2 <= 16, W <= 80) derives from its shape (plan.cpp): KX = ceil((H/2 + 1) / 4) k-steps of folded rows in the
forward transform, T = ceil(H / 16) row tiles in the inverse, SA = 4 + ceil(m1 / 4) and SB = ceil(2 m2 / 4) k-steps of its two stages,
NJ = max(4, ceil(W / 16)) columns per lane in the generic kernels, NJG = ceil(W / 16) column tiles in the general-width ones."""
from __future__ import annotations

import ctypes

import numpy as np

from cfdbench_amd._capi import CfdError, FnoShape
from oracle import synth
from tests import backends as BK
from tests import fno_checks as F
from tests import grid_checks as G
from tests import kernel_checks as K
from tests import modes_checks as MK

nm = K.nm

# (H, W, m1, m2)
SHAPES = [
    # ---- generic exact-fp32 k_dft_fwd / k_idft: the only transforms of a narrow plan with H > 70 (80 where k_idft64 applies) ----
    (128, 64, 12, 12),   # KX = 17, T = 8, float4 rows: the tallest grid at the default modes, s_tab of both kernels exactly full
    (96, 64, 12, 12),    # KX = 13, T = 6, float4 rows
    (81, 64, 12, 12),    # KX = 11, T = 6 with one row in the last tile (x >= H in fifteen of its sixteen rows)
    (112, 32, 12, 12),   # KX = 15, T = 7, float4 rows with half the lanes past the row (4 n >= W)
    (83, 50, 12, 12),    # KX = 11, T = 6, scalar loads (W % 4 != 0), y >= W inside a lane's four columns
    (100, 30, 15, 16),   # KX = 13, T = 7, scalar loads, full modes (SA = SB = 8) and the Nyquist column (m2 = W/2 + 1)
    (128, 2, 1, 2),      # KX = 17, T = 8 on the narrowest grid: one lane holds a row; m1 = 1; the Nyquist column
    (95, 70, 13, 5),     # NJ = 5, KX = 12, T = 6, unequal modes
    (111, 77, 7, 16),    # NJ = 5, KX = 14, T = 7
    (127, 79, 15, 16),   # NJ = 5, KX = 16, T = 8, full modes, nothing a multiple of 4
    (128, 80, 15, 16),   # NJ = 5, KX = 17, T = 8: every extent of the narrow route at its maximum
    # ---- the narrow route's maxima m1 = 15, m2 = 16 (kap = lane & 15 and the e - 15 sine block full, SA = SB = 8, CFD_DFT_OS and
    #      CFD_IDFT_ZMAX exactly full) on each family that serves H <= 70; 961 staged floats are too many for k_idft64 / k_block ----
    (64, 64, 15, 16),    # k_dft_fwd64_b3, k_idft_g<4>, FnoBlock in two passes
    (66, 65, 15, 16),    # k_dft_fwd_g<5>, k_idft_g<5>
    (70, 80, 15, 16),    # the largest grid of the general-width family; the seam to (70, 81, 3, 4)
    (48, 64, 15, 16),    # k_dft_fwd_g<4>; W = 64 and H % 16 == 0, yet k_idft_g<4> (the modes decide)
    (30, 30, 15, 16),    # NJG = 2; 2 m1 == H and the Nyquist column at once
    # ---- the Nyquist column on the narrow route (weight 1, not 2, in the inverse tables and the spectral weight gradient) ----
    (16, 16, 8, 9),      # NJG = 1, even W, 2 m1 == H
    (31, 17, 15, 9),     # odd W: m2 = (W + 1) / 2 is the last column and has weight 2
    # ---- unequal and minimal modes ----
    (64, 64, 13, 3),     # the 64-wide kernels (k_dft_fwd64_b3, k_idft64, k_block) at m1 > m2
    (64, 64, 1, 1),      # ... at one mode: SA = 5, SB = 1
    (66, 65, 3, 14),     # the general-width kernels and k_block's general form at m1 < m2
    # ---- NJG = 1, 2, 3 and the smallest plans (fewer rows than one MFMA k-step, fewer than 64 pixels per image) ----
    (5, 7, 2, 4),        # NJG = 1, odd H and W
    (24, 24, 12, 12),    # NJG = 2, 2 m1 == H
    (30, 48, 12, 12),    # NJG = 3
    (2, 2, 1, 2),        # the smallest plan: every row is its own mirror, the Nyquist column
    (2, 3, 1, 1),
    (3, 2, 1, 2),
    # ---- k_idft64 (W = 64, H % 16 == 0, H <= 80) at its two ends ----
    (16, 64, 8, 12),     # T = 1, 2 m1 == H
    (80, 64, 12, 12),    # T = 5 = CFD_KB_TMAX; H > 70: the forward transform is the generic one (KX = 11)
    # ---- k_block's general form (64 <= W <= 68, H <= 80) at the ends of its range, and just outside it ----
    (80, 68, 12, 12),    # E = 4 tail columns, T = 5
    (80, 68, 15, 16),    # the same grid at full modes: over CFD_BLK_ZS, so two passes with k_idft<5> at T = 5
    (72, 66, 12, 12),    # E = 2, T = 5 with a half-empty last tile
    (64, 67, 12, 12),    # E = 3 on whole tiles
    (64, 69, 12, 12),    # W = 69: no 64-column tables, two passes with k_idft_g<5>
    (63, 64, 12, 12),    # W = 64 but H % 16 != 0: k_block's general form, k_idft_g<4> in place of k_idft64
    # ---- the seam to the many-modes plan (dft_many.hip), both sides ----
    (70, 81, 3, 4),      # W = 81 at narrow mode counts
    (32, 34, 15, 16),    # NJG = 3 at full narrow modes
    (32, 34, 16, 17),    # one mode more each way: many-modes, 2 m1 == H
]
assert len(set(SHAPES)) == len(SHAPES)

BLOCK_CHANNELS = (20, 25, 32)      # the three k_block chunkings of tests/test_gpu_block_mix.py
WIDE_CHANNELS = 40                 # above 32: the two-pass wide route
MODEL_CHANNELS = (8, 24, 25, 33)
BF16_SHAPES = [(24, 24, 12, 12), (30, 48, 12, 12), (25, 33, 12, 12), (70, 80, 12, 12), (12, 16, 6, 8)]  # NJG = 2, 3, 3, 5, 1
LOOP_WRAP = (16500, 81, 8, 3, 4)   # (images, plan): more than twice the 4 waves x 2048 workgroups k_dft_fwd launches at most


EXACT_TOL = 2e-13  # the fp32-exact class of the three-piece split-bf16 kernels (tests/test_{gpu,emul}_kernels.py, which pin it at 64 x 64
#                    and 66 x 65): two pieces cost 2e-11 .. 5e-11, so K.TOL alone would let an instantiation that dropped a piece pass


def is_block_grid(H, W):
    """The grids with 64-column inverse tables (k_idft64, k_block)."""
    return 64 <= W <= 68 and H <= 80


def few_modes(m1, m2):
    """The staged mode vector of k_idft64 / k_block holds 4 m1 m2 <= 576 floats (CFD_BLK_ZS)."""
    return 4 * m1 * m2 <= 576


def idft64_applies(H, W, m1, m2):
    return W == 64 and H % 16 == 0 and H <= 80 and few_modes(m1, m2)


def reaches_k_block(H, W, m1, m2, C, B=2):
    """block_fused_ok (spectral.hip) at the default knobs: up to 24 channels on every grid with 64-column tables, 25 .. 32 on the
    64-wide whole-tile grids at any batch and on the others from 128 entries."""
    if not is_block_grid(H, W) or not few_modes(m1, m2) or C > 32:
        return False
    return C <= 24 or (W == 64 and H % 16 == 0) or B >= 128


def split_bf16_transforms(H, W, m1, m2):
    """Both default transforms of the plan are three-piece split-bf16 kernels (k_dft_fwd64_b3 / k_dft_fwd_g, k_idft64 / k_idft_g)."""
    return not G.is_many(W, m1, m2) and H <= 70


def block_tol(H, W, m1, m2, C):
    """EXACT_TOL where the FnoBlock runs on three-piece kernels alone: k_block, or k_chanmix_b3 + k_idft64 / k_idft_g.  K.TOL where
    its inverse transform is the generic exact-fp32 k_idft or dft_many.hip's, as the existing tests of those hold them."""
    if G.is_many(W, m1, m2):
        return K.TOL
    return EXACT_TOL if H <= 70 or reaches_k_block(H, W, m1, m2, C) or idft64_applies(H, W, m1, m2) else K.TOL


def border_of(H, W):
    """synth.make_batch's border mask zeroes the first and last row and the first column: on a grid with H < 3 or W < 3 it leaves at
    most one pixel (none at 2 x 2 and 2 x 3), and the oracle's nMSE is then 0/0.  Those grids run with the mask of ones."""
    return H >= 3 and W >= 3


def _prefixed(prefix, res):
    return {f"{prefix}:{k}": v for k, v in res.items()}


def routes(H, W, m1, m2):
    """The knob settings that change which transform kernels serve the plan.  general_b3 = 0 swaps the general-width kernels
    (H <= 70, unless both directions are 64-wide ones) for the generic exact-fp32 k_dft_fwd / k_idft; exact_fp32 = 1 swaps the 64-wide
    ones too.  A narrow plan above 70 rows runs the generic kernels whatever the knobs say -- but for k_idft64 up to 80 rows -- and a
    many-modes plan has no knob: running those again would report one family under three names."""
    out = ["default"]
    if not G.is_many(W, m1, m2):
        if H <= 70 and not ((H, W) == (64, 64) and few_modes(m1, m2)):
            out.append("general_b3=0")
        if H <= 70 or idft64_applies(H, W, m1, m2):
            out.append("exact_fp32=1")
    return out


def check_transforms(be, H, W, m1, m2):
    """K.check_spectral (B = 3, Cin = 3, Cout = 2) and K.check_idft_epilogues (5 images) on every route of routes(): each family that
    can serve the shape is held to the oracle."""
    res = {}
    for route in routes(H, W, m1, m2):
        knob, _, value = route.partition("=")
        with K.tuned(be, **({knob: int(value)} if value else {})):
            res.update(_prefixed(route + ":spectral", K.check_spectral(be, 3, 3, 2, H, W, m1, m2)))
            res.update(_prefixed(route + ":idft", K.check_idft_epilogues(be, 5, H, W, m1, m2)))
    return res


def check_block(be, H, W, m1, m2, C):
    """cfd_fno_block_fwd / cfd_fno_block_bwd_input at B = 2 and C channels each way."""
    return K.check_block(be, 2, C, C, H, W, m1, m2)


def check_model(be, H, W, m1, m2, C):
    """The whole model (B = 2, two layers): predictions from the training and inference workspaces, the nMSE loss, every parameter
    gradient.  (MK.oracle_step asserts that the oracle's own loss and gradients are finite.)"""
    return MK.check_fno_vs_oracle(be, 2, C, 2, H, W, m1, m2, border=border_of(H, W))


def check_step(be, H, W, m1, m2, C, B=2, L=2, p=5, pseed=27, bseed=28):
    """One fused training step (cfd_fno_forward_train_f / cfd_fno_backward_phase_f / cfd_fno_adam_step) with flags = 0: the flat gradient
    against the oracle, slice by slice.  Then the comparison of the deferral tests over two steps, flags = 7 against flags = 0.  Where the
    route defers (narrow plan, C <= 32: fno.cpp, route()) that is K.check_fno_train_step_deferred's: the raw gradient of flags = 7 lacks the
    nMSE normaliser until cfd_fno_adam_step has run, so it is rescaled by n / sum (label * mask)^2 before it is compared.  Elsewhere every
    flag is ignored and the two runs are bitwise equal (MK.check_train_step_deferred's claim)."""
    params = synth.make_fno_params(pseed, C, L, m1, m2, p, spectral_gain=4.0)
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=border_of(H, W))
    _ref, rg = MK.oracle_step(params, batch, L, "nmse")
    out, layout = F.run_fused_steps(be, params, batch, L, C, H, W, p, m1, m2, which="nmse", flags=7, steps=2)
    a, b = out[0], out[7]
    res = {"oracle:" + k: nm(F.flat_slice(a["g1"], layout, k), F.flat_view(rg[k])) for k in layout}
    if C <= 32 and not G.is_many(W, m1, m2):
        g7 = b["g1"] * (b["sums1"][3] / b["sums1"][2])
        res.update({"params": nm(b["flat"], a["flat"]), "preds": nm(b["preds1"], a["preds1"]), "grad_vs_immediate": nm(g7, a["g1"]),
                    "sums": float(np.max(np.abs(b["sums1"] - a["sums1"]) / np.abs(a["sums1"])))})
        res.update({"deferred:" + k: nm(F.flat_slice(g7, layout, k), F.flat_view(rg[k])) for k in layout})
    else:
        res["bitwise"] = K.nan_max(*[np.max(np.abs(a[k] - b[k])) for k in ("flat", "g1", "sums1", "preds1")])
    return res


def check_bf16(be, H, W, m1=12, m2=12):
    """bf16 activation storage (cfd_fno_forward_ex, act_dtype = 1) against the oracle with the same storage rule, at B = 2, C = 8, L = 2."""
    return K.check_fno_bf16_storage(be, 2, 8, 2, H, W, m1=m1, m2=m2)


def check_bf16_refusal(be, H=72, W=64, m1=12, m2=12, B=1, C=8, L=1, p=5):
    """bf16 activation storage needs the general-width transforms, so H <= 70: on a taller narrow plan the inference forward and the
    training step return CFD_ERR_UNSUPPORTED before anything is launched -- predictions, sums and the workspace still hold the poison."""
    api, P = be.api, be.ptr
    params = synth.make_fno_params(3, C, L, m1, m2, p)
    batch = synth.make_batch(4, B, H, W, p)
    plan = api.plan_create(H, W, m1, m2)
    try:
        shape = FnoShape(B, H, W, 2, 2, p, C, L, m1, m2, 128)
        pd = {k: be.dev(v) for k, v in params.items()}
        gd = {k: be.out(v.shape, np.complex64 if np.iscomplexobj(v) else np.float32) for k, v in params.items()}
        sh, pr, gr = ctypes.byref(shape), ctypes.byref(F.make_param_struct(be, pd, L)), ctypes.byref(F.make_param_struct(be, gd, L))
        di, dc, dm, dl = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask", "label"))
        ws = be.scratch(api.size("cfd_fno_workspace_bytes_ex", plan, sh, 1, 0))
        preds, sums, coef = be.out((B, 2, H, W)), be.out((4,)), be.out((2,))

        def untouched():
            be.sync()
            bufs = [preds, sums, coef, ws[:ws.shape[0] // 4 * 4], *gd.values()]
            return all((be.host(t).reshape(-1).view(np.uint32) == BK.POISON_WORD).all() for t in bufs)

        res = {}
        for name, fn, args in (("forward", "cfd_fno_forward_ex", (plan, sh, pr, P(di), P(dc), P(dm), P(dl), P(preds), P(sums), P(ws), 0, 1,
                                                                 be.stream)),
                               ("train", "cfd_fno_forward_train_ex", (plan, sh, pr, gr, P(di), P(dc), P(dm), P(dl), P(preds), P(sums), P(coef),
                                                                      P(ws), 1, 1.0, 1, be.stream))):
            try:
                api.call(fn, *args)
                res[name + " refused as unsupported"] = False
            except CfdError as e:
                res[name + " refused as unsupported"] = "(status -2)" in str(e)
            res[name + " left every buffer untouched"] = untouched()
        return res
    finally:
        api.plan_destroy(plan)


def sweep_plans(n=120, seed=2026):
    """`n` plans drawn from the whole accepted range, a quarter from each of: narrow with H <= 70, narrow with H > 70, many-modes with
    W <= 80, many-modes with W > 80; in every quarter a third of the draws has the last column the grid admits, m2 = W/2 + 1."""
    rng = np.random.default_rng(seed)

    def ri(lo, hi):
        return int(rng.integers(lo, hi + 1))

    plans = []
    for i in range(n):
        quarter, last = i % 4, (i // 4) % 3 == 0
        if quarter < 2:
            H = ri(2, 70) if quarter == 0 else ri(71, 128)
            W = ri(2, 31) if last else ri(2, 80)  # (m2 = W/2 + 1 <= 16)
            m1 = ri(1, min(15, H // 2))
            m2 = W // 2 + 1 if last else ri(1, min(16, W // 2 + 1))
        elif quarter == 2:
            if ri(0, 1):  # many rows ...
                H, W = ri(32, 128), ri(2, 80)
                m1 = ri(16, H // 2)
                m2 = W // 2 + 1 if last else ri(1, W // 2 + 1)
            else:         # ... or many columns
                H, W = ri(2, 128), ri(32, 80)
                m1 = ri(1, H // 2)
                m2 = W // 2 + 1 if last else ri(17, W // 2 + 1)
        else:
            H, W = ri(2, 128), ri(81, 128)
            m1 = ri(1, H // 2)
            m2 = W // 2 + 1 if last else ri(1, W // 2 + 1)
        assert 2 <= H <= 128 and 2 <= W <= 128 and 1 <= m1 and 2 * m1 <= H and 1 <= m2 <= W // 2 + 1, (H, W, m1, m2)
        assert G.is_many(W, m1, m2) == (quarter >= 2), (H, W, m1, m2)
        plans.append((H, W, m1, m2))
    return plans


SWEEP = sweep_plans()


# ---- what the tests of both files assert: the project's bounds, NaN-safe ------------------------------------------------------
def assert_all(res, tol=K.TOL, what=""):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"{what}parity failures (tol {tol}): {bad}; all: {res}"


def assert_model(res, what=""):
    """K.TOL on every tensor; the scalar loss at the bound of every whole-model test (fp32 sums: 1e-5)."""
    res = dict(res)
    loss = res.pop("nmse_loss")
    assert loss < 1e-5, f"{what}nmse_loss {loss}; all: {res}"
    assert_all(res, K.TOL, what)


def assert_step(res, what=""):
    """K.TOL on every gradient slice; the two-step comparison at the bounds of its existing tests (tests/test_gpu_kernels.py:
    test_fused_train_step_with_deferred_launches; tests/test_gpu_fno_modes.py: test_fused_train_step_modes_ignores_deferrals)."""
    res = dict(res)
    if "bitwise" in res:
        v = res.pop("bitwise")
        assert v == 0.0, f"{what}flags = 7 and flags = 0 differ by {v} where nothing is deferred; all: {res}"
    else:
        sums, preds = res.pop("sums"), res.pop("preds")
        assert sums < 1e-6 and preds == 0.0, f"{what}sums {sums}, preds {preds}; all: {res}"
        assert_all({k: res.pop(k) for k in ("params", "grad_vs_immediate")}, 1e-11, what)
    assert_all(res, K.TOL, what)


def assert_transforms(res, H, W, m1, m2, what=""):
    """The default route at EXACT_TOL where both its transforms are three-piece split-bf16 kernels; K.TOL on the generic exact-fp32
    kernels (H > 70, the knob routes) and on many-modes plans, as their existing tests hold them."""
    exact = {k: v for k, v in res.items() if k.startswith("default:")} if split_bf16_transforms(H, W, m1, m2) else {}
    assert_all(exact, EXACT_TOL, what)
    assert_all({k: v for k, v in res.items() if k not in exact}, K.TOL, what)


def assert_bf16(res, what=""):
    """What tests/test_gpu_kernels.py: test_bf16_activation_storage_forward asserts, but for its last line.  That one -- the price of
    the storage format lies in (1e-7, 1e-3): visible, and small -- is a statement about the input as much as about the kernels: at
    (12, 16) with 6 x 8 modes the ORACLE's two storage rules are 5.3e-8 apart.  Here the price must be the one the oracle pays, within a
    factor of two: both apply the same rounding to values that agree to 1e-7, and a path that stored fp32 after all would pay exactly
    nothing.  The upper end stays."""
    res = dict(res)
    info = {k: v for k, v in res.items() if k.startswith("info:")}
    loss = res.pop("bf16_loss")
    assert loss < 1e-5, f"{what}bf16_loss {loss}"
    assert_all({k: v for k, v in res.items() if not k.startswith("info:")}, 1e-7, what)
    price, oracle_price = info["info:bf16_vs_f32"], info["info:oracle_bf16_vs_f32"]
    assert 0.0 < oracle_price and 0.5 * oracle_price < price < 2.0 * oracle_price and price < 1e-3, f"{what}{info}"
