"""Checks of the FNO on grids wider than 80 columns (up to 128 x 128: many-modes plans whatever their mode counts,
cfdbench_amd/csrc/dft_many.hip) that the shared helpers of tests/kernel_checks.py and tests/modes_checks.py do not have: the LDS figure of
the transforms, the plan's range, one misaligned run.  Used by tests/test_emul_fno_grid.py (CPU, SIMT emulator) and
tests/test_gpu_fno_grid.py (MI355X)."""
from __future__ import annotations

from tests import kernel_checks as K
from tests import modes_checks as MK

LDS_CAP = 163840  # the 160 KB of LDS of a CU: what a workgroup may ask for

# (H, W, m1, m2)
SHAPES = [
    (24, 84, 3, 4),        # narrow mode counts routed to the many-modes plan just past W = 80
    (20, 128, 10, 65),     # widest grid, Nyquist column, few rows
    (96, 96, 12, 12),      # the default modes on a typical larger grid
    (97, 113, 48, 57),     # nothing a multiple of 4 or 16, odd W
    (100, 120, 50, 61),    # H not a multiple of any band size; over 160 KB in both directions in the whole-image layout
    (128, 96, 64, 49),     # over 160 KB in the inverse only
    (128, 128, 64, 65),    # the extreme in both directions
]


def is_many(W, m1, m2):
    return m1 > 15 or m2 > 16 or W > 80


def lds_bytes(be, H, W, m1, m2, inverse):
    return be.api.size("cfd_spectral_transform_lds_bytes", H, W, m1, m2, inverse)


def mode_choices(H, W):
    """Full modes, (12, 12) and (16, 17) where the grid admits them."""
    out = [(H // 2, W // 2 + 1)]
    for m1, m2 in ((12, 12), (16, 17)):
        if 2 * m1 <= H and m2 <= W // 2 + 1:
            out.append((m1, m2))
    return [m for m in out if m[0] >= 1]


def check_lds_sweep(be):
    """{plan: (forward, inverse)} of every swept many-modes plan whose LDS figure is not in (0, LDS_CAP], and of every swept narrow plan
    whose figure is not 0: every H in 2..128 with W in 81..128, and every many-modes plan with W <= 80, at mode_choices()."""
    bad, n_many, n_narrow = {}, 0, 0
    for H in range(2, 129):
        for W in range(2, 129):
            for m1, m2 in mode_choices(H, W):
                f, i = lds_bytes(be, H, W, m1, m2, 0), lds_bytes(be, H, W, m1, m2, 1)
                if is_many(W, m1, m2):
                    n_many += 1
                    ok = 0 < f <= LDS_CAP and 0 < i <= LDS_CAP
                else:
                    n_narrow += 1
                    ok = f == 0 and i == 0
                if not ok:
                    bad[(H, W, m1, m2)] = (f, i)
    return bad, n_many, n_narrow


def check_range(be):
    """The plan's range: what cfd_plan_create refuses and accepts around the new limits."""
    r = MK._plan_refused
    return {"W=129": r(be, 64, 129, 12, 12), "H=129": r(be, 129, 64, 12, 12), "W=200": r(be, 64, 200, 12, 12),
            "2m1>H at 96x100": r(be, 96, 100, 49, 12), "m2>W/2+1 at 96x100": r(be, 96, 100, 12, 52),
            "accepts (128,128,64,65)": not r(be, 128, 128, 64, 65), "accepts (2,128,1,1)": not r(be, 2, 128, 1, 1),
            "accepts (96,100,48,51)": not r(be, 96, 100, 48, 51)}


def check_transforms_misaligned(be, nimg, H, W, m1, m2, shift=4):
    """The transforms (forward with and without GELU, inverse with its three epilogues) on buffers `shift` bytes past a 16-byte boundary,
    through tests/align_checks.py's runner: results within K.TOL, guard bands intact."""
    from tests import align_checks as AC
    row = AC.Row("grid_idft_epilogues", K.check_idft_epilogues, (nimg, H, W, m1, m2), AC.tol(K.TOL))
    return AC._run(be, row, shift)


def check_index_guard(be):
    """Whole-model shapes on a wide grid whose activation tensors pass 2^31 - 1 elements (B * max(hidden, head) * H * W) refuse with
    CFD_ERR_UNSUPPORTED before anything else is looked at; one batch entry fewer gets as far as the argument checks.  No buffer is
    passed: both calls end at a check."""
    import ctypes

    from cfdbench_amd._capi import CfdError, FnoShape
    plan = be.api.plan_create(128, 128, 12, 12)
    try:
        msgs = {}
        for B in (1023, 1024):
            shape = FnoShape(B, 128, 128, 2, 2, 5, 20, 2, 12, 12, 128)
            try:
                be.api.call("cfd_fno_forward", plan, ctypes.byref(shape), None, None, None, None, None, None, None, None, 0, be.stream)
                msgs[B] = "accepted"
            except CfdError as e:
                msgs[B] = str(e)
        return {"B=1024 refused as unsupported": "(status -2)" in msgs[1024] and "2^31" in msgs[1024],
                "B=1023 passes the guard": "2^31" not in msgs[1023] and "NULL pointer" in msgs[1023]}
    finally:
        be.api.plan_destroy(plan)
