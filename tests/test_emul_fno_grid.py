"""CPU (SIMT emulator): the FNO on grids wider than 80 columns, up to 128 x 128 -- many-modes plans whatever their mode counts
(cfdbench_amd/csrc/dft_many.hip) -- against the fp64 oracle at small batches, and the LDS figure of the transforms over the whole range
(the emulator does not model LDS capacity: the sweep reads the function the launchers use).  The GPU twin is tests/test_gpu_fno_grid.py."""
from pathlib import Path

import numpy as np
import pytest

from tests import grid_checks as G
from tests import kernel_checks as K
from tests import modes_checks as MK
from tests.backends import NumpyBackend

SHAPES = G.SHAPES


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_all(res, tol=K.TOL):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_spectral_fwd_bwd_grid(be, H, W, m1, m2):
    """SpectralConv2d forward (kept modes and output) and backward (input and both weight gradients)."""
    _assert_all(K.check_spectral(be, 1, 2, 3, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_idft_epilogues_and_gelu_dft_grid(be, H, W, m1, m2):
    """Inverse transform with addend (in place) and with gelu'; forward transform with GELU on load."""
    _assert_all(K.check_idft_epilogues(be, 3, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", [SHAPES[0], SHAPES[4], SHAPES[6]])
def test_mix_and_spectral_wgrad_grid(be, H, W, m1, m2):
    _assert_all(K.check_mix_wgrad(be, 3, 4, 5, m1, m2, H, W))


@pytest.mark.parametrize("H,W,m1,m2", [SHAPES[0], SHAPES[2], SHAPES[3], SHAPES[6]])
def test_block_grid(be, H, W, m1, m2):
    """FnoBlock forward (GELU on load) and input gradient (with and without gelu'): the two-pass form on many-modes plans."""
    _assert_all(K.check_block(be, 1, 3, 4, H, W, m1, m2))


def test_block_grid_wide(be):
    """A width above 32 (wide route) composes with the transforms of a wide grid."""
    _assert_all(K.check_block(be, 1, 40, 40, 96, 100, 12, 12))


@pytest.mark.parametrize("H,W,m1,m2", [(96, 96, 12, 12), (128, 128, 64, 65)])
def test_fno_grid_vs_oracle(be, H, W, m1, m2):
    """Whole model: forward, loss and every parameter gradient through cfd_fno_forward / cfd_fno_backward."""
    res = MK.check_fno_vs_oracle(be, 1, 6, 2, H, W, m1, m2)
    assert res.pop("nmse_loss") < 1e-5
    _assert_all(res, 1e-9)


def test_transform_lds_within_the_cu(be):
    """cfd_spectral_transform_lds_bytes, the figure the launchers size their dynamic LDS by: within (0, 160 KB] in both directions for every
    H in 2..128 and W in 81..128 and for every many-modes plan with W <= 80 (full modes, (12, 12), (16, 17)); 0 for a narrow plan."""
    bad, n_many, n_narrow = G.check_lds_sweep(be)
    assert n_many > 127 * 48 and n_narrow > 0
    assert not bad, f"{len(bad)} plans outside (0, {G.LDS_CAP}] (many-modes) or != 0 (narrow); first: {sorted(bad.items())[:8]}"


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_transform_lds_of_the_shapes(be, H, W, m1, m2):
    for inverse in (0, 1):
        assert 0 < G.lds_bytes(be, H, W, m1, m2, inverse) <= G.LDS_CAP
    assert G.lds_bytes(be, 64, 64, 12, 12, 0) == 0 and G.lds_bytes(be, 128, 80, 15, 16, 1) == 0


def test_grid_range(be):
    res = G.check_range(be)
    assert all(res.values()), res


def test_grid_bf16_storage_refused(be):
    """bf16 activation storage on W > 80 (inference forward and training step, the two _ex entries) refuses as on every many-modes plan."""
    res = MK.check_refusals(be, H=24, W=84, m1=3, m2=4)
    assert res["bf16_forward"] and res["bf16_train"], res


@pytest.mark.parametrize("name", ["spectral_g100x120_m50x61"])
def test_spectral_grid_vs_reference_golden(be, name):
    """SpectralConv2d at 100 x 120, modes (50, 61), of the reference (tools/make_golden_grid.py): every row and the Nyquist column."""
    g = np.load(Path(__file__).resolve().parent / "golden" / f"{name}.npz")
    _assert_all(MK.check_spectral_golden(be, g), 1e-9)


def test_grid_index_guard(be):
    res = G.check_index_guard(be)
    assert all(res.values()), res
