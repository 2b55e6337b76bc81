"""CPU (SIMT emulator): the FNO's many-modes route, modes1 > 15 or modes2 > 16 up to 2 modes1 <= H and modes2 <= W/2 + 1
(cfdbench_amd/csrc/dft_many.hip), against the fp64 oracle at small batches.  The GPU twin is tests/test_gpu_fno_modes.py."""
import pytest

from tests import kernel_checks as K
from tests import modes_checks as MK
from tests.backends import NumpyBackend

# (H, W, m1, m2): both blocks of rows up to every row (2 m1 = H) and up to the Nyquist column (m2 = W/2 + 1), odd grids
SHAPES = [(64, 64, 16, 16), (64, 64, 24, 20), (64, 64, 12, 20), (64, 64, 32, 33), (66, 65, 33, 33), (66, 65, 16, 17), (34, 40, 17, 21)]


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
def test_spectral_fwd_bwd_modes(be, H, W, m1, m2):
    """SpectralConv2d forward (kept modes and output) and backward (input and both weight gradients)."""
    _assert_all(K.check_spectral(be, 1, 2, 3, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_idft_epilogues_and_gelu_dft_modes(be, H, W, m1, m2):
    """Inverse transform with addend (in place) and with gelu'; forward transform with GELU on load."""
    _assert_all(K.check_idft_epilogues(be, 3, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_mix_and_spectral_wgrad_modes(be, H, W, m1, m2):
    _assert_all(K.check_mix_wgrad(be, 3, 4, 5, m1, m2, H, W))


@pytest.mark.parametrize("C", [20, 32])
def test_mix_and_spectral_wgrad_modes_fused_widths(be, C):
    """20 and 32 channels reach the fused adjoint mix + weight gradient and the matrix-pipe mode kernels where they apply."""
    with K.tuned(be, mode_mfma=1):
        _assert_all(K.check_mix_wgrad(be, 2, C, C, 32, 33, 64, 64))
    _assert_all(K.check_mix_wgrad(be, 2, C, C, 24, 20, 64, 64))


@pytest.mark.parametrize("H,W,m1,m2", [(64, 64, 16, 16), (64, 64, 32, 33), (66, 65, 33, 33), (34, 40, 17, 21)])
def test_block_modes(be, H, W, m1, m2):
    """FnoBlock forward (GELU on load) and input gradient (with and without gelu'): the two-pass form on many-modes plans."""
    _assert_all(K.check_block(be, 1, 3, 4, H, W, m1, m2))


def test_block_modes_wide(be):
    """A width above 32 (wide route) composes with the many-modes transforms."""
    _assert_all(K.check_block(be, 1, 40, 40, 64, 64, 24, 24))


@pytest.mark.parametrize("H,W,m1,m2", [(64, 64, 16, 16), (64, 64, 32, 33), (66, 65, 33, 33)])
def test_fno_modes_vs_oracle(be, H, W, m1, m2):
    """Whole model: forward, loss and every parameter gradient through cfd_fno_forward / cfd_fno_backward."""
    res = MK.check_fno_vs_oracle(be, 1, 6, 2, H, W, m1, m2)
    assert res.pop("nmse_loss") < 1e-5
    _assert_all(res, 1e-9)


def test_fused_train_step_modes_ignores_deferrals(be):
    res = MK.check_train_step_deferred(be, B=1, C=6, L=1, H=64, W=64, m1=20, m2=20)
    assert res.pop("bitwise") == 0.0
    _assert_all(res, 1e-9)


def test_spectral_modes_vs_reference_golden(be):
    """SpectralConv2d at 66 x 65, modes (33, 33), of the reference (tools/make_golden_modes.py): every row and every column of the
    half spectrum, where the reference's autograd of irfft2 is the arbiter."""
    from pathlib import Path

    import numpy as np
    g = np.load(Path(__file__).resolve().parent / "golden" / "spectral_m33_66x65.npz")
    _assert_all(MK.check_spectral_golden(be, g), 1e-9)


def test_modes_refusals(be):
    res = MK.check_refusals(be)
    assert all(res.values()), res
