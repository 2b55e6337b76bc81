"""CPU (SIMT emulator): the FNO with domain padding (cfd_fno_shape.pad, cfdbench_amd/csrc/pad.hip) against the padded fp64 oracle of
tests/pad_checks.py at small batches, and that oracle against two fixtures of the reference's Fno2d(padding=p).  The GPU twin is
tests/test_gpu_fno_pad.py."""
from pathlib import Path

import numpy as np
import pytest

from tests import kernel_checks as K
from tests import pad_checks as PC
from tests.backends import NumpyBackend

SHAPES = PC.SHAPES


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


@pytest.mark.parametrize("name", ["fno_pad8_64x64", "fno_pad9_66x65"])
def test_padded_oracle_vs_reference_golden(name):
    """The oracle extension itself: fp64 composition against the reference's fp32 Fno2d(padding=p) (tools/make_golden_pad.py), at the
    tolerances of tests/test_oracle_golden.py."""
    res, pad = PC.check_oracle_golden(np.load(Path(__file__).resolve().parent / "golden" / f"{name}.npz"))
    assert pad >= 8
    assert res.pop("preds") < 1e-11 and res.pop("g_inputs") < 1e-9
    for k in ("mse", "rmse", "mae", "nmse"):
        assert res.pop("loss_" + k) <= 2e-6
    for k in [k for k in res if k.startswith("gnorm:")]:
        assert res.pop(k) <= 1e-4, k
    _assert_all(res, 1e-8)


@pytest.mark.parametrize("H,W,pad,m1,m2", SHAPES)
def test_fno_pad_vs_oracle(be, H, W, pad, m1, m2):
    """Whole model: forward under both workspaces, loss and every parameter gradient through cfd_fno_forward / cfd_fno_backward."""
    PC.accept_vs_oracle(PC.check_fno_pad_vs_oracle(be, 1, 6, 1 if H == 120 else 2, H, W, pad, m1, m2))


@pytest.mark.parametrize("which", ["mse", "nmse"])
@pytest.mark.parametrize("H,W,pad,m1,m2", PC.DEFERRAL_SHAPES)
def test_pad_train_step_ignores_deferrals(be, H, W, pad, m1, m2, which):
    res = PC.check_pad_train_step(be, 1, 6, 2, H, W, pad, m1, m2, which=which)
    assert res.pop("bitwise") == 0.0
    _assert_all(res, 1e-9)


@pytest.mark.parametrize("H,W,pad,m1,m2", [SHAPES[0], SHAPES[2], SHAPES[3]])
def test_pad_band_written_on_every_call(be, H, W, pad, m1, m2):
    res = PC.check_pad_dirty(be, 1, 6, 2, H, W, pad, m1, m2)
    assert res.pop("second_run") == 0.0 and res.pop("finite_fill") == 0.0, res
    _assert_all(res)


def test_pad_misaligned(be):
    assert PC.check_pad_misaligned(be) >= 1


@pytest.mark.parametrize("H,W,pad,m1,m2", [SHAPES[0], SHAPES[1], SHAPES[2], SHAPES[4]])
def test_pad_zero_spectral_equals_unpadded(be, H, W, pad, m1, m2):
    _assert_all(PC.check_pad_zero_spectral(be, 1, 6, 2, H, W, pad, m1, m2))


def test_pad_refusals(be):
    res = PC.check_pad_refusals(be)
    assert all(v is True for v in res.values()), res


def test_pad_zero_is_the_unpadded_call(be):
    res = PC.check_pad_zero_is_unpadded(be)
    assert all(res.values()), res
