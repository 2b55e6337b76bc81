"""CPU (SIMT emulator): gradient-norm clipping inside cfd_fno_adam_step (cfd_fno_params.clip / max_grad_norm, ABI 604) through the C ABI, on
hostile memory with the clip buffer NaN-poisoned on entry -- tests/clip_checks.py.  The GPU twin is tests/test_gpu_fno_clip.py."""
import numpy as np
import pytest

from tests import clip_checks as CC
from tests.backends import NumpyBackend


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


@pytest.mark.parametrize("name", list(CC.CASES))
def test_threshold_that_does_not_bite_is_bitwise_the_unclipped_step(be, name):
    """(a) max_grad_norm = +inf and (f) a finite threshold far above the norm: parameters, moments and the gradient buffer of three steps
    bit for bit those of the call without clip; clip[1] == 1."""
    norm1 = CC.check_coef_one_is_bitwise(be, name, "inf", float("inf"))
    CC.check_coef_one_is_bitwise(be, name, "above", 1e3 * norm1)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_clipped_step_against_the_rule(be, name):
    """(b) norm and coefficient against the fp64 restatement at 2.5e-7, moments after every step and parameter deltas after three against
    oracle.adam_step at 1e-9; (c) the gradient buffer, fc0 rows included, stays the unclipped step's; (d) two calls, the same bits."""
    CC.check_clipped(be, name)


def test_bad_thresholds_are_refused_before_any_launch(be):
    """(e) 0, -1 and NaN: CFD_ERR_INVALID_ARG, every buffer still poison."""
    got = CC.check_refusals(be)
    assert got == {repr(b): (-1, True) for b in (0.0, -1.0, float("nan"))}, got


def test_empty_buffer(be):
    pair, untouched = CC.check_empty(be)
    assert pair.tolist() == [0.0, 1.0] and untouched, (pair, untouched)
