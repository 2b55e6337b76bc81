"""CPU (SIMT emulator): gradient accumulation over micro-batches inside cfd_fno_adam_step (CFD_STEP_ACCUMULATE / CFD_STEP_ACCUM_INIT;
k_grad_accum) through the C ABI, on hostile memory with the accumulator NaN-poisoned before its first call -- tests/accum_checks.py.  The
GPU twin is tests/test_gpu_fno_accum.py.  A library that ignores the two bits runs Adam on the "accumulator": every check here fails."""
import pytest

from tests import accum_checks as AC
from tests.backends import NumpyBackend


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


@pytest.mark.parametrize("name", list(AC.CASES))
def test_init_with_scale_one_copies_the_gradient_bit_for_bit(be, name):
    """(1) flags = 0, mse, grad_scale = 1, NULL moments: a poisoned accumulator equals the gradient buffer afterwards."""
    AC.check_init_exact(be, name)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_init_finishes_the_deferred_work_and_touches_nothing_else(be, name):
    """(2) the fc0 rows, poison before the call, are bitwise those the optimiser call leaves on the same pass; the accumulator against
    fp32(s) * grad at 1e-13.  (4) poisoned moments and clip buffer stay poison, the weights keep their bits."""
    AC.check_init_deferred(be, name)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_sum_over_micro_batches_then_adam_on_the_accumulator(be, name):
    """(3) three micro-batches with weights 1/3 against the fp64 sum of the device's own per-pass gradients at 1e-12, each of those against
    the fp64 oracle; three optimiser steps on the accumulator against oracle.adam_step at 1e-9, clipped (norm, coefficient at 2.5e-7) and
    unclipped.  (5) the add call repeated on a copy of the accumulator gives the same bits."""
    AC.check_sum_and_adam(be, name)


def test_misaligned_placement_gives_the_aligned_bits(be):
    AC.check_misaligned_gives_the_aligned_bits(be)


def test_refusals_before_any_launch(be):
    """(6) INIT without ACCUMULATE, NULL param, NULL grad: CFD_ERR_INVALID_ARG, every buffer still poison."""
    got = AC.check_refusals(be)
    assert got == {k: (-1, True) for k in ("init_alone", "null_param", "null_grad")}, got


def test_empty_buffer_launches_nothing(be):
    assert AC.check_empty(be)
