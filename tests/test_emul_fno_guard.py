"""CPU (SIMT emulator): skipping non-finite steps inside cfd_fno_adam_step (CFD_STEP_SKIP_NONFINITE) -- tests/guard_checks.py on the
unmodified kernels, on hostile memory between guard bands.  The GPU twin is tests/test_gpu_fno_guard.py."""
import pytest

from tests import guard_checks as GC
from tests.backends import NumpyBackend


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_a_nonfinite_gradient_writes_nothing(be, misalign):
    """(a) n = 1, 7, 1028; NaN, +inf, -inf at element 0, at the last element, in the n % 4 tail, and a NaN grad_scale; with and without
    AdamW, max_grad_norm = +inf and 1: parameters, moments and gradient keep their bits, clip[1] = 0, both counters go up by one.  Fails
    without the kernel variant: the bit is then ignored and the NaN reaches every buffer."""
    assert GC.check_skip_flat(be, misalign) == 4 * sum(3 * len(GC.bad_positions(n)) + 1 for n in GC.FLAT_NS) == 84


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_finite_gradients_are_bitwise_the_call_without_the_bit(be, misalign):
    """(b) three steps, clip set on both sides: every buffer and clip[0..1] bit for bit, the counters 0."""
    GC.check_finite_is_bitwise(be, misalign)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_finite_nonfinite_finite_follows_the_rule_at_t_1_and_3(be, misalign):
    """(c) the step count runs on over the skip: the fp64 rule at t = 1 and t = 3, at the Adam bound of finetune_checks."""
    GC.check_sequence(be, misalign)


@pytest.mark.parametrize("kind", ["inf", "zero"], ids=["inf_in_label", "zero_label"])
def test_whole_steps_with_deferrals(be, kind):
    """(d) 64 x 64, C = 20, L = 2, nmse, flags = 7 | 64: one +inf in the label, and an all-zero label (the normaliser is inf)."""
    GC.check_deferred_steps(be, kind)


def test_the_bit_is_ignored_with_accumulate_and_skips_the_group_afterwards(be):
    """(e)"""
    GC.check_accumulate_ignores_the_bit(be)


def test_refusal_and_empty_buffer(be):
    """(f) the bit without grads->clip: CFD_ERR_INVALID_ARG before any launch; n == 0: clip = (0, 1), counters untouched."""
    assert GC.check_refusal(be) == (-1, True)
    assert GC.check_empty(be) == ([0.0, 1.0], (4.0, 3.0), True)
