"""CPU (SIMT emulator): the fused FNO engine's K-step rollout window as its call sequence over the C ABI -- tests/window_checks.py: K
forward passes on workspaces of their own, the backward passes K .. 1 chained through grads->d_inputs / gpreds_ext, every pass's gradient
added to the accumulator by cfd_fno_adam_step(CFD_STEP_ACCUMULATE).  The GPU twin is tests/test_gpu_fno_window.py.

Left to the GPU twin: the shape 64x64_w20_b5 (B = 5, width 20: two forward and two backward passes of tens of seconds each on the
emulator) and the two-pass-head run of the K = 3 fixture fno_unroll3 (64 x 64, six passes: 6 s per run here; the one-pass head, the
engine's default, runs)."""
import pytest

from tests import window_checks as WC
from tests.backends import NumpyBackend

CASES = [n for n in WC.CASES if n != "64x64_w20_b5"]
HEADS = {"one_pass_head": True, "two_pass_head": False}


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_all(res, tol):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


def test_window_of_three_vs_reference_golden(be):
    """The reference's own unrolled run at the bound the eager window is held to (tests/test_gpu_fno_ingrad.py)."""
    res, loss_err = WC.check_golden(be, True)
    print(res, "loss", loss_err)
    _assert_all(res, WC.MODEL_TOL)
    assert loss_err <= 5e-6


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("name", CASES)
def test_window_vs_fp64(be, name, head):
    res = WC.check_small(be, name, HEADS[head])
    print(name, head, res)
    _assert_all(res, WC.ABI_TOL)


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("name", ["9x7_scalar_form", "12x12_pad4"])
def test_two_windows_with_weight_one_half(be, name, head):
    _assert_all(WC.check_two_windows(be, name, HEADS[head]), WC.ABI_TOL)


@pytest.mark.parametrize("head", list(HEADS))
def test_first_window_never_reads_the_accumulator_and_repeats_bitwise(be, head):
    WC.check_poisoned_accumulator_and_repeat(be, "9x7_scalar_form", HEADS[head])


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("name", ["9x7_scalar_form", "p8_cin3"])
def test_detached_window_is_the_mean_of_the_one_step_gradients(be, name, head):
    res, far = WC.check_detach(be, name, HEADS[head])
    print(name, head, res, "distance from the full gradient", far)
    _assert_all(res, WC.ABI_TOL)
    assert far > 1e3 * WC.ABI_TOL, f"the truncated gradient equals the full one ({far}): the flag does nothing"
