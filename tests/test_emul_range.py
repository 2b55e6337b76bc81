"""CPU (SIMT emulator): the FNO transforms over the whole range of grids and mode counts the plan accepts (tests/range_checks.py) against
the fp64 oracle (R.EXACT_TOL where the split-bf16 kernels serve, K.TOL on the generic ones).  Every row of the table and every one of the 120 plans of the seeded sweep runs the transforms on every route that can
serve it; the FnoBlock, the whole model, the fused training step and bf16 storage run at 8 channels on the rows of at most 1100 pixels
and on one tall row.  The emulator holds the index math and the tables; the operand layouts of the matrix pipe, LDS at full size and the
launch bounds are the GPU twin's, tests/test_gpu_range.py."""
import pytest

from tests import range_checks as R
from tests.backends import NumpyBackend

SMALL = [s for s in R.SHAPES if s[0] * s[1] <= 1100] + [(100, 30, 15, 16)]  # (the tall row: T = 7, full modes, the Nyquist column)


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def test_the_table_covers_what_it_claims():
    """The classes of the table, read off the shapes: every tile count of the tall region on float4 rows, on scalar rows and at NJ = 5;
    the narrow maxima on every family; NJG = 1 .. 5; both sides of the seam."""
    tall = [(H, W) for H, W, m1, m2 in R.SHAPES if H > 80 and not R.G.is_many(W, m1, m2)]
    assert {(H + 15) // 16 for H, W in tall if W % 4 == 0 and W <= 64} == {6, 7, 8}
    assert {(H + 15) // 16 for H, W in tall if W % 4 != 0 and W <= 64} == {6, 7, 8}
    assert {(H + 15) // 16 for H, W in tall if W > 64} == {6, 7, 8}
    assert {(H // 2 + 4) // 4 for H, W in tall} >= {11, 13, 15, 16, 17}
    full = {(H, W) for H, W, m1, m2 in R.SHAPES if (m1, m2) == (15, 16)}
    assert full >= {(64, 64), (66, 65), (70, 80), (48, 64), (30, 30), (128, 80), (80, 68)}
    assert {(W + 15) // 16 for H, W, m1, m2 in R.SHAPES if H <= 70 and W <= 80} == {1, 2, 3, 4, 5}
    assert sum(R.G.is_many(W, m1, m2) for H, W, m1, m2 in R.SHAPES) == 2
    assert len(R.SWEEP) == 120 and len(set(R.SWEEP)) > 110
    for q in range(4):
        assert sum(m2 == W // 2 + 1 for H, W, m1, m2 in R.SWEEP[q::4]) >= 10


@pytest.mark.parametrize("H,W,m1,m2", R.SHAPES)
def test_transforms_range(be, H, W, m1, m2):
    R.assert_transforms(R.check_transforms(be, H, W, m1, m2), H, W, m1, m2)


@pytest.mark.parametrize("H,W,m1,m2", SMALL)
def test_block_range(be, H, W, m1, m2):
    R.assert_all(R.check_block(be, H, W, m1, m2, 8), R.block_tol(H, W, m1, m2, 8))


@pytest.mark.parametrize("H,W,m1,m2", SMALL)
def test_model_range(be, H, W, m1, m2):
    R.assert_model(R.check_model(be, H, W, m1, m2, 8))


@pytest.mark.parametrize("H,W,m1,m2", SMALL)
def test_step_range(be, H, W, m1, m2):
    R.assert_step(R.check_step(be, H, W, m1, m2, 8))


@pytest.mark.parametrize("H,W,m1,m2", R.BF16_SHAPES)
def test_bf16_storage_range(be, H, W, m1, m2):
    R.assert_bf16(R.check_bf16(be, H, W, m1, m2))


def test_bf16_storage_refused_above_70_rows(be):
    res = R.check_bf16_refusal(be)
    assert all(res.values()), res


@pytest.mark.parametrize("H,W,m1,m2", R.SWEEP)
def test_transforms_sweep(be, H, W, m1, m2):
    R.assert_transforms(R.check_transforms(be, H, W, m1, m2), H, W, m1, m2, what=f"plan (H, W, m1, m2) = {(H, W, m1, m2)}: ")
