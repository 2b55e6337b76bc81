"""MI355X: the FNO over the whole range of grids and mode counts the plan accepts (tests/range_checks.py; the CPU twin is
tests/test_emul_range.py) against the fp64 oracle -- the transforms on every route that can serve a shape, the FnoBlock at the three
k_block chunkings (and the wide two passes on k_block's grids), the whole model and the fused training step at four widths, bf16
storage at NJG = 1 .. 5, the 120 plans of the seeded sweep.  Batches of 2 .. 5 everywhere: these are the smallest shapes that reach
each instantiation.  One test has many images, so that the capped launch of the generic forward transform wraps."""
import pytest

from tests import kernel_checks as K
from tests import range_checks as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    from tests.backends import TorchBackend
    return TorchBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


BLOCK_CASES = [(*s, C) for s in R.SHAPES for C in R.BLOCK_CHANNELS + ((R.WIDE_CHANNELS,) if R.is_block_grid(s[0], s[1]) else ())]
MODEL_CASES = [(*s, C) for s in R.SHAPES for C in R.MODEL_CHANNELS]


@pytest.mark.parametrize("H,W,m1,m2", R.SHAPES)
def test_transforms_range(be, H, W, m1, m2):
    R.assert_transforms(R.check_transforms(be, H, W, m1, m2), H, W, m1, m2)


@pytest.mark.parametrize("H,W,m1,m2,C", BLOCK_CASES)
def test_block_range(be, H, W, m1, m2, C):
    R.assert_all(R.check_block(be, H, W, m1, m2, C), R.block_tol(H, W, m1, m2, C))


@pytest.mark.parametrize("H,W,m1,m2,C", MODEL_CASES)
def test_model_range(be, H, W, m1, m2, C):
    R.assert_model(R.check_model(be, H, W, m1, m2, C))


@pytest.mark.parametrize("H,W,m1,m2,C", MODEL_CASES)
def test_step_range(be, H, W, m1, m2, C):
    R.assert_step(R.check_step(be, H, W, m1, m2, C))


@pytest.mark.parametrize("H,W,m1,m2", R.BF16_SHAPES)
def test_bf16_storage_range(be, H, W, m1, m2):
    R.assert_bf16(R.check_bf16(be, H, W, m1, m2))


def test_bf16_storage_refused_above_70_rows(be):
    res = R.check_bf16_refusal(be)
    assert all(res.values()), res


def test_generic_transforms_wrap_their_capped_launch(be):
    """k_dft_fwd launches at most 2048 workgroups of four waves and strides over the images: 16500 images of 81 x 8 (43 MB a tensor)
    give every wave a second image and some a third; k_idft takes one image per wave, 4125 workgroups here."""
    nimg, H, W, m1, m2 = R.LOOP_WRAP
    assert nimg > 2 * 4 * 2048 and nimg * H * W * 4 < 64 << 20
    R.assert_all(K.check_idft_epilogues(be, nimg, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", R.SWEEP)
def test_transforms_sweep(be, H, W, m1, m2):
    R.assert_transforms(R.check_transforms(be, H, W, m1, m2), H, W, m1, m2, what=f"plan (H, W, m1, m2) = {(H, W, m1, m2)}: ")
