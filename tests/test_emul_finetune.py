"""CPU (SIMT emulator): fine-tuning on the fused FNO step through the C ABI -- decoupled weight decay inside cfd_fno_adam_step
(CFD_STEP_DECOUPLED_WD) and whole steps over a trainable subset on compact flat buffers -- tests/finetune_checks.py, on hostile memory between
guard bands.  The GPU twin is tests/test_gpu_finetune.py."""
import pytest

from tests import finetune_checks as FT
from tests.backends import NumpyBackend


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_adamw_bit_on_flat_buffers(be, misalign, clip):
    """n = 1, 3, 4, 5, 1027 (scalar form, the n % 4 tail, the 16-byte form), three steps: the bit with weight_decay = 0.1 against the fp64
    rule at 1e-9 (fails without the kernel variant: the bit is then ignored and the decay is coupled); with weight_decay = 0 bitwise plain
    Adam; without the bit the coupled form, bitwise cfd_adam_flat."""
    FT.check_adamw_flat(be, misalign, clip)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_adamw_bit_beside_the_deferral_flags(be, misalign, clip):
    """64 x 64, C = 20, L = 2, nmse, flags = 7 | CFD_STEP_DECOUPLED_WD: the normaliser, the lifting layer's rows and the clip factor are what
    they are without the bit; moments and parameter deltas of three steps against the rule at 1e-9."""
    FT.check_adamw_deferred(be, misalign, clip)


@pytest.mark.parametrize("subset", ["head", "last_block_head", "fc0_head", "spectral"])
@pytest.mark.parametrize("shape", list(FT.SHAPES))
def test_frozen_subset_steps(be, shape, subset):
    """Two steps with compact buffers, sink pointers and the shortened phase list: trainable tensors against the fp64 oracle, frozen ones
    bitwise untouched, guard bands of the compact moments intact."""
    FT.check_subset(be, shape, subset)
