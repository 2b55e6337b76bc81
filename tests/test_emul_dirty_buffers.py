"""CPU (SIMT emulator): a second, smaller call into the outputs and the workspace an earlier call left dirty -- what the training engine
and the rollout do with the buffers they size once -- must give, bit for bit, what it gives on fresh poisoned buffers
(tests/kernel_checks.py: Arena, check_dirty_reuse).  The GPU twin is tests/test_gpu_dirty_buffers.py."""
import pytest

from tests import kernel_checks as K
from tests.backends import NumpyBackend


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_bitwise(res):
    bad = {k: v for k, v in res.items() if v != 0}
    assert not bad, f"words that differ from the run on fresh buffers: {bad}"


# (big, small): fewer batch entries; for the FNO also fewer channels / modes where that changes the route
FNO_PAIRS = {
    "batch": (dict(B=2, C=20, L=1), dict(B=1, C=20, L=1)),
    "wide_to_narrow": (dict(B=2, C=40, L=1), dict(B=1, C=20, L=1)),
    "many_modes_to_narrow": (dict(B=2, C=6, L=1, m1=20, m2=20), dict(B=1, C=6, L=1)),
    "general_grid": (dict(B=2, C=6, L=1, H=34, W=33), dict(B=1, C=5, L=1, H=34, W=33)),
}


@pytest.mark.parametrize("pair", sorted(FNO_PAIRS))
def test_fno_forward_backward_on_dirty_buffers(be, pair):
    """cfd_fno_forward (training and inference workspace) + cfd_fno_backward."""
    _assert_bitwise(K.check_dirty_reuse(be, K.case_fno, *FNO_PAIRS[pair]))


@pytest.mark.parametrize("flags", [0, 7])
def test_fused_train_step_on_dirty_buffers(be, flags):
    """cfd_fno_forward_train_f / cfd_fno_backward_phase_f / cfd_fno_adam_step, two steps."""
    _assert_bitwise(K.check_dirty_reuse(be, K.case_fno_train_step, dict(B=2, C=20, L=1, flags=flags), dict(B=1, C=20, L=1, flags=flags)))


def test_one_workspace_across_the_three_routes(be):
    _assert_bitwise(K.check_workspace_across_routes(be, K.case_fno))


@pytest.mark.parametrize("flags", [0, 7])
def test_one_training_workspace_across_the_three_routes(be, flags):
    _assert_bitwise(K.check_workspace_across_routes(be, K.case_fno_train_step, flags=flags, steps=1))


@pytest.mark.parametrize("big,small", [(dict(B=3, Cin=20, Cout=20), dict(B=1, Cin=20, Cout=20)), (dict(B=2, Cin=5, Cout=7, H=66, W=65), dict(B=1, Cin=3, Cout=4, H=66, W=65)),
                                       (dict(B=2, Cin=3, Cout=4, m1=20, m2=20), dict(B=1, Cin=3, Cout=4, m1=20, m2=20))])
def test_spectral_conv_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_spectral, big, small))


@pytest.mark.parametrize("big,small", [(dict(B=3, C=20), dict(B=1, C=20)), (dict(B=2, C=7, H=66, W=65), dict(B=1, C=5, H=66, W=65))])
def test_fno_block_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_block, big, small))


@pytest.mark.parametrize("big,small", [(dict(B=9, Ci=5, Co=20, H=9, W=10, ks=3), dict(B=2, Ci=5, Co=20, H=9, W=10, ks=3)),
                                       (dict(B=5, Ci=12, Co=18, H=16, W=16, ks=3), dict(B=1, Ci=12, Co=18, H=16, W=16, ks=3))])
def test_conv_with_statistics_on_dirty_buffers(be, big, small):
    """cfd_conv2d_fwd_ex with the BatchNorm records (the cfd_conv2d_fwd_stats form) / cfd_conv2d_bwd_ex."""
    with K.tuned(be, conv6_grid=3):
        _assert_bitwise(K.check_dirty_reuse(be, K.case_conv, big, small))


@pytest.mark.parametrize("big,small", [(dict(B=5, Ci=12, Co=6, H=8, W=8), dict(B=2, Ci=12, Co=6, H=8, W=8)), (dict(B=3, Ci=5, Co=3, H=5, W=7), dict(B=1, Ci=5, Co=3, H=5, W=7))])
def test_transposed_conv_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_convt, big, small))


@pytest.mark.parametrize("big,small", [(dict(R=130, dims=[7, 128, 64, 100]), dict(R=17, dims=[7, 128, 64, 100])), (dict(R=300, dims=[100, 100, 100]), dict(R=33, dims=[100, 100, 100]))])
def test_ffn_stack_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_ffn_stack, big, small))


@pytest.mark.parametrize("big,small", [(dict(M=2300, K=3, N=100), dict(M=37, K=3, N=100)), (dict(M=24, K=520, N=20), dict(M=5, K=520, N=20))])
def test_linear_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_linear, big, small))


def test_deeponet_inner_on_dirty_buffers(be):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_deeponet_inner, dict(B=5, P_=100, Kq=77, HW=300), dict(B=2, P_=100, Kq=77, HW=300)))
