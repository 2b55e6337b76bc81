"""MI355X: a second, smaller call into the outputs and the workspace an earlier call left dirty -- what the training engine and the
rollout do with the buffers they size once -- must give, bit for bit, what it gives on fresh poisoned buffers (tests/kernel_checks.py:
Arena, check_dirty_reuse).  Same cases as tests/test_emul_dirty_buffers.py at the sizes where the GPU kernels change their work split:
more batch entries than compute units and fewer, persistent-workgroup walks, split-K sums."""
import pytest

from tests import kernel_checks as K

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


def _assert_bitwise(res):
    bad = {k: v for k, v in res.items() if v != 0}
    assert not bad, f"words that differ from the run on fresh buffers: {bad}"


# (big, small): fewer batch entries; for the FNO also fewer channels / modes where that changes the route
FNO_PAIRS = {
    "batch": (dict(B=64, C=20, L=4), dict(B=5, C=20, L=4)),
    "wide_to_narrow": (dict(B=4, C=64, L=2), dict(B=3, C=20, L=2)),
    "many_modes_to_narrow": (dict(B=4, C=20, L=2, m1=24, m2=24), dict(B=3, C=20, L=2)),
    "general_grid": (dict(B=8, C=32, L=2, H=66, W=65), dict(B=3, C=20, L=2, H=66, W=65)),
    "width32": (dict(B=300, C=32, L=2), dict(B=2, C=32, L=2)),
}


@pytest.mark.parametrize("pair", sorted(FNO_PAIRS))
def test_fno_forward_backward_on_dirty_buffers(be, pair):
    """cfd_fno_forward (training and inference workspace) + cfd_fno_backward."""
    _assert_bitwise(K.check_dirty_reuse(be, K.case_fno, *FNO_PAIRS[pair]))


@pytest.mark.parametrize("flags", [0, 7])
def test_fused_train_step_on_dirty_buffers(be, flags):
    """cfd_fno_forward_train_f / cfd_fno_backward_phase_f / cfd_fno_adam_step, two steps."""
    _assert_bitwise(K.check_dirty_reuse(be, K.case_fno_train_step, dict(B=300, C=20, L=2, flags=flags), dict(B=7, C=20, L=2, flags=flags)))


def test_one_workspace_across_the_three_routes(be):
    _assert_bitwise(K.check_workspace_across_routes(be, K.case_fno))


@pytest.mark.parametrize("flags", [0, 7])
def test_one_training_workspace_across_the_three_routes(be, flags):
    _assert_bitwise(K.check_workspace_across_routes(be, K.case_fno_train_step, flags=flags, steps=1))


@pytest.mark.parametrize("big,small", [(dict(B=300, Cin=20, Cout=20), dict(B=3, Cin=20, Cout=20)), (dict(B=16, Cin=32, Cout=32, H=66, W=65), dict(B=3, Cin=20, Cout=12, H=66, W=65)),
                                       (dict(B=16, Cin=64, Cout=64), dict(B=2, Cin=64, Cout=64)), (dict(B=16, Cin=20, Cout=20, m1=32, m2=33), dict(B=3, Cin=20, Cout=20, m1=32, m2=33))])
def test_spectral_conv_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_spectral, big, small))


@pytest.mark.parametrize("big,small", [(dict(B=300, C=20), dict(B=2, C=20)), (dict(B=300, C=32), dict(B=5, C=32)), (dict(B=290, C=7, H=66, W=65), dict(B=2, C=5, H=66, W=65))])
def test_fno_block_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_block, big, small))


@pytest.mark.parametrize("big,small", [(dict(B=128, Ci=12, Co=12, H=64, W=64, ks=3), dict(B=3, Ci=12, Co=12, H=64, W=64, ks=3)),
                                       (dict(B=128, Ci=96, Co=192, H=4, W=4, ks=3), dict(B=5, Ci=96, Co=192, H=4, W=4, ks=3)),
                                       (dict(B=16, Ci=24, Co=48, H=16, W=16, ks=3), dict(B=2, Ci=24, Co=48, H=16, W=16, ks=3))])
def test_conv_with_statistics_on_dirty_buffers(be, big, small):
    """cfd_conv2d_fwd_ex with the BatchNorm records (the cfd_conv2d_fwd_stats form) / cfd_conv2d_bwd_ex."""
    _assert_bitwise(K.check_dirty_reuse(be, K.case_conv, big, small))


@pytest.mark.parametrize("big,small", [(dict(B=128, Ci=24, Co=12, H=32, W=32), dict(B=3, Ci=24, Co=12, H=32, W=32)), (dict(B=128, Ci=192, Co=96, H=4, W=4), dict(B=5, Ci=192, Co=96, H=4, W=4)),
                                       (dict(B=9, Ci=5, Co=3, H=5, W=7), dict(B=1, Ci=5, Co=3, H=5, W=7))])
def test_transposed_conv_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_convt, big, small))


@pytest.mark.parametrize("big,small", [(dict(R=4290, dims=[7, 128, 64, 100]), dict(R=17, dims=[7, 128, 64, 100])), (dict(R=70001, dims=[100, 100, 100]), dict(R=333, dims=[100, 100, 100]))])
def test_ffn_stack_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_ffn_stack, big, small))


@pytest.mark.parametrize("big,small", [(dict(M=70001, K=9, N=100), dict(M=37, K=9, N=100)), (dict(M=512, K=4295, N=100), dict(M=5, K=4295, N=100)), (dict(M=4290, K=100, N=100), dict(M=300, K=100, N=100))])
def test_linear_on_dirty_buffers(be, big, small):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_linear, big, small))


def test_deeponet_inner_on_dirty_buffers(be):
    _assert_bitwise(K.check_dirty_reuse(be, K.case_deeponet_inner, dict(B=512, P_=100, Kq=4290, HW=4290), dict(B=37, P_=100, Kq=4290, HW=4290)))
