"""CPU (SIMT emulator): the FNO's wide-channel route, hidden widths 33 .. 128 (cfdbench_amd/csrc/wide.hip), against the fp64
oracle at small batches.  The GPU twin is tests/test_gpu_fno_wide.py."""
import pytest

from tests import kernel_checks as K
from tests import wide_checks as WK
from tests.backends import NumpyBackend


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


@pytest.mark.parametrize("Cin,Cout", [(33, 33), (48, 40), (64, 64), (20, 72)])
def test_mix_and_spectral_wgrad_wide(be, Cin, Cout):
    _assert_all(K.check_mix_wgrad(be, 2, Cin, Cout))


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
def test_spectral_fwd_bwd_wide(be, H, W):
    _assert_all(K.check_spectral(be, 1, 64, 64, H, W))


@pytest.mark.parametrize("C", [33, 64])
@pytest.mark.parametrize("act", [0, 1])
def test_chanmix_wide(be, C, act):
    """1x1 conv forward, input gradient and weight gradient (GELU on load with act)."""
    _assert_all(K.check_chanmix(be, 2, C, C, 130, act))


def test_chanmix_wide_mixed_counts(be):
    _assert_all(K.check_chanmix(be, 2, 20, 72, 66, 1))


def test_block_wide(be):
    _assert_all(K.check_block(be, 1, 40, 40, 66, 65))


@pytest.mark.parametrize("C", [48, 64])
def test_stem_wide(be, C):
    _assert_all(K.check_stem(be, 2, 24, 26, 3, C, True))


@pytest.mark.parametrize("C", [48, 64])
@pytest.mark.parametrize("act", [0, 1])
def test_head_fwd_wide(be, C, act):
    _assert_all(WK.check_head_fwd(be, 2, C, 150, act))


@pytest.mark.parametrize("C,act,which,ext", [(48, True, "nmse", False), (64, False, "mse", True), (64, True, "mae", False)])
def test_head_wide(be, C, act, which, ext):
    res = K.check_head(be, 2, C, 150, act, which, ext)
    _assert_all({k: v for k, v in res.items() if k not in ("sums", "scores")})
    assert res["sums"] < 1e-5 and res["scores"] < 1e-5


@pytest.mark.parametrize("C,act,which", [(48, True, "nmse"), (64, False, "mse")])
def test_head_train_wide(be, C, act, which):
    res = K.check_head_train(be, 2, C, 150, act, which)
    assert res.pop("sums") < 1e-5
    _assert_all(res)


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
def test_fno_forward_wide_vs_oracle(be, H, W):
    _assert_all(WK.check_fno_forward_vs_oracle(be, 1, 64, 2, H, W, border=True))


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
def test_fno_wide_vs_oracle(be, H, W):
    """Whole model at width 64: forward, loss and every parameter gradient through cfd_fno_forward / cfd_fno_backward."""
    res = K.check_fno_vs_oracle(be, 1, 64, 2, H, W, border=True)
    assert res.pop("nmse_loss") < 1e-5
    _assert_all(res, 1e-9)


def test_fused_train_step_wide_ignores_deferrals(be):
    """The wide route has no fused kernel to carry a deferred launch: with every CFD_TRAIN_DEFER_* flag set the step equals the step
    without flags bit for bit, and its gradient holds the oracle."""
    res = K.check_fno_train_step_deferred(be, B=1, C=40, L=1, H=64, W=64, which="mse", flags=7)
    assert res.pop("sums") == 0.0 and res.pop("preds") == 0.0
    assert res.pop("params") == 0.0 and res.pop("grad_vs_immediate") == 0.0
    _assert_all(res, 1e-11)


def test_bf16_storage_refused_wide(be):
    res = WK.check_wide_refusals(be)
    assert all(res.values()), res
