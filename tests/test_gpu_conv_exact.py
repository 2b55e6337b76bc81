"""MI355X: every row of tests/conv_exact_checks.py -- one per live instantiation of k_conv6, k_conv6_wgrad, k_convt6, k_conv1, their
weight-gradient kernels and fp32 fallbacks, and per edge the planners make -- with every output under max(2e-13, 2 x the error of a
sequential float32 chain over the same terms): the fp32-exact class, a bound that a kernel which lost one of its three bf16 pieces or
one of its six piece products cannot meet (tests/test_emul_conv_exact.py shows that from references alone, checks what each row
reaches and runs the small rows on the emulator)."""
import pytest

from tests import conv_exact_checks as X

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


@pytest.mark.parametrize("row", X.ROWS, ids=lambda r: "-".join(map(str, r.shape)) + "-" + r.mode)
def test_row_at_its_bound(be, row):
    X.assert_row(X.run_row(be, row), row)
