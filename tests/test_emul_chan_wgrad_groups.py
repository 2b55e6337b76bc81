"""CPU (SIMT emulator): the 1x1 weight / bias gradient at 17 .. 24 channels with the second operand tiles done once per group of
chunks (k_chan_wgrad_grp) -- against fp64 and, bitwise, against the per-chunk kernel (`chan_wgrad_grp` = 0).  The cases live in
tests/wgrad_group_checks.py; the GPU twin is tests/test_gpu_chan_wgrad_groups.py."""
import numpy as np
import pytest

from tests import kernel_checks as K
from tests import wgrad_group_checks as G
from tests.backends import NumpyBackend

@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("B,blocks,lo,hi", G.TAILS)
def test_group_tails(be, B, blocks, lo, hi, act):
    """C = 20, HW = 4096: one wave walks 4, 5, 6, 7 chunks (a full group of four, then full + 1, 2, 3; B = 1 included), activation on / off."""
    assert G.chunks_per_wave(B, 4096, blocks) == (lo, hi)
    G.assert_case(G.check_wgrad_groups(be, B, 20, 20, 4096, act, blocks=blocks))


@pytest.mark.parametrize("C", G.SQUARE)
def test_live_lane_counts(be, C):
    """1, 3, 4 live lanes (groups of four chunks), 5 and 8 (groups of two); 16, 25, 32 and 8 channels stay on the per-chunk kernel."""
    assert G.chunks_per_wave(2, 1024, 2) == (8, 8)
    G.assert_case(G.check_wgrad_groups(be, 2, C, C, 1024, C % 2, blocks=2))


@pytest.mark.parametrize("Ci,Co", G.MIXED)
def test_unequal_channel_counts(be, Ci, Co):
    G.assert_case(G.check_wgrad_groups(be, 2, Ci, Co, 1024, 1, blocks=2))


@pytest.mark.parametrize("act", [0, 1])
def test_ragged_pixels(be, act):
    """66 x 65 (HW = 4290): 135 chunks per entry, the last one holds 2 pixels; planes are 8-byte aligned only (the unaligned loads)."""
    G.assert_case(G.check_wgrad_groups(be, 2, 20, 20, 66 * 65, act, blocks=6))


def test_odd_plane_size(be):
    """HW = 333: 4-byte aligned planes (the element-wise route of a partial chunk), 11 chunks per entry."""
    G.assert_case(G.check_wgrad_groups(be, 3, 20, 20, 333, 1, blocks=1))
    G.assert_case(G.check_wgrad_groups(be, 3, 22, 19, 333, 0, blocks=1))


def test_default_workgroup_count(be):
    """No cap: the launch geometry the training step uses (B = 2: one chunk per wave, a group of one)."""
    G.assert_case(G.check_wgrad_groups(be, 2, 20, 20, 4096, 1))


def test_two_piece_route(be):
    """act_pieces = 2 (the operand format the bf16-storage instantiation shares): the bound of the existing two-piece checks."""
    G.assert_case(G.check_wgrad_groups(be, 3, 20, 20, 4096, 1, blocks=16, pieces=2), 1e-9)
    G.assert_case(G.check_wgrad_groups(be, 2, 23, 21, 66 * 65, 0, blocks=6, pieces=2), 1e-9)


@pytest.mark.parametrize("C,HW,blocks", [(20, 66 * 65, 6), (17, 4096, 16), (24, 333, 1)])
def test_bias_gradient_counts_pixels(be, C, HW, blocks):
    """A constant gradient: gb[o] = 0.5 B HW exactly -- the ones column holds 1 for every pixel of the plane and 0 beyond it."""
    B = 3
    res = G.check_wgrad_groups(be, B, C, C, HW, 1, blocks=blocks, const_g=0.5)
    assert np.array_equal(res["gb_values"], np.full(C, 0.5 * B * HW, np.float32)), res["gb_values"]
    G.assert_case(res)


def test_bias_gradient_on_its_own(be):
    res = G.check_wgrad_groups(be, 5, 20, 20, 4096, 0, blocks=32)
    assert K.nm(res["gb_values"], res["gb_ref"]) < K.TOL and res["gb_bits"]


@pytest.mark.parametrize("Ci,Co,grp,label", G.ROUTES)
def test_launcher_route(be, Ci, Co, grp, label):
    """The profiler hook names the kernel that ran: both sides at 17 .. 24 channels take k_chan_wgrad_grp, every other width -- and
    chan_wgrad_grp = 0 -- the per-chunk kernel (so the bitwise comparisons above compare two kernels, not one with itself)."""
    G.assert_route(be, Ci, Co, grp, label)


@pytest.mark.parametrize("B,H,W,blocks", G.BF16_STEPS)
def test_bf16_storage_step(be, B, H, W, blocks):
    """bf16 input (the __bf16 instantiations, two pieces) at C = 20, reached through one training step with bf16 activation storage:
    waves walk a full group of four chunks plus a tail, the last chunk of a plane is partial; with and without activation (L = 2)."""
    G.assert_bf16_step(G.check_bf16_step(be, B, H, W, blocks))
