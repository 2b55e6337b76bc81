"""MI355X: the channel mix of the fused FnoBlock kernel (k_block) on its transposed source-chunk layout -- a lane reads rows 4q .. 4q+3
of one column per LDS read and accumulates them with packed FMAs.  Through the C ABI (cfd_fno_block_fwd / cfd_fno_block_bwd_input), at
64 x 64 with 12 x 12 modes and three batch entries: every launcher shape with its dead channel slots, the tail columns of the 66 x 65
grid, the row split (one tile per workgroup against tile pairs, both LDS buffers) and poisoned / dirty destinations."""
import numpy as np
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


# channels -> (waves, destination channels per wave, source chunks) of launch_block
SHAPES = [
    (8, 8, 64, 64),     # (4,2,2)
    (16, 16, 64, 64),   # (4,4,4)
    (20, 20, 64, 64),   # (10,2,2) forward and plain input gradient, (8,3,3) with gelu'
    (23, 23, 64, 64),   # (8,3,3), one dead slot
    (32, 32, 64, 64),   # (8,4,4), single source-chunk buffer
    (17, 20, 64, 64),   # unequal: dead source slots in one direction, dead destination slots in the other
    (20, 20, 66, 65),   # general grid: (8,3,3) with the tail column and a ragged fifth row tile
]


@pytest.mark.parametrize("Cin,Cout,H,W", SHAPES)
def test_block_against_the_oracle(be, Cin, Cout, H, W):
    """Forward with and without GELU on load, input gradient with and without gelu', against the fp64 oracle at the bound
    tests/test_gpu_kernels.py holds these entries to."""
    res = K.check_block(be, 3, Cin, Cout, H, W)
    bad = {k: v for k, v in res.items() if not (v < K.TOL)}
    assert not bad, f"parity failures (tol {K.TOL}): {bad}; all: {res}"


def test_row_split_is_bitwise_neutral(be):
    """Entry 0 computed alone (B = 1: four workgroups of one row tile each, every chunk of a tile in the same buffer order) equals entry 0
    inside B = 160 (one workgroup per entry: tile pairs, both tile parities, the buffers alternating across tiles) bit for bit -- all
    four forms at 20 channels."""
    api, P = be.api, be.ptr
    Bbig, C, H, W, m1, m2 = 160, 20, 64, 64, 12, 12
    rng = np.random.default_rng(41)
    a = rng.standard_normal((Bbig, C, H, W), dtype=np.float32)
    g = rng.standard_normal((Bbig, C, H, W), dtype=np.float32)
    z = (rng.standard_normal((Bbig, C, 2 * m1, m2)) + 1j * rng.standard_normal((Bbig, C, 2 * m1, m2))).astype(np.complex64)
    w0 = rng.standard_normal((C, C)).astype(np.float32)
    b0 = rng.standard_normal((C,)).astype(np.float32)
    plan = api.plan_create(H, W, m1, m2)
    try:
        da, dg, dz, dw, db = be.dev(a), be.dev(g), be.dev(z), be.dev(w0), be.dev(b0)
        got = {}
        for B in (Bbig, 1):
            outs = {k: be.out((B, C, H, W)) for k in ("fwd", "fwd_act", "bwd", "bwd_dgelu")}
            api.call("cfd_fno_block_fwd", plan, P(da), P(dz), P(dw), P(db), P(outs["fwd"]), B, C, C, 0, be.stream)
            api.call("cfd_fno_block_fwd", plan, P(da), P(dz), P(dw), P(db), P(outs["fwd_act"]), B, C, C, 1, be.stream)
            api.call("cfd_fno_block_bwd_input", plan, P(dg), P(dz), P(dw), None, P(outs["bwd"]), B, C, C, be.stream)
            api.call("cfd_fno_block_bwd_input", plan, P(dg), P(dz), P(dw), P(da), P(outs["bwd_dgelu"]), B, C, C, be.stream)
            be.sync()
            got[B] = {k: be.host(v)[:1] for k, v in outs.items()}
        diff = {k: K.words_that_differ(got[1][k], got[Bbig][k]) for k in got[1]}
        assert not any(diff.values()), f"words of entry 0 that depend on the row split: {diff}"
    finally:
        api.plan_destroy(plan)


@pytest.mark.parametrize("big,small", [(dict(B=37, C=23), dict(B=2, C=23)), (dict(B=37, C=8), dict(B=3, C=5)),
                                       (dict(B=20, C=32), dict(B=2, C=17)), (dict(B=9, C=20, H=66, W=65), dict(B=2, C=20, H=66, W=65))])
def test_poisoned_and_dirty_destinations(be, big, small):
    """The destinations start poisoned (NaN) between guard bands, then hold what a larger call left: the smaller call gives the same
    finite words either way -- nothing of a dead channel slot or a stale buffer reaches a result, nothing outside `dst` is written
    (the guard bands are verified after every test)."""
    res = K.check_dirty_reuse(be, K.case_block, big, small)
    bad = {k: v for k, v in res.items() if v != 0}
    assert not bad, f"words that differ from the run on fresh buffers, or are not finite: {bad}"
