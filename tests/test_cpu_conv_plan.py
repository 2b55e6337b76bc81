"""CPU: the Python mirror of the convolution planners (tests/conv_plan.py) against the real host code, through the entries of the C ABI
that show a plan (listed in the mirror's docstring).  They are plain host functions, so the emulator library serves: its only
difference is the build's CFD_CONV6_GRID (2 where the product has 512), which the conv6_grid knob overrides.  A seeded sweep of 3200
shapes over the accepted range, each at one of three grids, and three named shapes at all three; what the entries cannot show (MT, NI at
k = 5 / 7, the tile) is checked only for consistency with what they do show."""
import pytest

from tests import conv_plan as CP
from tests import kernel_checks as K
from tests.backends import NumpyBackend

GRIDS = CP.GRIDS


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


SWEEP = CP.SWEEP


def test_sweep_is_what_the_docstring_says():
    assert len(SWEEP) >= 3000 and len(set(SWEEP)) > 0.98 * len(SWEEP)
    for j, lo, hi in ((0, 1, 130), (1, 1, 192), (2, 1, 192), (3, 1, 128), (4, 1, 128)):
        vals = {s[j] for s in SWEEP}
        assert min(vals) == lo and max(vals) == hi, (j, min(vals), max(vals))
    assert {s[5] for s in SWEEP} == {3, 5, 7} and {s[6] for s in SWEEP} == set(GRIDS)
    for ks in (3, 5, 7):
        for grid in GRIDS:
            assert sum(s[5] == ks and s[6] == grid for s in SWEEP) > 250


def test_mirror_predicts_every_observable_of_the_c_abi(be):
    size = be.api.size
    bad = []
    for grid_knob in GRIDS:
        grid = CP.resolve_grid(grid_knob, CP.EMUL_GRID)
        with K.tuned(be, conv6_grid=grid_knob):
            for (B, Ci, Co, H, W, ks, gk) in SWEEP:
                if gk != grid_knob:
                    continue
                s = (B, Ci, Co, H, W, ks)
                got = (size("cfd_conv2d_fwd_workspace_bytes", *s), size("cfd_conv2d_bwd_workspace_bytes", *s),
                       size("cfd_conv2d_fwd_stats_slots", *s), size("cfd_conv2d_zeropad_supported", *s),
                       size("cfd_conv2d_wfrag_bytes", Ci, Co, ks, 0), size("cfd_conv2d_wfrag_bytes", Ci, Co, ks, 1),
                       size("cfd_convt2_bwd_workspace_bytes", B, Ci, Co, H, W))
                want = (CP.fwd_workspace_bytes(*s, grid), CP.bwd_workspace_bytes(*s, grid), CP.stats_slots(*s, grid),
                        int(CP.zeropad_covers(*s, grid)), CP.wfrag_bytes(Ci, Co, ks, False), CP.wfrag_bytes(Ci, Co, ks, True),
                        CP.convt2_bwd_workspace_bytes(B, Ci, Co, H, W))
                if got != want:
                    bad.append((s, grid_knob, got, want))
    assert not bad, (len(bad), bad[:5])


def test_workspace_sizes_show_ksplit_in_both_directions(be):
    """After the fragments are subtracted, what is left of the forward workspace is ksplit partial outputs: the mirror's ksplit, read
    back from the library's figure (and the same for the input gradient inside cfd_conv2d_bwd_workspace_bytes)."""
    size = be.api.size
    seen = set()
    for (B, Ci, Co, H, W, ks, gk) in SWEEP[::7]:
        grid = CP.resolve_grid(gk, CP.EMUL_GRID)
        with K.tuned(be, conv6_grid=gk):
            left = size("cfd_conv2d_fwd_workspace_bytes", B, Ci, Co, H, W, ks) - size("cfd_conv2d_wfrag_bytes", Ci, Co, ks, 0)
        P = CP.conv6_plan(B, Ci, Co, H, W, ks, False, grid)
        assert P.ok
        assert left == (CP.align_up(P.ksplit * B * Co * H * W * 4) if P.ksplit > 1 else 0), (B, Ci, Co, H, W, ks, gk)
        seen.add(P.ksplit)
    assert {1, 2, 16} <= seen


def test_plans_are_consistent_where_the_abi_cannot_see():
    """Invariants the kernels rely on, on every plan of the sweep: the tile fits 256 threads, a thread's halo items fit NI, the LDS of an
    MT = 2 plan fits two workgroups per CU, every split-K slice owns a chunk, the weight gradient's halo fits three items per thread."""
    for (B, Ci, Co, H, W, ks, gk) in SWEEP:
        grid = CP.resolve_grid(gk)
        for ext in (False, True):
            P = CP.conv6_plan(B, Ci, Co, H, W, ks, ext, grid)
            assert P.ok and P.NB * P.TW * P.TH <= 256 and P.plane <= P.NI * 256, (B, Ci, Co, H, W, ks, ext)
            assert P.mtw == 1 or P.lds <= CP.MAX_LDS
            assert 1 <= P.ksplit <= min(P.nch, 16) and (P.ksplit - 1) * P.per < P.nch <= P.ksplit * P.per
            assert 1 <= P.gx <= P.ptiles and P.gx * P.mgroups * P.ksplit <= max(grid, P.mgroups * P.ksplit)
        wg = CP.wg6_plan(B, Ci, Co, H, W, ks, grid)
        assert wg.ok and wg.HP * 16 <= 768 and 1 <= wg.groups <= wg.ntiles


def test_tile_search_examples_from_the_planner_comments():
    """cfd_conv_tile_shape's own comments: the 66 x 66 extended grid leaves the 32 x 8 power-of-two tiles; the 10 x 10 and 6 x 6 extended grids
    of the deep U-Net levels take whole-image tiles shared by 2 and 7 images."""
    TW, TH, NB = CP.tile_shape(66, 66, 8)
    assert (TW * TH <= 256) and CP.cdiv(66, TW) * CP.cdiv(66, TH) < 27
    assert CP.tile_shape(10, 10, 8) == (10, 10, 2)
    assert CP.tile_shape(6, 6, 8) == (6, 6, 7)
    assert CP.tile_shape(64, 64, 8) == (32, 8, 1)
