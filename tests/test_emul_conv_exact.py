"""CPU: the table of tests/conv_exact_checks.py checks itself against the planner mirror (every row reaches what it says, every live
kernel instantiation has a row, every dead one has its reason, every bound excludes a lost piece), a reference-only demonstration
that the bound sees what K.TOL cannot, and the rows the SIMT emulator finishes in reasonable time.  The GPU twin,
tests/test_gpu_conv_exact.py, runs every row."""
import numpy as np
import pytest

from oracle import conv_oracle as CO
from tests import conv_exact_checks as X
from tests import conv_plan as CP
from tests import kernel_checks as K
from tests.backends import NumpyBackend

# Rows left to the GPU: those of more than 10^8 multiply-adds in their passes (the emulator runs a workgroup's 256 threads as host
# fibers: the rest of the table takes it under a minute).  They are the two rows of 32 760 pixels, there for the NT4 forms of k_convt6's
# input gradient and of k_conv1 at the product's threshold of 512 workgroups; the emulator build lowers that threshold to 2, so it
# reaches the same forms on small rows (test_every_live_instantiation_... checks that no form is left to neither side).
LEFT_TO_GPU = tuple(r for r in X.ROWS if 3 * np.prod(r.shape[:5], dtype=np.int64) * max(r.shape[5], 2) ** 2 > 1e8)
assert [r.shape for r in LEFT_TO_GPU] == [(8, 145, 2, 63, 65, 2, -1), (8, 145, 146, 63, 65, 1, -1)]
EMUL_ROWS = [r for r in X.ROWS if r not in LEFT_TO_GPU]


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(request):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    if "be" in request.fixturenames:
        request.getfixturevalue("be").verify()


def _id(r):
    return "-".join(map(str, r.shape)) + "-" + r.mode


@pytest.mark.parametrize("row", X.ROWS, ids=_id)
def test_row_reaches_what_it_says(row):
    got = X.reach_of(row)
    assert row.reach, "a row says what it is there for"
    wrong = {k: (v, got.get(k)) for k, v in row.reach.items() if got.get(k) != v}
    assert not wrong, (row.shape, row.mode, "claimed, mirror:", wrong)
    B, Ci, Co, H, W, ks, gk = row.shape
    assert B * H * W <= 15000 or row.mode == "fwd+gin", "only the rows that assert no weight or bias gradient may exceed 15 000 pixels"


def test_sweep_selects_every_live_instantiation_and_no_dead_one():
    seen = set()
    for (B, Ci, Co, H, W, ks, gk) in CP.SWEEP:
        seen |= CP.conv6_keys(B, Ci, Co, H, W, ks, CP.resolve_grid(gk))
    assert {k for k in seen if k[0] != "wgrad"} == set(X.LIVE), (sorted(set(X.LIVE) - seen), sorted(k for k in seen if k in X.DEAD))
    assert {k for k in seen if k[0] == "wgrad"} == set(CP.ALL_WGRAD_KEYS)
    assert set(X.DEAD) | set(X.LIVE) == set(CP.ALL_CONV6_KEYS) and not set(X.DEAD) & set(X.LIVE) and all(X.DEAD.values())


def test_every_live_instantiation_has_a_row_on_the_gpu_and_none_is_left_to_neither_side():
    gpu = set().union(*(X.instantiations(r) for r in X.ROWS))
    missing = [k for k in X.EVERY_LIVE if k not in gpu]
    assert not missing, missing
    assert not gpu & set(X.DEAD)
    emul = set().union(*(X.instantiations(r, emul=True) for r in EMUL_ROWS))
    gpu_only = set().union(*(X.instantiations(r) for r in LEFT_TO_GPU))
    neither = [k for k in X.EVERY_LIVE if k not in emul and k not in gpu_only]
    assert not neither, neither
    assert len(LEFT_TO_GPU) < len(X.ROWS) // 3


def test_the_edges_the_planner_makes_have_rows():
    reach = [X.reach_of(r) for r in X.ROWS if r.shape[5] > 2]
    for d in ("fwd", "ext"):
        assert any(r[d + "_ksplit"] == 16 for r in reach)
        assert any(r[d + "_ragged_nb"] for r in reach)
        assert any(t[0] & (t[0] - 1) or t[1] & (t[1] - 1) for t in (r[d + "_tile"] for r in reach))  # not a power of two
    assert any(r["fwd_ragged_k"] for r in reach)  # (one kernel serves both directions: the slice bounds are the same code)
    assert any(r["fwd_tile"][0] == 64 for r in reach)
    rows3 = [(row, X.reach_of(row)) for row in X.ROWS if row.shape[5] > 2]
    assert any(t["fwd_tile"][:2] == (row.shape[4], row.shape[3]) and t["fwd_tile"][2] > 1 for row, t in rows3)  # whole image, several images
    assert any(r["wg_TW"] == 4 for r in reach) and {True, False} <= {r["direct"] for r in reach}
    assert any(not r["direct"] and r["ext_ksplit"] == 1 for r in reach) and any(not r["direct"] and r["ext_ksplit"] > 1 for r in reach)
    assert {m for m in (r.mode for r in X.ROWS)} >= {"gin", "gw+gb", "gw", "gb", "zeropad", "stats"}
    assert {r.shape[5] for r in X.ROWS if r.mode == "zeropad"} == {3, 5, 7}
    # every reason for which a matrix-pipe weight gradient leaves the call to the fp32 kernel
    fp32 = [r for r in X.ROWS if X.reach_of(r).get("convt_wg") == "fp32" and "gw" in "".join(X.outputs_of(r))]
    assert any(r.shape[4] % 4 for r in fp32) and any(r.shape[4] % 4 == 0 and r.shape[3] * r.shape[4] % 8 for r in fp32) and any(r.mode == "in+4" for r in fp32)
    fp32 = [r for r in X.ROWS if X.reach_of(r).get("conv1_wg") == "fp32" and "gw" in X.outputs_of(r)]
    assert any(r.shape[3] * r.shape[4] % 8 for r in fp32) and any(r.mode == "in+4" for r in fp32)


@pytest.mark.parametrize("row", X.ROWS, ids=_id)
def test_bound_excludes_a_lost_piece(row):
    """The condition of the table: every asserted output's bound, from the references alone, is under MAX_BOUND."""
    bd = X.bounds_of(row)
    assert set(bd) == set(X.outputs_of(row))
    print(row.shape, row.mode, {k: f"chain {e:.2e} bound {b:.2e}" for k, (b, e) in bd.items()})
    bad = {k: v for k, v in bd.items() if not (X.EXACT_TOL <= v[0] < X.MAX_BOUND)}
    assert not bad, (row.shape, row.mode, bad)


def test_a_lost_third_piece_fails_the_bound_and_passes_the_old_one():
    """References only: the fp64 oracle on operands rounded to TWO bf16 pieces is what a kernel that lost its third piece would
    return at best.  It passes K.TOL, the bound of every conv test before this file, and fails the row's bound."""
    for shape in ((31, 9, 33, 5, 26, 3, -1), (16, 3, 33, 65, 1, 5, -1), (1, 3, 5, 17, 1, 7, -1)):
        row = next(r for r in X.ROWS if r.shape == shape and r.mode == "conv")
        I = X.inputs_of(row)
        x, w, b, g = (I[k].astype(np.float64) for k in ("x", "w", "b", "g"))
        x2, w2, g2 = (X.two_pieces(I[k]).astype(np.float64) for k in ("x", "w", "g"))
        ref = X.refs_of(row, I)
        gin2, gw2, _ = CO.conv2d_bwd(g2, x2, w2)
        lost = {"out": CO.conv2d(x2, w2, b), "gin": gin2, "gw": gw2}
        for name, v in lost.items():
            e, bound = K.nm(v, ref[name]), X.bounds_of(row)[name][0]
            assert bound < e < K.TOL, (shape, name, e, bound)
        # ... and the split of one operand alone
        e = K.nm(CO.conv2d(x, w2, b), ref["out"])
        assert X.bounds_of(row)["out"][0] < e < K.TOL, (shape, e)


def test_the_emulator_order_alone_exceeds_the_bound_where_a_row_says_so():
    """EMUL_ORDER: the order of the emulator's MFMA twin, evaluated in NumPy float32 (a reference, not the kernel), is over the plain
    bound of each output listed there -- and twice its figure still excludes a lost piece."""
    rows = {(r.shape, r.mode): r for r in X.ROWS}
    assert set(X.EMUL_ORDER) <= set(rows)
    for key, names in X.EMUL_ORDER.items():
        plain, emul = X.bounds_of(rows[key]), X.bounds_of(rows[key], "emul")
        for n in names:
            print(key, n, f"chain32 {plain[n][1]:.2e} bound {plain[n][0]:.2e}; emulator order {emul[n][1]:.2e} bound {emul[n][0]:.2e}")
            assert emul[n][1] > plain[n][0] and emul[n][0] < X.MAX_BOUND, (key, n, plain[n], emul[n])


@pytest.mark.parametrize("row", EMUL_ROWS, ids=_id)
def test_row_at_its_bound(be, row):
    X.assert_row(X.run_row(be, row), row)
