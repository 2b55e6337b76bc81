"""CPU (SIMT emulator): the FNO's gradients with respect to its inputs and case parameters through the C ABI (cfd_fno_params.d_inputs /
d_case_params, cfdbench_amd/csrc/ingrad.hip), against the reference's fixtures and the fp64 restatement of tests/ingrad_checks.py, and that
restatement against the fixtures and tests/pad_checks.py's oracle.  The GPU twin is tests/test_gpu_fno_ingrad.py."""
import numpy as np
import pytest

from tests import ingrad_checks as IC
from tests import pad_checks as PC
from tests.backends import NumpyBackend

ABI_TOL = 1e-9    # C ABI against fp64
MODEL_TOL = 1e-8  # against the reference's fp32 fixtures (tests/test_gpu_model.py's bound on parameter gradients)


@pytest.fixture(scope="module")
def be():
    return NumpyBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_all(res, tol):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


# ---- the restatement itself ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IC.REFERENCE_GOLDENS + ["fno_ingrad_c3"])
def test_restatement_vs_reference_golden_and_oracle(name):
    """The fp64 torch restatement against the reference's fp32 g_inputs (and g_case_params, sampled parameter gradients) at the fixtures'
    own bounds, and against the NumPy oracle's `__inputs__` and parameter gradients at 1e-9.  Measured fp32-fixture-vs-fp64 nMSE of the new
    fixture fno_ingrad_c3: g_inputs 1.5e-13, g_case_params 5e-13, sampled parameter gradients <= 2.6e-12 -- inside 1e-8, so that bound holds."""
    g = IC.load_golden(name)
    params, batch, s = IC.golden_case(g)
    ref = IC.cached(("golden_ref", name), lambda: IC.ref_run(params, batch, s["L"], s["pad"]))
    res = {"g_inputs": IC.golden_field(g, "g_inputs", ref["g_inputs"])}
    if "g_case_params" in g.files:
        res["g_case_params"] = IC.nm(ref["g_case_params"], g["g_case_params"])
    res.update(IC.golden_gsums(g, ref["grads"]))
    print(name, "fixture vs fp64:", res)
    assert res.pop("g_inputs") < 1e-9
    _assert_all(res, MODEL_TOL)
    _oref, og = PC.oracle_run(params, batch, s["L"], s["pad"])
    ores = {"__inputs__": IC.nm(ref["g_inputs"], og["__inputs__"]), "preds": IC.nm(ref["preds"], _oref["preds"])}
    ores.update({k: IC.nm(ref["grads"][k], og[k]) for k in params})
    _assert_all(ores, 1e-9)


def test_restatement_vs_unrolled_golden():
    """K = 3 through the restatement against the reference's unrolled run.  Measured fp32-fixture-vs-fp64 nMSE: predictions 3e-14, loss
    5e-8 relative, g_inputs 5e-14, g_case_params 4e-14, sampled parameter gradients <= 8e-13 -- inside 1e-8, so that bound holds."""
    g = IC.load_golden("fno_unroll3")
    params, batch, s = IC.golden_case(g)
    K_, lseed = int(g["meta"][13]), int(g["meta"][14])
    ref = IC.cached(("unroll_ref",), lambda: IC.ref_unroll(params, batch, IC.unroll_labels(lseed, batch, K_), s["L"]))
    res = {"preds": IC.golden_field(g, "preds", np.stack(ref["preds"]))}
    res.update(g_inputs=IC.golden_field(g, "g_inputs", ref["g_inputs"]), g_case_params=IC.nm(ref["g_case_params"], g["g_case_params"]))
    res.update(IC.golden_gsums(g, ref["grads"]))
    print("fno_unroll3 fixture vs fp64:", res, "loss", ref["loss"], float(g["loss"]))
    assert abs(ref["loss"] - float(g["loss"])) / ref["loss"] < 2e-6
    _assert_all(res, MODEL_TOL)


# ---- 1. the reference's numbers through the C ABI ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", IC.REFERENCE_GOLDENS + ["fno_ingrad_c3"])
def test_golden_input_gradients(be, name):
    res, _ = IC.check_golden(be, name)
    _assert_all(res, MODEL_TOL)


def test_route_steps_aside_and_flags_are_ignored(be):
    """64 x 64, C = 8, in_chan = 2: the shape on which the lifting layer's fused sums (stemg) are on.  With the pointers set the phases give
    the reference's g_inputs, and flags = 7 equals flags = 0 bit for bit."""
    res0, out0 = IC.check_golden(be, "fno_small_64x64", route="phases", flags=0)
    res7, out7 = IC.check_golden(be, "fno_small_64x64", route="phases", flags=7)
    _assert_all(res0, MODEL_TOL)
    assert IC.bits_equal(out0, out7) == 0.0


# ---- 2. small shapes against fp64 -------------------------------------------------------------------------------------------------
# (B, C, L, H, W, m1, m2, p, cin, pad, kwargs)
SMALL = {
    "9x7_scalar_form": (3, 6, 2, 9, 7, 4, 4, 5, 2, 0, {}),
    "66x65_8byte_form": (1, 6, 1, 66, 65, 12, 12, 5, 2, 0, {}),
    "p0_cin1": (1, 5, 1, 8, 8, 2, 3, 0, 1, 0, {}),
    "p8_cin3": (2, 7, 1, 8, 8, 2, 3, 8, 3, 0, {}),
    "c33": (1, 33, 1, 8, 8, 2, 3, 5, 2, 0, {}),
    "c128": (1, 128, 1, 8, 8, 2, 3, 5, 2, 0, {}),
    "12x12_pad4": (2, 6, 2, 12, 12, 4, 4, 5, 2, 4, {}),
    "no_layers": (2, 6, 0, 8, 8, 2, 3, 5, 2, 0, {}),
    "no_mask": (2, 6, 1, 8, 8, 2, 3, 5, 2, 0, dict(with_mask=False)),
    "gext_and_label": (2, 6, 1, 8, 8, 2, 3, 5, 2, 0, dict(with_gext=True)),
    "gext_alone": (2, 6, 1, 8, 8, 2, 3, 5, 2, 0, dict(with_gext=True, with_label=False)),
    "cin8_ni8_form": (2, 6, 1, 8, 8, 2, 3, 5, 8, 0, {}),
    "cin9_two_groups": (2, 6, 1, 8, 8, 2, 3, 5, 9, 0, dict(cout=2)),
}
WANTS = {"both": ("inputs", "case_params"), "inputs": ("inputs",), "case_params": ("case_params",)}


@pytest.mark.parametrize("want", list(WANTS))
@pytest.mark.parametrize("case", list(SMALL))
def test_small_shapes_vs_fp64(be, case, want):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    _assert_all(IC.check_small(be, B, C, L, H, W, m1, m2, p, cin, pad, want=WANTS[want], **kw), ABI_TOL)


def test_small_shape_through_the_phases(be):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL["9x7_scalar_form"]
    _assert_all(IC.check_small(be, B, C, L, H, W, m1, m2, p, cin, pad, route="phases"), ABI_TOL)


# ---- 3. placement -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [4, 8])
@pytest.mark.parametrize("case", ["p8_cin3", "66x65_8byte_form"])
def test_misaligned_buffers(be, case, shift):
    """Every tensor -- d_inputs and d_case_params among them -- `shift` bytes past a 16-byte boundary."""
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    with be.misaligned(shift):
        res = IC.check_small(be, B, C, L, H, W, m1, m2, p, cin, pad)
        assert be.allocations >= 10
    _assert_all(res, ABI_TOL)


# ---- 4. nothing else moves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["p8_cin3", "12x12_pad4", "c33"])
def test_nothing_else_moves(be, case):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    res = IC.check_nothing_else_moves(be, B, C, L, H, W, m1, m2, p, cin, pad)
    assert res == dict(preds_sums=0.0, param_grads=0.0), res


def test_nothing_else_moves_where_the_fused_sums_are_on(be):
    """64 x 64, C = 8: without the pointers the lifting layer's gradient comes from the fused sums; with them from the stand-alone pass --
    the bits of cfd_tune_set("stem_fuse", 0)."""
    res = IC.check_nothing_else_moves(be, 1, 8, 1, 64, 64, 12, 12, 5, 2)
    assert res == dict(preds_sums=0.0, param_grads=0.0), res


def test_fused_step_with_null_pointers_still_defers(be):
    """What this checks is behaviour, not bits against a recording: fno_checks.run_fused_steps fills a zeroed struct (both pointers NULL)
    and the deferrals stay on.  Under flags = 7 the raw first gradient is still short of the nMSE normaliser count / sum (label mask)^2 =
    sums[3] / sums[2] -- times that factor it is the flags = 0 gradient -- while the predictions are the same bits and the parameters
    after two steps agree.  That the default step keeps its bits is what the unchanged suite (its fixtures and bitwise checks) holds."""
    params, batch = IC.small_case(1, 8, 1, 64, 64, 12, 12, 5, 2)
    out, layout = IC.F.run_fused_steps(be, params, batch, 1, 8, 64, 64, 5)
    a, b = out[0], out[7]
    factor = float(b["sums1"][3]) / float(b["sums1"][2])
    assert abs(factor - 1.0) > 1e-3, factor  # (so that a gradient without the deferral is told from one with it: nMSE >= 1e-6 apart)
    assert IC.nm(b["g1"], a["g1"]) > 1e-7, "flags = 7 no longer defers the normaliser"
    assert IC.nm(b["g1"] * np.float32(factor), a["g1"]) < 1e-9
    assert np.array_equal(a["preds1"], b["preds1"])
    assert IC.nm(b["flat"], a["flat"]) < 1e-9


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["p8_cin3", "66x65_8byte_form"])
def test_two_calls_on_a_dirty_workspace_give_the_same_bits(be, case):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    params, batch = IC.small_case(B, C, L, H, W, m1, m2, p, cin, pad)
    first, second = IC.run_ingrad(be, params, batch, L, C, H, W, p, m1, m2, pad, repeat=2)
    assert IC.bits_equal(first, second) == 0.0


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------
# a shape that bf16-storage training takes (out_chan <= 2, hidden <= 32, pad = 0, narrow modes), so that a refusal is the fields' doing
BF16_OK = (2, 7, 1, 8, 8, 2, 3, 8, 2, 0)


def test_bf16_storage_runs_without_the_pointers(be):
    B, C, L, H, W, m1, m2, p, cin, pad = BF16_OK
    params, batch = IC.small_case(B, C, L, H, W, m1, m2, p, cin, pad)
    out = IC.run_ingrad(be, params, batch, L, C, H, W, p, m1, m2, pad, want=(), route="phases", act_dtype=1)
    assert "status" not in out and np.isfinite(out["preds"]).all() and all(np.isfinite(v).all() for v in out["grads"].values())


@pytest.mark.parametrize("route", ["phases", "phases_only", "adam_only"])
@pytest.mark.parametrize("want", ["inputs", "case_params"])
def test_bf16_storage_is_refused(be, route, want):
    """On the shape of the test above, either pointer alone makes the training forward, a backward phase and cfd_fno_adam_step return
    CFD_ERR_UNSUPPORTED before anything is launched: every output is still poison."""
    B, C, L, H, W, m1, m2, p, cin, pad = BF16_OK
    params, batch = IC.small_case(B, C, L, H, W, m1, m2, p, cin, pad)
    res = IC.run_ingrad(be, params, batch, L, C, H, W, p, m1, m2, pad, want=WANTS[want], route=route, act_dtype=1)
    assert res == dict(status=-2, poisoned=True), res


# ---- 7. the chain rule through the ABI ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["p8_cin3", "12x12_pad4"])
def test_chain_rule_over_two_steps(be, case):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    _assert_all(IC.check_chain(be, B, C, L, H, W, m1, m2, p, cin, pad), ABI_TOL)
