"""CPU: host side of the Sobolev objective -- the two entry points in the header and the binding, the size macro, the loss classes, the
flags with their validation and directory suffix, the refusals of the engine and the trainer -- and tests/sobolev_checks.reference
against the fixture made from the reference's HsLoss (tools/make_golden_hsloss.py).  The kernels and the engine:
tests/test_emul_sobolev.py, tests/test_gpu_sobolev.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from cfdbench_amd import _capi
from tests import objective_checks as OC
from tests import sobolev_checks as SC

REPO = Path(__file__).resolve().parent.parent
GRIDS = ((5, 7), (6, 9))


# ---- header and binding ----------------------------------------------------------------------------------------------------------
def test_header_signatures_and_the_binding():
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    flat = lambda s: " ".join(s.split())  # noqa: E731
    fwd = flat(re.search(r"^int cfd_sobolev_fwd\(([^;]*)\);", header, flags=re.M).group(1))
    bwd = flat(re.search(r"^int cfd_sobolev_bwd\(([^;]*)\);", header, flags=re.M).group(1))
    assert fwd == ("const float* preds, const float* label, const float* mask, float* rec, float* value, int B, int Co, int H, int W, int k, "
                   "float a1, float a2, int balanced, void* stream")
    assert bwd == ("const float* preds, const float* label, const float* mask, const float* rec, const float* gadd, const float* upstream_dev, "
                   "float upstream, float* gpreds, int B, int Co, int H, int W, int k, float a1, float a2, int balanced, void* stream")
    I, P, F = _capi._I, _capi._P, _capi._F
    assert _capi._SIGS["cfd_sobolev_fwd"] == (I, [P] * 5 + [I] * 5 + [F, F, I, P])
    assert _capi._SIGS["cfd_sobolev_bwd"] == (I, [P] * 6 + [F, P] + [I] * 5 + [F, F, I, P])
    # no size function and no plan; ABI 604 and the objectives' ids stay
    assert not re.search(r"size_t\s+cfd_sobolev", header) and "cfd_sobolev_plan" not in header
    assert _capi.ABI_VERSION == 604 and "#define CFD_ABI_VERSION 604" in header
    assert _capi.OBJECTIVE_IDS == {"rel_l2": 0, "nmse_sample": 1, "nmse_channel": 2}


def test_header_states_the_rule_and_the_macro_matches():
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    para = header[header.index("Sobolev objective (FnoTrainEngine"):header.index("#define CFD_HS_REC_FLOATS")]
    for word in ("kx(i) = i if i < H / 2", "0 1 3 2 1", "E_t[b] = sum r^t |Dh|^2", "balanced 1", "v_mfma_f32_16x16x4_f32", "(-i, W - l)",
                 "2 <= H, W <= 128", "CFD_ERR_UNSUPPORTED", "CFD_ERR_INVALID_ARG", "No atomics", "gpreds may alias gadd"):
        assert word in para, word
    macro = re.search(r"#define CFD_HS_REC_FLOATS\(B, Co\) (.*)", header).group(1)
    expr = macro.replace("(size_t)", "")
    for B, Co in ((1, 1), (3, 2), (256, 8)):
        assert eval(expr, {}, dict(B=B, Co=Co)) == _capi.CFD_HS_REC_FLOATS(B, Co) == 2 + 12 * B + 12 * B * Co


def test_exported_by_the_library():
    assert {"cfd_sobolev_fwd", "cfd_sobolev_bwd"} <= set(_capi.exported_symbols())


# ---- Python layers ---------------------------------------------------------------------------------------------------------------
def test_loss_classes_and_names():
    from cfdbench_amd import functional
    from cfdbench_amd.models.loss import MseLoss, ObjectiveLoss, SobolevLoss, objective_to_fn
    from cfdbench_amd.sobolev import SobolevLossFn, hs_arguments
    fn = objective_to_fn("hs")
    assert isinstance(fn, SobolevLoss) and isinstance(fn, MseLoss) and fn.normalize and fn.objective == "hs"
    assert fn.get_score_names() == ["mse", "rmse", "mae", "nmse", "hs"] and (fn.hs_k, fn.hs_a, fn.hs_group) == (1, None, False)
    fn = objective_to_fn("HS", k=2, a=[0.5, 0.25], group=True)
    assert (fn.hs_k, fn.hs_a, fn.hs_group) == (2, (0.5, 0.25), True)
    assert type(objective_to_fn("rel_l2")) is ObjectiveLoss and type(objective_to_fn("nmse")) is MseLoss
    for bad in ("l2", "rel", ""):
        with pytest.raises(NotImplementedError):
            objective_to_fn(bad)
    with pytest.raises(ValueError):
        objective_to_fn("rel_l2", k=2)
    for bad in (dict(k=0), dict(k=3), dict(k=2, a=[1.0])):
        with pytest.raises(ValueError):
            SobolevLoss(**bad)
    assert hs_arguments() == (1, 1.0, 1.0, 0) and hs_arguments(2, [0.5, 0.25], True) == (2, 0.5, 0.25, 1)
    sig = inspect.signature(functional.sobolev_loss).parameters
    assert [sig[n].default for n in ("mask", "k", "a", "group")] == [None, 1, None, False]
    assert issubclass(SobolevLossFn, torch.autograd.Function) and not hasattr(functional, "SobolevLossFn")


def test_flags_validation_and_directory():
    from cfdbench_amd.harness.args import _FLAGS, ALL_OBJECTIVES, OBJECTIVES, Args, hs_arguments_of, is_args_valid
    from cfdbench_amd.harness.common import get_output_dir
    assert OBJECTIVES == ("nmse", "rel_l2", "nmse_sample", "nmse_channel") and ALL_OBJECTIVES == OBJECTIVES + ("hs",)
    assert (_FLAGS["hs_k"], _FLAGS["hs_a"], _FLAGS["hs_group"]) == (1, "", 0)
    base = ["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse"]
    plain = Args().parse_args(base)
    is_args_valid(plain)
    assert hs_arguments_of(plain) == {} and "obj" not in str(get_output_dir(plain, is_auto=True))
    for extra, suffix, want in (
            (["--objective", "hs"], "_obj-hs-k1", dict(k=1, a=None, group=False)),
            (["--objective", "hs", "--hs_k", "2", "--fused", "1"], "_obj-hs-k2", dict(k=2, a=None, group=False)),
            (["--objective", "hs", "--hs_k", "2", "--hs_a", "0.5,0.25"], "_obj-hs-k2-a0.5,0.25", dict(k=2, a=(0.5, 0.25), group=False)),
            (["--objective", "hs", "--hs_k", "1", "--hs_a", "2", "--hs_group", "1", "--unroll_steps", "2"], "_obj-hs-k1-a2-grp",
             dict(k=1, a=(2.0,), group=True))):
        a = Args().parse_args(base + extra)
        is_args_valid(a)
        out = str(get_output_dir(a, is_auto=True))
        assert out.endswith(suffix) and out.startswith(str(get_output_dir(plain, is_auto=True))), out
        assert hs_arguments_of(a) == want
    ok = dict(model="fno", data_name="cavity_bc", loss_name="nmse", objective="hs")
    for bad in (dict(hs_k=3), dict(hs_k=0), dict(hs_group=2), dict(hs_a="x"), dict(hs_k=2, hs_a="1"), dict(hs_a="1,2"), dict(graph=1),
                dict(model="unet"), dict(dtype="bf16", fused=1), dict(loss_name="mse"), dict(objective="rel_l2", hs_k=2),
                dict(objective="nmse", hs_group=1), dict(objective="nmse", hs_a="1")):
        with pytest.raises(AssertionError):
            is_args_valid(Args(**{**ok, **bad}))


def _data():
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    return SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)


def _fno():
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    return Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4)


def test_engine_refusals_need_no_gpu():
    from cfdbench_amd.engine import FnoTrainEngine
    sig = inspect.signature(FnoTrainEngine.__init__).parameters
    assert [sig[n].default for n in ("hs_k", "hs_a", "hs_group")] == [None, None, None]
    for kw, match in ((dict(objective="hs", act_dtype="bf16"), "bf16"), (dict(objective="hs", loss_name="mse"), "loss_name"),
                      (dict(objective="hs", hs_k=3), "k = 3"), (dict(objective="hs", hs_k=2, hs_a=[1.0]), "coefficients"),
                      (dict(objective="rel_l2", hs_k=1), "hs_k"), (dict(hs_group=False), "hs_k"), (dict(objective="h1"), "objective must be")):
        with pytest.raises(ValueError, match=match):
            FnoTrainEngine(_fno(), **kw)


class _Built(Exception):
    pass


def test_trainer_refusals_and_what_it_hands_the_engine(tmp_path, monkeypatch):
    from cfdbench_amd.harness import train_auto as TA
    from cfdbench_amd.models.loss import SobolevLoss
    ds = _data()
    kw = dict(num_epochs=1, plot_interval=0)
    with pytest.raises(ValueError, match="hs_k"):
        TA.train(_fno(), ds, ds, tmp_path / "run", objective="rel_l2", hs_k=2, **kw)
    with pytest.raises(ValueError, match="k = 4"):
        TA.train(_fno(), ds, ds, tmp_path / "run", objective="hs", hs_k=4, **kw)
    with pytest.raises(NotImplementedError, match="graph"):
        TA.train(_fno(), ds, ds, tmp_path / "run", objective="hs", graph=True, **kw)
    with pytest.raises(NotImplementedError, match="bf16"):
        TA.train(_fno(), ds, ds, tmp_path / "run", objective="hs", fused=True, act_dtype="bf16", **kw)
    assert not (tmp_path / "run").exists()
    seen = {}

    def fake(model, **kwargs):
        seen.update(kwargs)
        raise _Built

    monkeypatch.setattr(TA, "FnoTrainEngine", fake)
    model = _fno()
    with pytest.raises(_Built):
        TA.train(model, ds, ds, tmp_path / "a", fused=True, objective="hs", hs_k=2, hs_a=(0.5, 0.25), hs_group=True, **kw)
    assert (seen["objective"], seen["hs_k"], seen["hs_a"], seen["hs_group"], seen["loss_name"]) == ("hs", 2, (0.5, 0.25), True, "nmse")
    assert isinstance(model.loss_fn, SobolevLoss) and model.loss_fn.get_score_names()[-1] == "hs"
    assert (model.loss_fn.hs_k, model.loss_fn.hs_a, model.loss_fn.hs_group) == (2, (0.5, 0.25), True)
    seen.clear()
    with pytest.raises(_Built):
        TA.train(_fno(), ds, ds, tmp_path / "b", fused=True, objective="rel_l2", **kw)
    assert seen["objective"] == "rel_l2" and not any(k.startswith("hs_") for k in seen)


# ---- the golden ------------------------------------------------------------------------------------------------------------------
def _golden():
    return np.load(REPO / "tests" / "golden" / "hsloss.npz")


def test_golden_is_what_the_issue_asks_for():
    g = _golden()
    assert [int(v) for v in g["meta"]] == [3, 2, 21, 5, 7, 6, 9]
    for H, W in GRIDS:
        p, lab, m = (g[f"g{H}x{W}_{n}"] for n in ("preds", "label", "mask"))
        assert p.dtype == lab.dtype == m.dtype == np.float32 and p.shape == lab.shape == (3, 2, H, W) and m.shape == (3, 1, H, W)
        assert set(np.unique(m)) <= {0.0, 1.0} and np.array_equal(p, p * m)
        for name in SC.SETTINGS:
            assert g[f"g{H}x{W}_{name}_grad"].dtype == np.float64 and g[f"g{H}x{W}_{name}_grad"].shape == p.shape
            assert g[f"g{H}x{W}_{name}_value"].dtype == np.float64
    assert (REPO / "tests" / "golden" / "hsloss.npz").stat().st_size < 32768  # (23 arrays, 7 KB of data)
    assert "set_default_dtype(torch.float64)" in (REPO / "tools" / "make_golden_hsloss.py").read_text()


@pytest.mark.parametrize("name", list(SC.SETTINGS))
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_fp64_rule_against_the_reference_golden(grid, name):
    """tests/sobolev_checks.reference (what every kernel test compares with) against HsLoss and its autograd gradient: fp64 both, 1e-12."""
    g = _golden()
    H, W = grid
    k, a, group = SC.SETTINGS[name]
    p, lab, m = (g[f"g{H}x{W}_{n}"] for n in ("preds", "label", "mask"))
    ref = SC.reference(p, lab, m[:, 0], k, a, group)
    value, want = float(g[f"g{H}x{W}_{name}_value"]), g[f"g{H}x{W}_{name}_grad"]
    assert abs(ref["value"] - value) <= 1e-12 * value
    assert np.max(np.abs(ref["grad"] - want)) <= 1e-12 * np.max(np.abs(want)) and np.any(want != 0.0)


def test_a1_zero_is_rel_l2():
    """Parseval: with a1 = 0, k = 1, not grouped, reference() is tests/objective_checks.reference(..., "rel_l2"), value and gradient."""
    preds, label, mask, gadd = SC.case(3, 2, 9, 12, seed=8)
    hs = SC.reference(preds, label, mask, 1, (0.0,), False, gadd, upstream=0.37)
    B, Co, H, W = preds.shape
    l2 = OC.reference(preds.reshape(B, Co, -1), label.reshape(B, Co, -1), mask.reshape(B, -1), "rel_l2", gadd.reshape(B, Co, -1), upstream=0.37)
    assert abs(hs["value"] - l2["value"]) <= 1e-13 * l2["value"]
    assert np.max(np.abs(hs["grad"].reshape(B, Co, -1) - l2["grad"])) <= 1e-13 * np.max(np.abs(l2["grad"]))


def test_the_emulation_follows_the_rule():
    """emulate(), which sets the bound of the kernel tests, is the same function as reference() up to fp32 rounding: well inside the ceiling."""
    preds, label, mask, gadd = SC.case(2, 2, 17, 33, seed=2)
    for name, (k, a, group) in SC.SETTINGS.items():
        ref, emu = SC.reference(preds, label, mask, k, a, group, gadd), SC.emulate(preds, label, mask, k, a, group, gadd)
        assert SC.rel_err(emu["value"], ref["value"]) <= 1e-6, name
        assert np.max(np.abs(emu["grad"] - ref["grad"])) <= 1e-6 * np.max(np.abs(ref["grad"])), name
        assert np.max(np.abs(emu["E"] / ref["E"] - 1.0)) <= 1e-6 and np.max(np.abs(emu["S"] / ref["S"] - 1.0)) <= 1e-6, name
