"""CPU: host side of the training objectives -- the two entry points in the header and the binding, the size macro, the loss classes, the
command-line flag and what the trainer refuses with it, that the default leaves the loop alone, and the reference-pinned fixture
tests/golden/lploss_rel.npz (tools/make_golden_lploss.py) against the fp64 formula that the kernel tests use as their reference.  The
kernels and the engine: tests/test_emul_fno_objective.py, tests/test_gpu_fno_objective.py."""
import inspect
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import objective_checks as OC
from tests.test_cpu_guard import _ToyAuto

REPO = Path(__file__).resolve().parent.parent
KINDS = ("rel_l2", "nmse_sample", "nmse_channel")


def test_entries_in_header_and_binding():
    from cfdbench_amd import _capi
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    flat = lambda text: [" ".join(a.split()) for a in text.split(",")]  # noqa: E731
    fwd = flat(re.search(r"^int cfd_objective_fwd\(([^;]*)\);", header, flags=re.M).group(1))
    bwd = flat(re.search(r"^int cfd_objective_bwd\(([^;]*)\);", header, flags=re.M).group(1))
    assert fwd == ["const float* preds", "const float* label", "const float* mask", "float* rec", "float* value", "int B", "int Co", "int HW",
                   "int kind", "void* stream"]
    assert bwd == ["const float* preds", "const float* label", "const float* mask", "const float* rec", "const float* gadd",
                   "const float* upstream_dev", "float upstream", "float* gpreds", "int B", "int Co", "int HW", "int kind", "void* stream"]
    P, I, F = _capi._P, _capi._I, _capi._F
    assert _capi._SIGS["cfd_objective_fwd"] == (I, [P] * 5 + [I] * 4 + [P])
    assert _capi._SIGS["cfd_objective_bwd"] == (I, [P] * 6 + [F, P] + [I] * 4 + [P])
    assert {"cfd_objective_fwd", "cfd_objective_bwd"} <= set(_capi.exported_symbols())
    # no ABI bump, no struct field, no flag bit, no size function
    assert _capi.ABI_VERSION == 604 == int(re.search(r"#define CFD_ABI_VERSION (\d+)", header).group(1))
    assert [f[0] for f in _capi.FnoParams._fields_][-2:] == ["clip", "max_grad_norm"]
    assert sorted(int(v) for v in re.findall(r"#define CFD_(?:TRAIN_DEFER|STEP)_\w+ (\d+)", header)) == [1, 2, 4, 8, 16, 32, 64]
    assert not re.search(r"size_t\s+cfd_objective", header)
    ids = {k: int(re.search(rf"#define CFD_OBJ_{k.upper()} (\d+)", header).group(1)) for k in KINDS}
    assert ids == _capi.OBJECTIVE_IDS == {"rel_l2": 0, "nmse_sample": 1, "nmse_channel": 2}


def test_header_states_definitions_and_alignment():
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    para = header[header.index("Training objectives beside mse / nmse / mae"):header.index("#define CFD_OBJ_REL_L2")]
    low = " ".join(" ".join(re.sub(r"^\s*\*", "", line) for line in para.splitlines()).lower().split())
    for words in ("d = preds - label * mask", "sum_b sqrt(e_b) / sqrt(s_b)", "2 d / (b s_b)", "2 d / (co s_c)", "e_b == 0: 0", "lploss(d=2, p=2).rel",
                  "two launches", "one launch (three for fwd + bwd)", "no atomics: two calls give the same bits", "any 4-byte boundary",
                  "gpreds may alias gadd", "rounded once", "rec[0..1] the batch-global sum d^2", "cfd_err_invalid_arg", "not special-cased"):
        assert words in low, words


def test_rec_floats_in_python_equals_the_header_macro(tmp_path):
    """The macro through a C compiler against the binding's function, at shapes on both sides of B == Co."""
    from cfdbench_amd._capi import CFD_OBJ_MAX_PARTS, CFD_OBJ_REC_FLOATS
    from tests.emul.build_emul import CLANG
    shapes = [(1, 1), (2, 2), (3, 8), (8, 3), (256, 2), (5, 8), (1024, 1)]
    src = tmp_path / "rec.c"
    calls = "\n".join(f'    printf("%zu\\n", (size_t)CFD_OBJ_REC_FLOATS({b}, {c}));' for b, c in shapes)
    src.write_text(f'#include <stdio.h>\n#include "cfdbench_amd.h"\nint main(void) {{\n    printf("%d\\n", CFD_OBJ_MAX_PARTS);\n{calls}\n    return 0;\n}}\n')
    subprocess.run([CLANG.replace("clang++", "clang"), "-x", "c", f"-I{REPO / 'include'}", str(src), "-o", str(tmp_path / "rec")], check=True)
    out = [int(v) for v in subprocess.run([str(tmp_path / "rec")], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == CFD_OBJ_MAX_PARTS == OC.MAX_PARTS
    assert out[1:] == [CFD_OBJ_REC_FLOATS(b, c) for b, c in shapes]
    assert CFD_OBJ_REC_FLOATS(256, 2) == 8 + 4 * 256 + 4 * 512 * 8


def test_loss_classes_and_names():
    from cfdbench_amd.models.loss import MseLoss, ObjectiveLoss, loss_name_to_fn, objective_to_fn
    for k in KINDS:
        fn = objective_to_fn(k)
        assert isinstance(fn, ObjectiveLoss) and isinstance(fn, MseLoss) and fn.normalize and fn.objective == k
        assert fn.get_score_names() == ["mse", "rmse", "mae", "nmse", k]
        with pytest.raises(NotImplementedError):
            loss_name_to_fn(k)  # (the reference's function keeps its two names)
    assert type(objective_to_fn("nmse")) is MseLoss and objective_to_fn("NMSE").get_score_names() == ["mse", "rmse", "mae", "nmse"]
    assert objective_to_fn("mse").get_score_names() == ["mse", "rmse", "mae"]
    for bad in ("l2", "rel", ""):
        with pytest.raises(NotImplementedError):
            objective_to_fn(bad)
        with pytest.raises(NotImplementedError):
            loss_name_to_fn(bad)
        with pytest.raises(NotImplementedError):
            ObjectiveLoss(bad)
    from cfdbench_amd import functional
    with pytest.raises(NotImplementedError):
        functional.objective_loss(torch.zeros(1, 1, 2), torch.zeros(1, 1, 2), "l2")
    assert inspect.signature(functional.objective_loss).parameters["mask"].default is None
    from cfdbench_amd.unroll import unrolled_loss
    assert inspect.signature(unrolled_loss).parameters["key"].default == "nmse"


def test_flag_and_validation():
    from cfdbench_amd.harness.args import _FLAGS, OBJECTIVES, Args, is_args_valid
    from cfdbench_amd.harness.common import get_output_dir
    assert OBJECTIVES == ("nmse",) + KINDS
    base = ["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse"]
    args = Args().parse_args(base)
    is_args_valid(args)
    # the default: every other key of args.json keeps its value, the result directory its name
    assert args.objective == "nmse" and set(args.as_dict()) == set(_FLAGS)
    plain = {k: v for k, v in Args().parse_args(base).as_dict().items() if k != "objective"}
    assert plain == {k: (v if k not in ("model", "data_name", "loss_name") else getattr(args, k)) for k, v in _FLAGS.items() if k != "objective"}
    assert "obj" not in str(get_output_dir(args, is_auto=True))
    for k in KINDS:
        for extra in ([], ["--fused", "1", "--fused_accumulation_steps", "2", "--unroll_steps", "2", "--max_grad_norm", "1.0", "--skip_nonfinite", "1",
                           "--ema_decay", "0.9", "--freeze", "fc0"]):
            a = Args().parse_args(base + ["--objective", k] + extra)
            is_args_valid(a)
            assert a.as_dict()["objective"] == k and str(get_output_dir(a, is_auto=True)).endswith(f"_obj-{k}")
            assert str(get_output_dir(a, is_auto=True)).startswith(str(get_output_dir(args, is_auto=True)))
    for bad in (dict(objective="l2"), dict(objective="rel_l2", graph=1), dict(objective="rel_l2", model="unet"),
                dict(objective="nmse_sample", dtype="bf16", fused=1), dict(objective="nmse_channel", loss_name="mse")):
        with pytest.raises(AssertionError):
            is_args_valid(Args(**{**dict(model="fno", data_name="cavity_bc", loss_name="nmse"), **bad}))
    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.harness import train_auto as TA
    assert inspect.signature(TA.train).parameters["objective"].default == "nmse"
    assert inspect.signature(FnoTrainEngine.__init__).parameters["objective"].default is None


def _data():
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    return SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)


def _fno():
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    return Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4)


def test_trainer_refusals_come_before_the_directory_is_made(tmp_path):
    from cfdbench_amd.harness.train_auto import train
    ds = _data()
    kw = dict(num_epochs=1, plot_interval=0)
    with pytest.raises(ValueError, match="objective"):
        train(_fno(), ds, ds, tmp_path / "run", objective="l2", **kw)
    with pytest.raises(NotImplementedError, match="fno model"):
        train(_ToyAuto(), ds, ds, tmp_path / "run", objective="rel_l2", **kw)
    with pytest.raises(NotImplementedError, match="graph"):
        train(_fno(), ds, ds, tmp_path / "run", objective="rel_l2", graph=True, **kw)
    with pytest.raises(NotImplementedError, match="bf16"):
        train(_fno(), ds, ds, tmp_path / "run", objective="nmse_sample", fused=True, act_dtype="bf16", **kw)
    assert not (tmp_path / "run").exists()


class _Built(Exception):
    pass


def test_the_default_builds_the_engine_it_always_built(tmp_path, monkeypatch):
    """--fused 1: with the default the engine is constructed without the new argument, call for call; with an objective it gets it, and the
    model's loss reports the objective last."""
    from cfdbench_amd.harness import train_auto as TA
    seen = {}

    def fake(model, **kw):
        seen.update(kw)
        raise _Built

    monkeypatch.setattr(TA, "FnoTrainEngine", fake)
    ds = _data()
    model = _fno()
    with pytest.raises(_Built):
        TA.train(model, ds, ds, tmp_path / "a", num_epochs=1, plot_interval=0, fused=True)
    assert "objective" not in seen and seen["loss_name"] == "nmse" and model.loss_fn.get_score_names() == ["mse", "rmse", "mae", "nmse"]
    seen.clear()
    with pytest.raises(_Built):
        TA.train(model, ds, ds, tmp_path / "b", num_epochs=1, plot_interval=0, fused=True, objective="nmse_channel")
    assert seen["objective"] == "nmse_channel" and seen["loss_name"] == "nmse"
    assert model.loss_fn.get_score_names()[-1] == "nmse_channel"


def test_the_default_writes_the_files_it_always_wrote(tmp_path, monkeypatch):
    from functools import partial

    from cfdbench_amd.harness import train_auto as TA
    monkeypatch.setattr(TA, "collate_fn", partial(TA.collate_fn, device=None))
    ds = _data()
    torch.manual_seed(5)
    TA.train(_ToyAuto(), ds, ds, tmp_path / "plain", num_epochs=1, batch_size=2, eval_batch_size=4, eval_interval=1, log_interval=100,
             plot_interval=0, lr=1e-2, objective="nmse")
    state = torch.load(tmp_path / "plain" / "train_state.pt", map_location="cpu", weights_only=False)
    assert "objective" not in state and "train_objective" not in state
    assert not (tmp_path / "plain" / "train_objective.json").exists() and not (tmp_path / "plain" / "ckpt-0" / "train_objective.json").exists()
    state["objective"] = "rel_l2"
    torch.save(state, tmp_path / "plain" / "train_state.pt")
    with pytest.raises(RuntimeError, match="--objective rel_l2"):
        TA.train(_ToyAuto(), ds, ds, tmp_path / "plain", num_epochs=2, batch_size=2, eval_batch_size=4, eval_interval=1, log_interval=100,
                 plot_interval=0, lr=1e-2, resume=True)


def test_engine_refusals_need_no_gpu():
    """bf16 storage, another loss_name and an unknown name: ValueError before anything touches the device."""
    from cfdbench_amd.engine import FnoTrainEngine
    for kw, match in ((dict(objective="rel_l2", act_dtype="bf16"), "bf16"), (dict(objective="rel_l2", loss_name="mse"), "loss_name"),
                      (dict(objective="l2"), "objective must be")):
        with pytest.raises(ValueError, match=match):
            FnoTrainEngine(_fno(), **kw)


# ---- the golden ------------------------------------------------------------------------------------------------------------------
def _golden():
    g = np.load(REPO / "tests" / "golden" / "lploss_rel.npz")
    B, Co, H, W = (int(v) for v in g["meta"][:4])
    return g, (B, Co, H * W)


def test_golden_is_what_the_issue_asks_for():
    g, (B, Co, HW) = _golden()
    assert (B, Co, HW) == (3, 2, 35) and g["preds"].dtype == g["label"].dtype == g["mask"].dtype == np.float32
    assert g["grad"].dtype == np.float64 and g["value"].dtype == np.float64 and g["grad"].shape == g["preds"].shape == (3, 2, 5, 7)
    assert set(np.unique(g["mask"])) <= {0.0, 1.0} and np.array_equal(g["preds"], g["preds"] * g["mask"])


def test_fp64_formula_against_the_reference_golden():
    """tests/objective_checks.reference (what every kernel test compares with) against LpLoss().rel and its autograd gradient: fp64 both."""
    g, (B, Co, HW) = _golden()
    ref = OC.reference(g["preds"].reshape(B, Co, HW), g["label"].reshape(B, Co, HW), g["mask"].reshape(B, HW), "rel_l2")
    assert abs(ref["value"] - float(g["value"])) <= 1e-14 * float(g["value"])
    want = g["grad"].reshape(B, Co, HW)
    assert np.max(np.abs(ref["grad"] - want)) <= 1e-14 * np.max(np.abs(want))
    assert np.any(want != 0.0)


def test_fp64_formulas_against_torch_autograd():
    """The gradients reference() states in closed form, for every kind, against torch's fp64 autograd of the value's formula."""
    preds, label, mask, gadd = OC.case(3, 2, 37, seed=9)
    for kind in KINDS:
        p = torch.from_numpy(preds.astype(np.float64)).requires_grad_(True)
        lm = torch.from_numpy(label.astype(np.float64)) * torch.from_numpy(mask.astype(np.float64))[:, None, :]
        d = p - lm
        E, S = (d * d).sum(-1), (lm * lm).sum(-1)
        value = {"rel_l2": (E.sum(1).sqrt() / S.sum(1).sqrt()).mean(), "nmse_sample": (E.sum(1) / S.sum(1)).mean(),
                 "nmse_channel": (E.sum(0) / S.sum(0)).mean()}[kind]
        (0.37 * value).backward()
        ref = OC.reference(preds, label, mask, kind, gadd, upstream=0.37)
        assert abs(ref["value"] - float(value.detach())) <= 1e-14 * abs(float(value.detach())), kind
        assert np.max(np.abs(ref["term"] - p.grad.numpy())) <= 1e-14 * np.max(np.abs(p.grad.numpy())), kind
        assert np.array_equal(ref["grad"], gadd.astype(np.float64) + ref["term"])
