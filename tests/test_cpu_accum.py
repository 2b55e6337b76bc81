"""CPU: host logic of gradient accumulation in the fused FNO engine -- the two flag bits of cfd_fno_adam_step in the header and the binding,
--fused_accumulation_steps and what is_args_valid refuses with it, and train() taking fused + accumulation up to the engine's own
"move the model to the GPU" error.  The kernel: tests/test_emul_fno_accum.py, tests/test_gpu_fno_accum.py."""
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def test_flag_bits_agree_between_header_and_binding():
    from cfdbench_amd import _capi
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    bits = {name: int(re.search(rf"#define {name} (\d+)", header).group(1))
            for name in ("CFD_TRAIN_DEFER_SCALE", "CFD_TRAIN_DEFER_HEAD", "CFD_TRAIN_DEFER_STEM", "CFD_STEP_ACCUMULATE", "CFD_STEP_ACCUM_INIT")}
    assert bits == dict(CFD_TRAIN_DEFER_SCALE=1, CFD_TRAIN_DEFER_HEAD=2, CFD_TRAIN_DEFER_STEM=4, CFD_STEP_ACCUMULATE=8, CFD_STEP_ACCUM_INIT=16)
    assert _capi.CFD_STEP_ACCUMULATE == bits["CFD_STEP_ACCUMULATE"] and _capi.CFD_STEP_ACCUM_INIT == bits["CFD_STEP_ACCUM_INIT"]
    # the feature travels through an argument that exists: no new version, no new entry point
    assert _capi.ABI_VERSION == 604 == int(re.search(r"#define CFD_ABI_VERSION (\d+)", header).group(1))
    assert len(_capi._SIGS["cfd_fno_adam_step"][1]) == 25


def test_flag_and_validation():
    from cfdbench_amd.harness.args import Args, is_args_valid
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc"])
    assert args.fused_accumulation_steps == 1 and isinstance(args.fused_accumulation_steps, int)
    is_args_valid(args)
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--fused", "1", "--fused_accumulation_steps", "4", "--max_grad_norm", "1.0"])
    is_args_valid(args)
    assert args.fused_accumulation_steps == 4 and args.as_dict()["fused_accumulation_steps"] == 4
    for bad in (dict(fused_accumulation_steps=0), dict(fused_accumulation_steps=2),               # needs --fused 1
                dict(model="unet", fused_accumulation_steps=2), dict(graph=1, fused_accumulation_steps=2),
                dict(fused=1, graph=1, fused_accumulation_steps=2)):
        with pytest.raises(AssertionError):
            is_args_valid(Args(**dict(dict(model="fno", data_name="cavity_bc"), **bad)))
    # the autograd path's flag stays refused with --fused 1, and the message names the flag to use instead
    with pytest.raises(AssertionError, match="--fused_accumulation_steps"):
        is_args_valid(Args(model="fno", data_name="cavity_bc", fused=1, gradient_accumulation_steps=2))
    is_args_valid(Args(model="fno", data_name="cavity_bc", gradient_accumulation_steps=2, fused_accumulation_steps=1))


def test_train_takes_fused_with_accumulation_up_to_the_engine(tmp_path, monkeypatch):
    """train(fused=True, gradient_accumulation_steps=2) on a CPU model: no NotImplementedError any more -- the first thing to object is the
    engine, which wants the model on the GPU.  unroll_steps > 1 keeps its refusals.  (The engine binds the product library before it
    looks at the model; the library is loaded with RTLD_GLOBAL and would shadow the emulator build's symbols for every later test of
    this process, so the loader is stubbed: nothing here reaches a C call.)"""
    from cfdbench_amd import _lib
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    monkeypatch.setattr(_lib, "api", lambda: None)
    from cfdbench_amd.harness.train_auto import train
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)
    model = Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4)
    with pytest.raises(RuntimeError, match="move the model to the GPU"):
        train(model, ds, ds, tmp_path / "run", num_epochs=1, fused=True, gradient_accumulation_steps=2, plot_interval=0)
    with pytest.raises(NotImplementedError, match="unroll_steps"):
        train(model, ds, ds, tmp_path / "run", num_epochs=1, fused=True, gradient_accumulation_steps=2, unroll_steps=2, plot_interval=0)


def test_main_hands_the_fused_flag_to_train(monkeypatch, tmp_path):
    """main() passes --fused_accumulation_steps as train()'s gradient_accumulation_steps when --fused 1, --gradient_accumulation_steps otherwise."""
    import torch

    from cfdbench_amd.harness import data as D
    from cfdbench_amd.harness import train_auto as T
    seen = []
    ds = D.SyntheticAutoDataset(n_cases=1, n_frames=3, height=8, width=8, seed=0)
    monkeypatch.setattr(D, "get_auto_dataset", lambda **kw: (ds, ds, ds))
    monkeypatch.setattr(T, "init_distributed", lambda: (0, 1))
    monkeypatch.setattr(T, "train", lambda model, **kw: seen.append((kw["fused"], kw["gradient_accumulation_steps"])))
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    common = ["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--mode", "train", "--fno_hidden_dim", "4", "--fno_depth", "1",
              "--output_dir", str(tmp_path)]
    T.main(common + ["--fused", "1", "--fused_accumulation_steps", "3"])
    T.main(common + ["--gradient_accumulation_steps", "2"])
    assert seen == [(True, 3), (False, 2)]
