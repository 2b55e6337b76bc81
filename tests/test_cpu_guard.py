"""CPU: host side of --skip_nonfinite -- the flag bit of cfd_fno_adam_step in the header and the binding, what the header says about it,
the two command-line flags and what the trainers refuse with them, the eager paths' skip (common.SkipGuard) and the abort after N
consecutive skips.  The kernel and the engine: tests/test_emul_fno_guard.py, tests/test_gpu_fno_guard.py."""
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


def test_flag_bit_agrees_between_header_and_binding():
    from cfdbench_amd import _capi
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    assert int(re.search(r"#define CFD_STEP_SKIP_NONFINITE (\d+)", header).group(1)) == 64 == _capi.CFD_STEP_SKIP_NONFINITE
    older = {n: int(re.search(rf"#define {n} (\d+)", header).group(1)) for n in
             ("CFD_TRAIN_DEFER_SCALE", "CFD_TRAIN_DEFER_HEAD", "CFD_TRAIN_DEFER_STEM", "CFD_STEP_ACCUMULATE", "CFD_STEP_ACCUM_INIT",
              "CFD_STEP_DECOUPLED_WD")}
    assert list(older.values()) == [1, 2, 4, 8, 16, 32]
    assert (_capi.CFD_STEP_ACCUMULATE, _capi.CFD_STEP_ACCUM_INIT, _capi.CFD_STEP_DECOUPLED_WD) == (8, 16, 32)
    assert _capi.ABI_VERSION == 604 == int(re.search(r"#define CFD_ABI_VERSION (\d+)", header).group(1))
    assert _capi.CFD_CLIP_FLOATS == 1024 == int(re.search(r"#define CFD_CLIP_FLOATS (\d+)", header).group(1))
    # the counters' places: the last two floats, named in the header
    assert re.search(r"#define CFD_CLIP_SKIPPED \(CFD_CLIP_FLOATS - 1\)", header) and _capi.CFD_CLIP_SKIPPED == 1023
    assert re.search(r"#define CFD_CLIP_CONSECUTIVE \(CFD_CLIP_FLOATS - 2\)", header) and _capi.CFD_CLIP_CONSECUTIVE == 1022
    # cfd_fno_adam_step keeps its 25 arguments, in the header and in the binding
    decl = re.search(r"int cfd_fno_adam_step\(([^;]*)\);", header).group(1)
    assert len(decl.split(",")) == 25
    assert len(_capi._SIGS["cfd_fno_adam_step"][1]) == 25
    # the struct tails are the pinned ones
    assert [f[0] for f in _capi.FnoParams._fields_][-2:] == ["clip", "max_grad_norm"] and _capi.FnoShape._fields_[-1][0] == "pad"


def test_header_states_the_rule():
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    para = header[header.index("CFD_STEP_SKIP_NONFINITE  needs grads->clip"):header.index("#define CFD_TRAIN_DEFER_SCALE")]
    low = " ".join(" ".join(re.sub(r"^\s*\*", "", line) for line in para.splitlines()).lower().split())  # (the comment's text, one line)
    assert "together with cfd_step_accumulate the bit is ignored" in low
    assert "the bias corrections after a skip are those of t, not of t - skipped" in low and "advances it on a skipped step too" in low
    assert "counters untouched" in low and "cfd_err_invalid_arg" in low and "cfd_err_unsupported" in low
    define = re.search(r"#define CFD_STEP_SKIP_NONFINITE 64\s*/\*(.*?)\*/", header).group(1)
    assert "cfd_fno_adam_step only" in define and "ignored with CFD_STEP_ACCUMULATE" in define


def test_flags_and_validation():
    from cfdbench_amd.harness.args import Args, is_args_valid
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc"])
    assert args.skip_nonfinite == 0 and args.max_consecutive_skips == 100
    is_args_valid(args)
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--fused", "1", "--skip_nonfinite", "1", "--max_consecutive_skips", "0"])
    is_args_valid(args)
    assert args.as_dict()["skip_nonfinite"] == 1 and args.as_dict()["max_consecutive_skips"] == 0
    is_args_valid(Args(model="unet", data_name="cavity_bc", skip_nonfinite=1))
    for bad in (dict(graph=1, skip_nonfinite=1), dict(skip_nonfinite=2), dict(skip_nonfinite=1, max_consecutive_skips=-1)):
        with pytest.raises(AssertionError):
            is_args_valid(Args(model="fno", data_name="cavity_bc", **bad))
    from cfdbench_amd.harness import train as T
    from cfdbench_amd.harness import train_auto as TA
    for fn in (T.train, TA.train):
        sig = inspect.signature(fn).parameters
        assert sig["skip_nonfinite"].default is False and sig["max_consecutive_skips"].default == 100


class _ToyAuto(torch.nn.Module):
    """CPU stand-in with the AutoCfdModel call interface (the product models run on the GPU only): a trainable 1 x 1 mix of the input
    fields plus a learned weight on the first case parameter, masked; mse and nmse as the product's loss functions name them."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.mix = torch.nn.Conv2d(2, 2, 1)
        self.cp = torch.nn.Parameter(torch.tensor(0.01))

    class _Loss:
        def get_score_names(self):
            return ["mse", "nmse"]

        def __call__(self, preds, labels):
            mse = torch.mean((preds - labels) ** 2)
            return dict(mse=mse, nmse=mse / torch.mean(labels ** 2))

    loss_fn = _Loss()

    def forward(self, inputs, label, case_params, mask):
        preds = (self.mix(inputs) + self.cp * case_params[:, :1, None, None]) * mask
        return dict(preds=preds, loss=self.loss_fn(preds=preds, labels=label))


def _model():
    return _ToyAuto()


def _data(bad_frame=True):
    """Two cases of five frames on 8 x 8; with `bad_frame` one value of case 0's frame 2 is NaN: the label of one item, the input of the next."""
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)
    if bad_frame:
        ds.all_features[0][2, 0, 3, 3] = np.nan
    return ds


@pytest.mark.parametrize("auto", [True, False])
def test_graph_with_the_guard_is_refused_before_the_directory_is_made(tmp_path, auto):
    if auto:
        from cfdbench_amd.harness.train_auto import train
    else:
        from cfdbench_amd.harness.train import train
    ds = _data(False)
    with pytest.raises(NotImplementedError, match="skip_nonfinite"):
        train(_model(), ds, ds, tmp_path / "run", num_epochs=1, graph=True, skip_nonfinite=True, plot_interval=0)
    assert not (tmp_path / "run").exists()


@pytest.fixture
def cpu_batches(monkeypatch):
    """The trainer's batches stay on the host: the eager loop then runs the CPU stand-in model end to end."""
    from functools import partial

    from cfdbench_amd.harness import train_auto as TA
    monkeypatch.setattr(TA, "collate_fn", partial(TA.collate_fn, device=None))


def _finite(model):
    return all(bool(torch.isfinite(torch.view_as_real(p_) if p_.is_complex() else p_).all()) for p_ in model.parameters())


def test_eager_path_skips_the_nonfinite_steps(tmp_path, capsys, cpu_batches):
    """train_auto on the CPU stand-in, batch size 1, two epochs: the two items that touch the NaN frame are skipped in each epoch, the
    weights stay finite, their losses stay out of the history, train_state.pt and the log line carry the count.  Without the flag the
    same run ends with NaN weights."""
    from cfdbench_amd.harness.train_auto import train
    kw = dict(num_epochs=2, batch_size=1, eval_batch_size=4, eval_interval=1, log_interval=4, plot_interval=0, lr=1e-2)
    model = _model()
    before = [p_.detach().clone() for p_ in model.parameters()]
    losses = train(model, _data(), _data(False), tmp_path / "guarded", skip_nonfinite=True, **kw)
    assert _finite(model) and any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert len(losses) == 2 * (8 - 2) and np.all(np.isfinite(losses))
    state = torch.load(tmp_path / "guarded" / "train_state.pt", map_location="cpu", weights_only=False)
    assert state["skipped_steps"] == 4
    assert "'skipped': " in capsys.readouterr().out
    plain = _model()
    train(plain, _data(), _data(False), tmp_path / "plain", **kw)
    assert not _finite(plain)
    assert "skipped_steps" not in torch.load(tmp_path / "plain" / "train_state.pt", map_location="cpu", weights_only=False)


def test_eager_accumulation_group_with_a_bad_micro_batch_is_dropped_whole(tmp_path):
    """The non-autoregressive trainer's loop with groups of two: SkipGuard.eager_step decides at the group's boundary."""
    from cfdbench_amd.harness.common import SkipGuard
    lin = torch.nn.Linear(3, 1)
    opt = torch.optim.Adam(lin.parameters(), lr=1e-2)
    guard = SkipGuard(True, 0)
    w0 = lin.weight.detach().clone()
    lin(torch.ones(1, 3)).sum().backward()
    (lin(torch.ones(1, 3)).sum() * float("nan")).backward()
    norm, applied = guard.eager_step(lin.parameters(), opt, 0.0, 0, 1)
    assert not applied and not np.isfinite(float(norm)) and torch.equal(lin.weight, w0) and (guard.skipped, guard.consecutive) == (1, 1)
    opt.zero_grad()
    lin(torch.ones(1, 3)).sum().backward()
    norm, applied = guard.eager_step(lin.parameters(), opt, 0.5, 0, 2)  # a finite threshold clips as before
    assert applied and np.isfinite(float(norm)) and not torch.equal(lin.weight, w0) and (guard.skipped, guard.consecutive) == (1, 0)
    assert float(torch.sqrt(sum((p_.grad ** 2).sum() for p_ in lin.parameters()))) <= 0.5 + 1e-6


def test_abort_after_n_consecutive_skips(tmp_path, cpu_batches):
    """Every frame of the training split is NaN: the run stops with a RuntimeError that names the count and the step, and nothing was
    written over."""
    from cfdbench_amd.harness.common import SkipGuard
    from cfdbench_amd.harness.train_auto import train
    ds = _data(False)
    for f in ds.all_features:
        f[:, 0, 3, 3] = np.nan
    model = _model()
    with pytest.raises(RuntimeError, match=r"3 optimiser steps in a row.*epoch 0, step 2"):
        train(model, ds, _data(False), tmp_path / "run", num_epochs=2, batch_size=1, eval_interval=1, plot_interval=0, skip_nonfinite=True,
              max_consecutive_skips=3)
    assert _finite(model) and not (tmp_path / "run" / "train_state.pt").exists()
    # the fused path hands the device counters to the same rule at its log interval; 0 = never abort
    g = SkipGuard(True, 5)
    g.check(4, 0, 9, skipped=7)
    with pytest.raises(RuntimeError, match=r"5 optimiser steps in a row.*epoch 1, step 3; 12 skipped in all"):
        g.check(5, 1, 3, skipped=12)
    SkipGuard(True, 0).check(10 ** 6, 0, 0)
    SkipGuard(False, 5).check(10, 0, 0)
