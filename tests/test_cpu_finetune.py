"""CPU: host logic of fine-tuning on the fused FNO engine -- the last backward phase of a trainable subset, the compact flat layout, which
deferral flags a subset keeps, --freeze / --train_only / --optimizer / --init_from and what is refused with them, the new flag bit in the
header and the binding, and the fp64 restatement of the AdamW rule against torch.optim.AdamW.  The kernel and whole steps:
tests/test_emul_finetune.py, tests/test_gpu_finetune.py."""
import itertools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from cfdbench_amd.engine import flatten_layout, last_backward_phase, mask_defer_flags, match_prefixes, param_phase
from tests import finetune_checks as FT
from tests import fno_checks as F

REPO = Path(__file__).resolve().parent.parent


def _mask(L, groups):
    """One flag per tensor for a set of groups: "fc0", block numbers, "head"."""
    return [("fc0" in groups)] * 2 + [l in groups for l in range(L) for _ in range(4)] + [("head" in groups)] * 4


@pytest.mark.parametrize("L", [0, 1, 3])
def test_last_phase_of_every_subset(L):
    """head -> 0, FnoBlock l -> L - l, fc0 -> L + 1; a subset stops behind its shallowest member; nothing trainable is refused."""
    groups = ["fc0", *range(L), "head"]
    phase = {"fc0": L + 1, "head": 0, **{l: L - l for l in range(L)}}
    seen = 0
    for r in range(1, len(groups) + 1):
        for sub in itertools.combinations(groups, r):
            assert last_backward_phase(_mask(L, sub), L) == max(phase[g] for g in sub), sub
            seen += 1
    assert seen == 2 ** len(groups) - 1
    # a single tensor of a group is enough to need the group's phase
    for i in range(6 + 4 * L):
        one = [j == i for j in range(6 + 4 * L)]
        assert last_backward_phase(one, L) == param_phase(i, L)
    assert [param_phase(i, L) for i in (0, 1)] == [L + 1] * 2 and [param_phase(2 + 4 * L + j, L) for j in range(4)] == [0] * 4
    assert last_backward_phase([True] * (6 + 4 * L), L) == L + 1
    with pytest.raises(ValueError, match="nothing is trainable"):
        last_backward_phase([False] * (6 + 4 * L), L)
    with pytest.raises(ValueError):
        last_backward_phase([True] * 5, L)


def test_compact_layout_offsets():
    """Trainable tensors in ABI order on 4-float boundaries, complex ones as pairs; a frozen tensor takes no room and carries the offset
    of the next trainable one, so the phase slices of the all-trainable layout rule hold on the compact buffer."""
    from cfdbench_amd.engine import backward_phase_slices
    L, C = 2, 3
    shapes = [(C, 7, 1, 1), (C,)] + [s for _ in range(L) for s in ((C, C, 2, 2), (C, C, 2, 2), (C, C, 1, 1), (C,))] + [(5, C, 1, 1), (5,), (2, 5, 1, 1), (2,)]
    cplx = [False, False] + [True, True, False, False] * L + [False] * 4
    ts = [torch.zeros(s, dtype=torch.complex64 if c else torch.float32) for s, c in zip(shapes, cplx)]
    size = [t.numel() * (2 if t.is_complex() else 1) for t in ts]
    pad4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    # all trainable: the layout of before
    offs, numel = flatten_layout(ts)
    assert offs == [sum(pad4(n) for n in size[:i]) for i in range(len(ts))] and numel == sum(pad4(n) for n in size)
    assert flatten_layout(ts, trainable=[True] * len(ts)) == (offs, numel)
    # last block + head
    mask = _mask(L, {1, "head"})
    offs, numel = flatten_layout(ts, trainable=mask)
    want, off = [], 0
    for n, t in zip(size, mask):
        want.append(off)
        off += pad4(n) if t else 0
    assert offs == want and numel == off == sum(pad4(n) for n, t in zip(size, mask) if t)
    assert offs[:6] == [0] * 6 and offs[6] == 0 and offs[7] == pad4(size[6])
    sl = backward_phase_slices(offs, numel, L)
    assert sl[0] == (offs[10], numel) and sl[1] == (0, offs[10]) and sl[2] == (0, 0) and sl[3] == (0, 0)
    # the checks' own layout (tests/finetune_checks.py) is the same rule
    names = F.param_names(L)
    params = {k: np.zeros(s, np.complex64 if c else np.float32) for k, s, c in zip(names, shapes, cplx)}
    layout, total, _ = FT.compact_layout(params, names, mask)
    assert total == numel and {k: v[0] for k, v in layout.items()} == {k: o for k, o, t in zip(names, offs, mask) if t}


def test_flag_masking_table():
    """STEM (4) goes with a frozen fc0, HEAD (2) when phase 1 does not run, SCALE (1) stays; flags that are not set stay unset."""
    table = {  # (fc0 trainable, last phase) -> what is left of 7
        (True, 3): 7, (True, 1): 7, (False, 2): 3, (False, 1): 3, (False, 0): 1, (True, 0): 5}
    for (fc0, last), want in table.items():
        assert mask_defer_flags(7, fc0, last) == want, (fc0, last)
        assert mask_defer_flags(0, fc0, last) == 0
        assert mask_defer_flags(1, fc0, last) == 1
    L = 2
    for sub, want in ((("head",), 1), ((1, "head"), 3), (("fc0", "head"), 7), ((0, 1), 3), (("fc0", 0, 1, "head"), 7)):
        m = _mask(L, set(sub))
        assert mask_defer_flags(7, m[0], last_backward_phase(m, L)) == want, sub


def test_prefix_matching():
    names = F.param_names(11)
    hit = match_prefixes(names, ["blocks.1", "fc2."])
    assert [k for k, h in zip(names, hit) if h] == [f"blocks.1.{t}" for t in ("conv0.weights1", "conv0.weights2", "w0.weight", "w0.bias")] + ["fc2.weight", "fc2.bias"]
    assert sum(match_prefixes(names, ["blocks"])) == 44 and sum(match_prefixes(names, ["fc0.weight"])) == 1
    for bad in (["fc3"], ["fc1", "block"], [""], ["fc"]):
        with pytest.raises(ValueError, match="matches no parameter"):
            match_prefixes(names, bad)


def test_flag_bit_agrees_between_header_and_binding():
    from cfdbench_amd import _capi
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    assert int(re.search(r"#define CFD_STEP_DECOUPLED_WD (\d+)", header).group(1)) == 32 == _capi.CFD_STEP_DECOUPLED_WD
    bits = [int(re.search(rf"#define {n} (\d+)", header).group(1)) for n in
            ("CFD_TRAIN_DEFER_SCALE", "CFD_TRAIN_DEFER_HEAD", "CFD_TRAIN_DEFER_STEM", "CFD_STEP_ACCUMULATE", "CFD_STEP_ACCUM_INIT", "CFD_STEP_DECOUPLED_WD")]
    assert bits == [1, 2, 4, 8, 16, 32]
    # the feature rides on what exists: no new version, no new entry point, no new argument
    assert _capi.ABI_VERSION == 604 == int(re.search(r"#define CFD_ABI_VERSION (\d+)", header).group(1))
    assert len(_capi._SIGS["cfd_fno_adam_step"][1]) == 25
    assert "ignored" in header[header.index("CFD_STEP_DECOUPLED_WD"):][:1500].lower()  # (the header says what CFD_STEP_ACCUMULATE does to it)


def test_arguments_and_refusals():
    from cfdbench_amd.harness.args import Args, is_args_valid
    base = ["--model", "fno", "--data", "cavity_bc"]
    args = Args().parse_args(base)
    assert (args.freeze, args.train_only, args.optimizer, args.init_from) == ("", "", "adam", "")
    is_args_valid(args)
    args = Args().parse_args(base + ["--fused", "1", "--train_only", "fc1,fc2", "--optimizer", "adamw", "--init_from", "x/model.pt", "--weight_decay", "0.01"])
    is_args_valid(args)
    assert args.as_dict()["train_only"] == "fc1,fc2" and args.optimizer == "adamw" and args.init_from == "x/model.pt"
    is_args_valid(Args(model="unet", data_name="cavity_bc", freeze="down", optimizer="adamw"))  # any model, any eager path
    with pytest.raises(AssertionError, match="mutually exclusive"):
        is_args_valid(Args(model="fno", data_name="cavity_bc", freeze="fc0", train_only="fc1"))
    with pytest.raises(AssertionError, match="cfd_adam_multi"):
        is_args_valid(Args(model="unet", data_name="cavity_bc", graph=1, optimizer="adamw"))
    with pytest.raises(AssertionError, match="--optimizer"):
        is_args_valid(Args(model="fno", data_name="cavity_bc", optimizer="sgd"))
    is_args_valid(Args(model="unet", data_name="cavity_bc", graph=1, optimizer="adam"))


def test_apply_trainable_and_optimizer():
    from cfdbench_amd.harness.common import apply_trainable, make_optimizer, split_prefixes
    net = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    assert split_prefixes(" 0 , 1.bias,") == ["0", "1.bias"] and split_prefixes("") == []
    assert apply_trainable(net) == ["0.weight", "0.bias", "1.weight", "1.bias"]
    assert apply_trainable(net, freeze="0") == ["1.weight", "1.bias"] and not net[0].weight.requires_grad
    assert apply_trainable(net, train_only="0.bias,1.weight") == ["0.bias", "1.weight"] and not net[1].bias.requires_grad
    with pytest.raises(ValueError, match="matches no parameter"):
        apply_trainable(net, freeze="2")
    with pytest.raises(ValueError, match="mutually exclusive"):
        apply_trainable(net, freeze="0", train_only="1")
    with pytest.raises(ValueError, match="nothing trainable"):
        apply_trainable(net, freeze="0,1")
    adam = make_optimizer(net.parameters(), "adam", 1e-3, 0.5)
    assert type(adam) is torch.optim.Adam and adam.defaults["weight_decay"] == 0  # (weight_decay stays unused, as in the reference)
    adamw = make_optimizer(net.parameters(), "adamw", 1e-3, 0.5)
    assert type(adamw) is torch.optim.AdamW and adamw.defaults["weight_decay"] == 0.5
    with pytest.raises(ValueError):
        make_optimizer(net.parameters(), "sgd", 1e-3)


def test_main_applies_the_flags_before_train(monkeypatch, tmp_path):
    """main() freezes through requires_grad_ before train() builds anything, and hands --optimizer / --weight_decay / --init_from on."""
    from cfdbench_amd.harness import data as D
    from cfdbench_amd.harness import train_auto as T
    seen = []
    ds = D.SyntheticAutoDataset(n_cases=1, n_frames=3, height=8, width=8, seed=0)
    monkeypatch.setattr(D, "get_auto_dataset", lambda **kw: (ds, ds, ds))
    monkeypatch.setattr(T, "init_distributed", lambda: (0, 1))
    monkeypatch.setattr(T, "train", lambda model, **kw: seen.append(
        ([k for k, p in model.named_parameters() if p.requires_grad], kw["optimizer_kind"], kw["weight_decay"], kw["init_from"])))
    monkeypatch.setattr(torch.nn.Module, "cuda", lambda self, *a, **k: self)
    common = ["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--mode", "train", "--fno_hidden_dim", "4", "--fno_depth", "1",
              "--output_dir", str(tmp_path)]
    T.main(common + ["--train_only", "fc1,fc2", "--optimizer", "adamw", "--weight_decay", "0.25", "--init_from", "a/model.pt"])
    T.main(common + ["--freeze", "blocks"])
    T.main(common)
    head = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert seen[0] == (head, "adamw", 0.25, "a/model.pt")
    assert seen[1] == (["fc0.weight", "fc0.bias"] + head, "adam", 1e-5, "")
    assert len(seen[2][0]) == 10 and seen[2][1:] == ("adam", 1e-5, "")
    with pytest.raises(ValueError, match="matches no parameter"):
        T.main(common + ["--freeze", "decoder"])


def test_init_from_is_ignored_by_a_resume_that_finds_its_state(tmp_path, monkeypatch, capsys):
    """train(): --init_from loads through load_ckpt before anything is built; with resume and a train_state.pt it is skipped, with a log line."""
    from cfdbench_amd.harness import train_auto as T
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    loaded = []
    monkeypatch.setattr(T, "load_ckpt", lambda model, path: loaded.append(Path(path)))

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()
    monkeypatch.setattr(T, "make_optimizer", stop)  # (the next thing train() does: nothing is trained here)
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)
    model = Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4)
    run = tmp_path / "run"
    with pytest.raises(Stop):
        T.train(model, ds, ds, run, num_epochs=1, plot_interval=0, init_from=str(tmp_path / "w.pt"))
    with pytest.raises(Stop):
        T.train(model, ds, ds, run, num_epochs=1, plot_interval=0, init_from=str(tmp_path / "w.pt"), resume=True)  # no state yet: loads
    assert loaded == [tmp_path / "w.pt"] * 2
    (run / "train_state.pt").write_bytes(b"")
    with pytest.raises(Stop):
        T.train(model, ds, ds, run, num_epochs=1, plot_interval=0, init_from=str(tmp_path / "w.pt"), resume=True)
    assert len(loaded) == 2 and "--init_from" in capsys.readouterr().out
    with pytest.raises(NotImplementedError, match="adamw"):
        T.train(model, ds, ds, run, num_epochs=1, plot_interval=0, optimizer_kind="adamw", graph=True)


def test_rule_against_torch_adamw():
    """The restatement the kernel is held to, against torch.optim.AdamW (single-tensor path) in fp64 on the CPU: three steps, to rounding."""
    n = 1027
    p0, gs = FT.flat_case(n)
    p = torch.nn.Parameter(torch.tensor(p0, dtype=torch.float64))
    opt = torch.optim.AdamW([p], lr=FT.LR, betas=(FT.B1, FT.B2), eps=FT.EPS, weight_decay=FT.WD, foreach=False)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step, g in enumerate(gs, 1):
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        FT.adamw_rule(p64, g.astype(np.float64), m64, v64, step, round_factor=False)
        st = opt.state[p]
        np.testing.assert_allclose(m64, st["exp_avg"].numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(v64, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)
        np.testing.assert_allclose(p64, p.detach().numpy(), rtol=1e-12, atol=1e-18)
    # the fp32 rounding of the factor (what a float32 parameter's mul_ sees) moves a parameter by at most half an ulp of the factor
    q64 = p0.astype(np.float64)
    FT.adamw_rule(q64, gs[0].astype(np.float64), np.zeros(n), np.zeros(n), 1, round_factor=True)
    r64 = p0.astype(np.float64)
    FT.adamw_rule(r64, gs[0].astype(np.float64), np.zeros(n), np.zeros(n), 1, round_factor=False)
    assert np.max(np.abs(q64 - r64)) <= 2.0 ** -24 * np.max(np.abs(p0))
    # and the coupled form is another rule: the oracle's Adam with weight_decay differs from it by far more than the checks' bound
    from oracle import fno_oracle as O
    c64, cm, cv = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for step, g in enumerate(gs, 1):
        O.adam_step(c64, g.astype(np.float64), cm, cv, step, FT.LR, FT.B1, FT.B2, FT.EPS, FT.WD)
    assert O.rel_nmse(c64 - p0, p64 - p0) > 1e3 * FT.ADAM_TOL
