"""MI355X: the Sobolev objective -- the C-ABI rows of tests/test_emul_sobolev.py on the device (tests/sobolev_checks.py), the
reference-pinned fixture through the kernels, FnoTrainEngine(objective="hs") against the fp64 chain oracle.fno_forward -> the fp64 Sobolev
gradient -> oracle.fno_backward -> oracle.adam_step, a rollout window, the eager path (functional.sobolev_loss, loss.SobolevLoss through
Fno2d) and train_auto --objective hs."""
from pathlib import Path

import numpy as np
import pytest

from tests import objective_checks as OC
from tests import sobolev_checks as SC

pytestmark = pytest.mark.gpu
ROW = SC.register_alignment_row()  # (while pytest collects: tests/align_checks.py's table has the new entries' row before any test runs)
REPO = Path(__file__).resolve().parent.parent
f64 = np.float64


@pytest.fixture(scope="module")
def be():
    from tests.backends import TorchBackend
    return TorchBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(SC.SETTINGS))
@pytest.mark.parametrize("shape", SC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_sums_and_gradient_within_the_bound(be, shape, setting):
    SC.check_parity(be, shape, setting)


@pytest.mark.parametrize("setting", list(SC.SETTINGS))
def test_two_calls_on_dirty_buffers_give_the_same_bits(be, setting):
    assert SC.check_twice(be, (3, 2, 5, 7), setting) == 0
    assert SC.check_twice(be, (2, 2, 17, 36), setting) == 0
    assert SC.check_twice(be, (1, 2, 128, 128), setting) == 0


def test_misplaced_buffers_give_the_aligned_bits(be):
    assert SC.check_misplaced(be) == 0
    assert SC.check_misplaced(be, (1, 2, 64, 64)) == 0


@pytest.mark.parametrize("placement", ["all0", "all4", "all8", "each4"])
def test_row_of_the_alignment_table(be, placement):
    from tests import align_checks as A
    assert placement in A.placements(ROW, False)
    A.run_row(be, ROW, placement)


def test_an_exactly_predicted_sample_has_gradient_zero(be):
    SC.check_exact_sample(be)


def test_an_all_zero_label_sample(be):
    SC.check_zero_label(be)


def test_refusals_leave_every_buffer_untouched(be):
    res = SC.check_refusals(be)
    assert res and res == SC.expected_refusals(res), res


def test_a1_zero_is_the_rel_l2_kernels_value(be):
    fig, bound = SC.check_parseval(be)
    assert fig <= bound <= SC.CEILING, (fig, bound)


def test_the_benchmark_batch(be):
    """B = 256, two channels, 64 x 64: k_hs_final walks one sample per thread over the whole workgroup."""
    shape = (256, 2, 64, 64)
    figs = SC.errors(SC.run(be, shape, "k2", with_gadd=True, updev=0.5), shape, True)
    SC.assert_within(figs, "B = 256")


@pytest.mark.parametrize("setting", list(SC.SETTINGS))
@pytest.mark.parametrize("grid", ((5, 7), (6, 9)), ids=lambda g: f"{g[0]}x{g[1]}")
def test_kernels_against_the_reference_golden(be, grid, setting):
    """tests/golden/hsloss.npz: HsLoss of the reference and its autograd gradient, in fp64, at the bound of the module's emulation."""
    g = np.load(REPO / "tests" / "golden" / "hsloss.npz")
    H, W = grid
    p, lab, m = (g[f"g{H}x{W}_{n}"] for n in ("preds", "label", "mask"))
    shape = p.shape
    res = SC.run(be, shape, setting, data=(p, lab, m[:, 0], np.zeros(shape, np.float32)))
    value, want = float(g[f"g{H}x{W}_{setting}_value"]), g[f"g{H}x{W}_{setting}_grad"]
    assert SC.rel_err(res["ref"]["value"], value) <= 1e-12 and np.max(np.abs(res["ref"]["grad"] - want)) <= 1e-12 * np.max(np.abs(want))
    SC.assert_within(SC.errors(res, shape, False), ("golden", grid, setting))


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _flat0(eng):
    return OC.engine_tensors(eng, eng.flat.data)


@pytest.mark.parametrize("setting", list(SC.SETTINGS))
@pytest.mark.parametrize("name", ["pair", "chan", "padded"])
def test_train_step_against_the_oracle_chain(name, setting):
    """One train_step: the call sequence of an objective pass with the Sobolev pair in it; gradients, moments and the parameter delta
    against the fp64 chain at the bound of the route's own fused-step check; objective_value() and the still reported nmse.

    The hardest tensor is fc2.bias at [pair-k2]: the sum of the masked gradient on the predictions over all pixels, a cancellation of
    three orders at k = 2 with a = (0.5, 0.25).  With one fp32 accumulator chain per transform element it measured 1.73e-11 against
    the route's 1e-11; with the kernels' segments of eight terms added in fp64 it measures 4.5e-12 (fp32 rounding of the exact gradient
    alone: 8e-13)."""
    import torch
    params, batch, s = OC.model_case(name)
    eng = SC.make_engine(params, s, setting)
    assert eng.defer_flags == 0
    flat0 = _flat0(eng)
    tb = OC.to_dev(batch)
    sums = eng.train_step(*OC.step_args(tb))
    torch.cuda.synchronize()
    assert eng.api.names == (["cfd_fno_forward", "cfd_sobolev_fwd", "cfd_sobolev_bwd"] + ["cfd_fno_backward_phase_f"] * (s["L"] + 2)
                             + ["cfd_adam_flat"]), eng.api.names
    ref = SC.ref_pass(params, batch, s, setting)
    OC.assert_step(OC.compare_step(eng, flat0, ref["grads"]), name, setting)
    value = float(eng.objective_value())
    assert eng.objective_value().dim() == 0 and abs(value - ref["value"]) <= OC.VALUE_TOL * ref["value"], (value, ref["value"])
    lab = (batch["label"] * batch["mask"]).astype(f64)
    nmse = float(np.sum((ref["preds"] - lab) ** 2) / np.sum(lab ** 2))
    rows = sums.cpu().numpy().astype(f64)
    assert abs(rows[0] / rows[2] - nmse) <= OC.VALUE_TOL * nmse and abs(eng.scores()["nmse"] - nmse) <= OC.VALUE_TOL * nmse


def test_full_gradient_window_of_two():
    """K = 2 through the fed-back frame: step 1's gpreds_ext is its objective's gradient (1 / K in `upstream`) plus step 2's d_inputs
    (gadd)."""
    import torch

    from tests import ingrad_checks as IC
    params, batch, s = OC.model_case("pair")
    labels = IC.unroll_labels(47, batch, 2)
    eng = SC.make_engine(params, s, "k2")
    flat0 = _flat0(eng)
    tb = OC.to_dev(batch)
    sums = eng.train_window(tb["inputs"], [torch.from_numpy(a).cuda() for a in labels], tb["case_params"], tb["mask"], detach=False)
    torch.cuda.synchronize()
    names = eng.api.names
    assert not {"cfd_loss_coef", "cfd_fno_forward_train_f", "cfd_objective_fwd", "cfd_objective_bwd"} & set(names)
    assert names.count("cfd_fno_forward") == 2 and names.count("cfd_sobolev_fwd") == names.count("cfd_sobolev_bwd") == 2
    ref = SC.ref_window(params, batch, s, "k2", labels)
    OC.assert_step(OC.compare_step(eng, flat0, ref["grads"]), "pair", "window hs")
    vals = eng.objective_value().cpu().numpy()
    assert vals.shape == (2,) and tuple(sums.shape) == (2, 4)
    assert all(abs(float(v) - w) <= OC.VALUE_TOL * w for v, w in zip(vals, ref["values"])), (vals, ref["values"])


def test_engine_refusals():
    params, _batch, s = OC.model_case("padded")
    from cfdbench_amd.engine import FnoTrainEngine
    for kw, match in ((dict(objective="hs", act_dtype="bf16"), "bf16"), (dict(objective="hs", hs_k=3), "k = 3"), (dict(objective="rel_l2", hs_group=True), "hs_k"),
                      (dict(objective="hs", loss_name="mse"), "loss_name")):
        with pytest.raises(ValueError, match=match):
            FnoTrainEngine(SC.make_model(params, s), **kw)


# ---- the eager path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", list(SC.SETTINGS))
def test_model_loss_backward_is_the_engines_gradient(setting):
    """model(**batch)["loss"]["hs"].backward(): Fno2d's parameter gradients through the autograd node against the engine's gradients()
    (the same kernels on the same predictions) and against the fp64 chain."""
    import torch

    from oracle import fno_oracle as O
    params, batch, s = OC.model_case("pair")
    model = SC.make_model(params, s, setting)
    out = model(**OC.to_dev(batch))
    assert list(out["loss"]) == ["mse", "rmse", "mae", "nmse", "hs"]
    out["loss"]["hs"].backward()
    eng = SC.make_engine(params, s, setting)
    eng.train_step(*OC.step_args(OC.to_dev(batch)))
    torch.cuda.synchronize()
    ref = SC.ref_pass(params, batch, s, setting)
    assert abs(float(out["loss"]["hs"].detach()) - ref["value"]) <= OC.VALUE_TOL * ref["value"]
    assert abs(float(out["loss"]["hs"].detach()) - float(eng.objective_value())) <= OC.VALUE_TOL * ref["value"]
    mine = {q: p_.grad.cpu().numpy() for q, p_ in model.named_parameters()}
    from tests import fno_checks as F
    theirs = OC.engine_tensors(eng, eng.gradients())
    vs = {q: O.rel_nmse(F.flat_view(mine[q]).astype(f64), theirs[q].astype(f64)) for q in theirs}
    print("sobolev eager against the engine", setting, max(vs.values()))
    assert all(v <= OC.grad_tol("pair") for v in vs.values()), vs
    res = {q: O.rel_nmse(v, ref["grads"][q]) for q, v in mine.items()}
    print("sobolev eager against fp64", setting, max(res.values()))
    assert all(v <= OC.grad_tol("pair") for v in res.values()), res


def test_sobolev_loss_on_views():
    """What tests/test_gpu_views.py asks of every autograd node of functional.py, for the node of cfdbench_amd/sobolev.py: offset views,
    batch slices and non-contiguous tensors give the value and the gradient of the plain tensors, bit for bit."""
    import torch

    from cfdbench_amd.functional import sobolev_loss
    from cfdbench_amd.sobolev import SobolevLossFn
    from tests.test_gpu_views import batch_slice, non_contiguous, offset_view
    preds, label, mask, _g = SC.case(3, 2, 32, 36, seed=8)
    plain = [torch.from_numpy(a).cuda() for a in (preds, label, mask[:, None])]

    def run(p, lab, m):
        p = p.detach().requires_grad_(True)
        value = sobolev_loss(p, lab, m, k=2, a=(0.5, 0.25))
        assert type(value.grad_fn).__name__ == SobolevLossFn.__name__ + "Backward"
        (value * 0.5).backward()
        return value.detach().clone().view(torch.int32), p.grad.contiguous().view(torch.int32)

    want = run(*plain)
    for how in (offset_view, batch_slice, non_contiguous):
        got = run(*[how(torch, t) for t in plain])
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), how.__name__
    ref = SC.reference(preds, label, mask, 2, (0.5, 0.25), False, upstream=0.5)
    emu = SC.emulate(preds, label, mask, 2, (0.5, 0.25), False, upstream=0.5)
    got = want[1].view(torch.float32).cpu().numpy().astype(f64)
    top = np.abs(ref["grad"]).max()
    assert np.max(np.abs(got - ref["grad"])) / top <= 2.0 * np.max(np.abs(emu["grad"] - ref["grad"])) / top + SC.FLOOR["grad_img"] <= SC.CEILING


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def _toy_model():
    params, _b, s = OC.model_case("padded")
    return OC.make_model(params, dict(s, pad=0))


def _data():
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    return (SyntheticAutoDataset(n_cases=4, n_frames=5, height=32, width=32, seed=0),
            SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1))


KW = dict(batch_size=4, eval_batch_size=4, log_interval=2, eval_interval=1, plot_interval=0, lr=5e-3)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "eager"])
def test_train_auto_hs_trains_and_writes_the_objective(tmp_path, fused):
    """train_auto --objective hs --hs_k 2 on SyntheticAutoDataset, both paths: train_objective.json carries the value, which falls."""
    import json

    import torch

    from cfdbench_amd.harness.train_auto import train
    tr, dev = _data()
    torch.manual_seed(3)
    train(_toy_model(), tr, dev, tmp_path / "run", num_epochs=3, fused=fused, objective="hs", hs_k=2, **KW)
    hist = json.loads((tmp_path / "run" / "train_objective.json").read_text())["hs"]
    nmse = json.loads((tmp_path / "run" / "train_losses.json").read_text())
    assert len(hist) == len(nmse) > 0 and np.isfinite(hist).all() and np.mean(hist[-4:]) < np.mean(hist[:4])
    dev_scores = json.loads((tmp_path / "run" / "ckpt-2" / "dev_scores.json").read_text())
    assert "hs" in dev_scores["mean"] and (tmp_path / "run" / "ckpt-2" / "train_objective.json").exists()
