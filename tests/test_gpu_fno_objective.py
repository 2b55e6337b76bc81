"""MI355X: the training objectives -- the C-ABI rows of tests/test_emul_fno_objective.py on the device (tests/objective_checks.py), the
reference-pinned fixture through the kernels, FnoTrainEngine(objective=) on every route against the fp64 chain oracle.fno_forward -> the
fp64 objective gradient -> oracle.fno_backward -> oracle.adam_step, the eager path (functional.objective_loss, loss.ObjectiveLoss through
Fno2d) and train_auto --objective."""
from pathlib import Path

import numpy as np
import pytest

from tests import objective_checks as OC

pytestmark = pytest.mark.gpu
ROW = OC.register_alignment_row()  # (while pytest collects: tests/align_checks.py's table has the new entries' row before any test runs)
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
@pytest.mark.parametrize("kind", OC.KINDS)
@pytest.mark.parametrize("shape", OC.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_value_and_gradient_within_the_derived_bound(be, shape, kind):
    OC.check_parity(be, shape, kind)


@pytest.mark.parametrize("kind", OC.KINDS)
def test_two_calls_on_dirty_buffers_give_the_same_bits(be, kind):
    assert OC.check_twice(be, (3, 3, 4290), kind) == 0
    assert OC.check_twice(be, (2, 2, 16384), kind) == 0


def test_misplaced_buffers_give_the_aligned_bits(be):
    assert OC.check_misplaced(be) == 0


@pytest.mark.parametrize("placement", ["all0", "all4", "all8", "each4"])
def test_row_of_the_alignment_table(be, placement):
    from tests import align_checks as A
    assert placement in A.placements(ROW, False)
    A.run_row(be, ROW, placement)


def test_an_exactly_predicted_sample_has_gradient_zero(be):
    OC.check_exact_sample(be)


def test_an_all_zero_label_slice(be):
    OC.check_zero_label(be)


def test_refusals_leave_every_buffer_untouched(be):
    res = OC.check_refusals(be)
    assert res and all(v == (-1, True) for v in res.values()), res


def test_nmse_channel_at_the_benchmark_batch(be):
    """B = 256, two channels, 64 x 64: k_obj_final adds 256 records per channel through the whole workgroup."""
    figs = OC.errors(OC.run(be, (256, 2, 4096), "nmse_channel", with_gadd=True, updev=0.5), (256, 2, 4096), True)
    OC.assert_within(figs, True, "B = 256")


def test_kernels_against_the_reference_golden(be):
    """tests/golden/lploss_rel.npz: LpLoss().rel of the reference and its autograd gradient, in fp64."""
    g = np.load(REPO / "tests" / "golden" / "lploss_rel.npz")
    B, Co, H, W = (int(v) for v in g["meta"][:4])
    shape = (B, Co, H * W)
    data = (g["preds"].reshape(shape), g["label"].reshape(shape), g["mask"].reshape(B, H * W), np.zeros(shape, np.float32))
    res = OC.run(be, shape, "rel_l2", data=data)
    want = g["grad"].reshape(shape)
    assert abs(float(res["value"][0]) - float(g["value"])) <= OC.UNITS["value"] * OC.SLACK * OC.U * float(g["value"])
    err = np.abs(res["gpreds"].astype(f64) - want)
    assert (err <= OC.UNITS["grad"] * OC.SLACK * OC.U * np.abs(want)).all() and np.any(want != 0.0)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _flat0(eng):
    return OC.engine_tensors(eng, eng.flat.data)


@pytest.mark.parametrize("kind", OC.KINDS)
@pytest.mark.parametrize("name", list(OC.MODEL_CASES))
def test_train_step_against_the_oracle_chain(name, kind):
    """One train_step: the call sequence of the issue; gradients, moments and the parameter delta against the fp64 chain at the bound of
    the route's own fused-step check; objective_value() and the still reported nmse against the fp64 model's."""
    import torch
    params, batch, s = OC.model_case(name)
    eng = OC.make_engine(params, s, objective=kind)
    assert eng.defer_flags == 0
    flat0 = _flat0(eng)
    tb = OC.to_dev(batch)
    sums = eng.train_step(*OC.step_args(tb))
    torch.cuda.synchronize()
    assert eng.api.names == (["cfd_fno_forward", "cfd_objective_fwd", "cfd_objective_bwd"] + ["cfd_fno_backward_phase_f"] * (s["L"] + 2)
                             + ["cfd_adam_flat"]), eng.api.names
    ref = OC.ref_pass(params, batch, s, kind)
    OC.assert_step(OC.compare_step(eng, flat0, ref["grads"]), name, kind)
    value = float(eng.objective_value())
    assert eng.objective_value().dim() == 0 and abs(value - ref["value"]) <= OC.VALUE_TOL * ref["value"], (value, ref["value"])
    lab = (batch["label"] * batch["mask"]).astype(f64)
    nmse = float(np.sum((ref["preds"] - lab) ** 2) / np.sum(lab ** 2))
    rows = sums.cpu().numpy().astype(f64)
    assert abs(rows[0] / rows[2] - nmse) <= OC.VALUE_TOL * nmse and abs(eng.scores()["nmse"] - nmse) <= OC.VALUE_TOL * nmse


def test_accumulation_over_two_micro_batches():
    import torch
    params, batch, s = OC.model_case("pair")
    _p, batch2, _s = OC.model_case("pair", bseed=52)
    eng = OC.make_engine(params, s, objective="rel_l2")
    flat0 = _flat0(eng)
    for k, b in enumerate((batch, batch2)):
        eng.accumulate(*OC.step_args(OC.to_dev(b)), weight=0.5, first=k == 0)
    eng.apply_accumulated()
    torch.cuda.synchronize()
    refs = [OC.ref_pass(params, b, s, "rel_l2") for b in (batch, batch2)]
    mean = {q: 0.5 * (refs[0]["grads"][q] + refs[1]["grads"][q]) for q in refs[0]["grads"]}
    OC.assert_step(OC.compare_step(eng, flat0, mean), "pair", "accumulate")
    assert eng.step_count == 1 and eng.api.names.count("cfd_objective_bwd") == 2 and eng.api.names.count("cfd_fno_adam_step") == 3
    assert abs(float(eng.objective_value()) - refs[1]["value"]) <= OC.VALUE_TOL * refs[1]["value"]


@pytest.mark.parametrize("kind", ["rel_l2", "nmse_channel"])
def test_full_gradient_window_of_two(kind):
    """K = 2 through the fed-back frame: step 1's gpreds_ext is its objective's gradient (1 / K in `upstream`) plus step 2's d_inputs
    (gadd); no cfd_loss_coef, no one-pass head, no label in the phases."""
    import torch

    from tests import ingrad_checks as IC
    params, batch, s = OC.model_case("pair")
    labels = IC.unroll_labels(47, batch, 2)
    eng = OC.make_engine(params, s, objective=kind)
    flat0 = _flat0(eng)
    tb = OC.to_dev(batch)
    sums = eng.train_window(tb["inputs"], [torch.from_numpy(a).cuda() for a in labels], tb["case_params"], tb["mask"], detach=False)
    torch.cuda.synchronize()
    names = eng.api.names
    assert not {"cfd_loss_coef", "cfd_fno_forward_train_f", "cfd_label_energy_coef"} & set(names)
    assert names.count("cfd_fno_forward") == 2 and names.count("cfd_objective_fwd") == names.count("cfd_objective_bwd") == 2
    ref = OC.ref_window(params, batch, s, kind, labels)
    OC.assert_step(OC.compare_step(eng, flat0, ref["grads"]), "pair", f"window {kind}")
    vals = eng.objective_value().cpu().numpy()
    assert vals.shape == (2,) and tuple(sums.shape) == (2, 4)
    assert all(abs(float(v) - w) <= OC.VALUE_TOL * w for v, w in zip(vals, ref["values"])), (vals, ref["values"])


def test_detached_window_is_two_plain_accumulates():
    import torch

    from tests import ingrad_checks as IC
    params, batch, s = OC.model_case("pair")
    labels = IC.unroll_labels(47, batch, 2)
    tb = OC.to_dev(batch)
    tl = [torch.from_numpy(a).cuda() for a in labels]
    eng = OC.make_engine(params, s, objective="nmse_sample")
    eng.train_window(tb["inputs"], tl, tb["case_params"], tb["mask"], detach=True)
    two = OC.make_engine(params, s, objective="nmse_sample")
    two.accumulate(tb["inputs"], tl[0], tb["case_params"], tb["mask"], weight=0.5, first=True)
    x2 = two.preds.clone()
    two.accumulate(x2, tl[1], tb["case_params"], tb["mask"], weight=0.5, first=False)
    two.apply_accumulated()
    torch.cuda.synchronize()
    assert torch.equal(eng.flat.data.view(torch.int32), two.flat.data.view(torch.int32))
    assert tuple(eng.objective_value().shape) == (2,) and float(eng.objective_value()[1]) == float(two.objective_value())


def test_clipping_takes_the_objectives_gradient():
    import torch

    from tests import clip_checks as CC
    params, batch, s = OC.model_case("pair")
    ref = OC.ref_pass(params, batch, s, "nmse_sample")
    norm = OC.ref_norm(ref["grads"], list(params))
    eng = OC.make_engine(params, s, objective="nmse_sample", max_grad_norm=0.5 * norm)
    flat0 = _flat0(eng)
    eng.train_step(*OC.step_args(OC.to_dev(batch)))
    torch.cuda.synchronize()
    coef = min(1.0, float(np.float32(0.5 * norm)) / (norm + 1e-6))
    assert abs(float(eng.grad_norm()) - norm) <= CC.CLIP_TOL * norm and abs(float(eng.clip_coef()) - coef) <= CC.CLIP_TOL
    OC.assert_step(OC.compare_step(eng, flat0, ref["grads"], coef=coef), "pair", "clipped")
    assert eng.api.names[-1] == "cfd_fno_adam_step"


def test_a_frozen_trunk_runs_the_head_phase_alone():
    import torch
    params, batch, s = OC.model_case("pair")
    eng = OC.make_engine(params, s, objective="nmse_channel", trainable={"fc1", "fc2"})
    assert eng.last_phase == 0
    flat0 = _flat0(eng)
    assert sorted(flat0) == ["fc1.bias", "fc1.weight", "fc2.bias", "fc2.weight"]
    eng.train_step(*OC.step_args(OC.to_dev(batch)))
    torch.cuda.synchronize()
    assert eng.api.names.count("cfd_fno_backward_phase_f") == 1
    OC.assert_step(OC.compare_step(eng, flat0, OC.ref_pass(params, batch, s, "nmse_channel")["grads"]), "pair", "head only")


def test_adamw_and_ema_ride_on_the_unchanged_optimiser_call():
    """AdamW with averaged weights: the optimiser call is cfd_fno_adam_step_ema with the objective's gradient -- bitwise the parameters of
    the same engine without EMA, and the average moved."""
    import torch
    params, batch, s = OC.model_case("padded")
    tb = OC.to_dev(batch)
    a = OC.make_engine(params, s, objective="rel_l2", optimizer="adamw", weight_decay=0.1, ema_decay=0.9)
    b = OC.make_engine(params, s, objective="rel_l2", optimizer="adamw", weight_decay=0.1)
    start = a.ema.clone()
    for eng in (a, b):
        for _ in range(2):
            eng.train_step(*OC.step_args(tb))
    torch.cuda.synchronize()
    assert a.api.names.count("cfd_fno_adam_step_ema") == 2 and b.api.names.count("cfd_fno_adam_step") == 2
    assert torch.equal(a.flat.data.view(torch.int32), b.flat.data.view(torch.int32)) and not torch.equal(a.ema, start)
    assert bool(torch.isfinite(a.ema).all()) and not torch.equal(a.ema, a.flat.data)


@pytest.mark.parametrize("kind", OC.KINDS)
def test_a_nan_label_is_skipped_on_the_device(kind):
    import torch
    params, batch, s = OC.model_case("padded")
    eng = OC.make_engine(params, s, objective=kind, skip_nonfinite=True)
    bad = {k: v.copy() for k, v in batch.items()}
    bad["label"][0, 0, s["H"] // 2, s["W"] // 2] = np.nan
    before = [t.clone().view(torch.int32) for t in (eng.flat.data, eng.exp_avg, eng.exp_avg_sq)]
    eng.train_step(*OC.step_args(OC.to_dev(bad)))
    torch.cuda.synchronize()
    after = [t.view(torch.int32) for t in (eng.flat.data, eng.exp_avg, eng.exp_avg_sq)]
    assert all(torch.equal(x, y) for x, y in zip(before, after)), "the skipped step moved a bit"
    assert float(eng.skipped_steps()) == 1.0 and bool(eng.last_step_skipped()) and not np.isfinite(float(eng.objective_value()))
    eng.train_step(*OC.step_args(OC.to_dev(batch)))
    torch.cuda.synchronize()
    assert float(eng.skipped_steps()) == 1.0 and not bool(eng.last_step_skipped()) and not torch.equal(before[0], eng.flat.data.view(torch.int32))


def test_graph_replay_equals_the_eager_step():
    import torch
    params, batch, s = OC.model_case("pair")
    _p, batch2, _s = OC.model_case("pair", bseed=52)
    eager, graph = OC.make_engine(params, s, objective="rel_l2"), OC.make_engine(params, s, objective="rel_l2")
    for b in (batch, batch2):
        tb = OC.to_dev(b)
        eager.train_step(*OC.step_args(tb))
        graph.train_step_graph(*OC.step_args(tb))
        torch.cuda.synchronize()
        assert torch.equal(eager.objective_value().view(torch.int32), graph.objective_value().view(torch.int32))
    for x, y in ((eager.flat.data, graph.flat.data), (eager.exp_avg, graph.exp_avg), (eager.exp_avg_sq, graph.exp_avg_sq)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert graph.api.names.count("cfd_objective_fwd") == 2  # (the warm-up pass and the captured one: replays make no C call)


def test_objective_none_is_the_engine_without_the_argument():
    import torch

    from cfdbench_amd.engine import FnoTrainEngine
    params, batch, s = OC.model_case("pair")
    tb = OC.to_dev(batch)
    with_arg = OC.make_engine(params, s, objective=None)
    without = FnoTrainEngine(OC.make_model(params, s), lr=OC.LR, loss_name="nmse")
    without.api = OC.Counting(without.api)
    for eng in (with_arg, without):
        for _ in range(2):
            eng.train_step(*OC.step_args(tb))
    torch.cuda.synchronize()
    assert with_arg.api.names == without.api.names and not any("objective" in n for n in with_arg.api.names)
    assert with_arg.defer_flags == without.defer_flags == 7
    for x, y in ((with_arg.flat.data, without.flat.data), (with_arg.exp_avg, without.exp_avg), (with_arg.exp_avg_sq, without.exp_avg_sq)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    with pytest.raises(RuntimeError, match="without objective"):
        with_arg.objective_value()


def test_engine_refusals():
    params, _batch, s = OC.model_case("padded")
    for kw, match in ((dict(objective="rel_l2", act_dtype="bf16"), "bf16"), (dict(objective="l2"), "objective must be")):
        with pytest.raises(ValueError, match=match):
            OC.make_engine(params, s, **kw)
    from cfdbench_amd.engine import FnoTrainEngine
    with pytest.raises(ValueError, match="loss_name"):
        FnoTrainEngine(OC.make_model(params, s), loss_name="mse", objective="rel_l2")


def _dp_worker(port, q):
    import os

    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_DP_ALWAYS_EXCHANGE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        params, batch, s = OC.model_case("padded")
        tb = OC.to_dev(batch)
        out = {}
        for overlap in (True, False):
            eng = OC.make_engine(params, s, objective="rel_l2", overlap=overlap)
            assert eng.sync.exchange and eng.defer_flags == 0
            for _ in range(2):
                eng.train_step(*OC.step_args(tb))
            torch.cuda.synchronize()
            out[overlap] = (list(eng.api.names), eng.flat.data.cpu().numpy(), float(eng.objective_value()))
        q.put(out)
    finally:
        dist.destroy_process_group()


def test_data_parallel_run_exchanges_once_behind_the_pass():
    """A one-rank gloo group with the exchange forced on: with and without `overlap` the pass is the objective's own (no per-phase
    exchange entry), and the parameters are bitwise those of the engine outside a group."""
    import socket

    import torch
    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_dp_worker, args=(port, q))
    proc.start()
    try:
        out = q.get(timeout=300)
    finally:
        proc.join(timeout=120)
        if proc.is_alive():
            proc.kill()
    assert proc.exitcode == 0
    params, batch, s = OC.model_case("padded")
    single = OC.make_engine(params, s, objective="rel_l2")
    for _ in range(2):
        single.train_step(*OC.step_args(OC.to_dev(batch)))
    torch.cuda.synchronize()
    for overlap in (True, False):
        names, flat, value = out[overlap]
        assert names == single.api.names and "cfd_fno_backward_phase_ex" not in names and names.count("cfd_objective_bwd") == 2
        assert np.array_equal(flat.view(np.uint32), single.flat.data.cpu().numpy().view(np.uint32)) and value == float(single.objective_value())


# ---- the eager path ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", OC.KINDS)
def test_objective_loss_gradient_against_fp64(kind):
    """functional.objective_loss: one autograd node, the upstream gradient read on the device; value and gradient within the kernel's
    derived bound of the fp64 formula (tests/test_cpu_objective.py holds that formula to torch's fp64 autograd and to the reference)."""
    import torch

    from cfdbench_amd.functional import objective_loss
    shape = (3, 2, 66 * 65)
    preds, label, mask, _gadd = OC.case(*shape, seed=6)
    p = torch.from_numpy(preds.reshape(3, 2, 66, 65)).cuda().requires_grad_(True)
    lab, m = torch.from_numpy(label.reshape(3, 2, 66, 65)).cuda(), torch.from_numpy(mask.reshape(3, 1, 66, 65)).cuda()
    value = objective_loss(p, lab, kind, m)
    (value * 0.37).backward()
    ref = OC.reference(preds, label, mask, kind, upstream=float(np.float32(0.37)))
    assert value.dim() == 0 and abs(float(value.detach()) - ref["value"]) <= OC.UNITS["value"] * OC.SLACK * OC.U * ref["value"]
    err = np.abs(p.grad.cpu().numpy().reshape(shape).astype(f64) - ref["grad"])
    assert (err <= OC.UNITS["grad"] * OC.SLACK * OC.U * np.abs(ref["grad"])).all()
    # without a mask, and through ObjectiveLoss: the dict of MseLoss plus the objective under its name
    from cfdbench_amd.models.loss import objective_to_fn
    out = objective_to_fn(kind)(p.detach(), lab)
    assert list(out) == ["mse", "rmse", "mae", "nmse", kind]
    want = OC.reference(preds, label, None, kind)["value"]
    assert abs(float(out[kind]) - want) <= OC.UNITS["value"] * OC.SLACK * OC.U * want


@pytest.mark.parametrize("kind", OC.KINDS)
def test_objective_loss_on_views(kind):
    """What tests/test_gpu_views.py asks of every autograd node of functional.py, for the node of cfdbench_amd/objective.py: predictions,
    labels and mask as contiguous views 4 bytes off the allocation, as slices of a larger batch and non-contiguous (channels_last) give
    the value and the gradient of the plain tensors, bit for bit -- the scalar form owns the same elements in the same order."""
    import torch

    from cfdbench_amd.functional import objective_loss
    from cfdbench_amd.objective import ObjectiveLossFn
    from tests.test_gpu_views import batch_slice, non_contiguous, offset_view
    preds, label, mask, _g = OC.case(3, 2, 64 * 64, seed=8)
    plain = [torch.from_numpy(a).cuda() for a in (preds.reshape(3, 2, 64, 64), label.reshape(3, 2, 64, 64), mask.reshape(3, 1, 64, 64))]

    def run(p, lab, m):
        p = p.detach().requires_grad_(True)
        value = objective_loss(p, lab, kind, m)
        assert type(value.grad_fn).__name__ == ObjectiveLossFn.__name__ + "Backward"
        (value * 0.5).backward()
        return value.detach().clone().view(torch.int32), p.grad.contiguous().view(torch.int32)

    want = run(*plain)
    for how in (offset_view, batch_slice, non_contiguous):
        got = run(*[how(torch, t) for t in plain])  # (run() detaches: the leaf keeps the view's offset and strides)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), how.__name__


@pytest.mark.parametrize("kind", OC.KINDS)
@pytest.mark.parametrize("name", ["pair", "chan"])
def test_model_loss_backward_against_the_oracle_chain(name, kind):
    """model(**batch)["loss"][kind].backward(): Fno2d's parameter gradients through gpreds_ext against the chain of the engine tests."""
    import torch

    from oracle import fno_oracle as O
    params, batch, s = OC.model_case(name)
    model = OC.make_model(params, s, loss=kind)
    out = model(**OC.to_dev(batch))
    assert list(out["loss"]) == ["mse", "rmse", "mae", "nmse", kind]
    out["loss"][kind].backward()
    torch.cuda.synchronize()
    ref = OC.ref_pass(params, batch, s, kind)
    assert abs(float(out["loss"][kind].detach()) - ref["value"]) <= OC.VALUE_TOL * ref["value"]
    res = {k: O.rel_nmse(p_.grad.cpu().numpy(), ref["grads"][k]) for k, p_ in model.named_parameters()}
    print("objective eager", name, kind, max(res.values()))
    assert all(v <= OC.grad_tol(name) for v in res.values()), res


def test_unrolled_loss_sums_the_objective():
    import torch

    from cfdbench_amd.unroll import unrolled_loss
    from oracle import fno_oracle as O
    from tests import ingrad_checks as IC
    params, batch, s = OC.model_case("pair")
    labels = IC.unroll_labels(47, batch, 2)
    model = OC.make_model(params, s, loss="rel_l2")
    tb = OC.to_dev(batch)
    loss, preds = unrolled_loss(model, tb["inputs"], [torch.from_numpy(a).cuda() for a in labels], tb["case_params"], tb["mask"], key="rel_l2")
    loss.backward()
    ref = OC.ref_window(params, batch, s, "rel_l2", labels)
    assert len(preds) == 2 and abs(float(loss.detach()) - np.mean(ref["values"])) <= OC.VALUE_TOL * np.mean(ref["values"])
    res = {k: O.rel_nmse(p_.grad.cpu().numpy(), ref["grads"][k]) for k, p_ in model.named_parameters()}
    assert all(v <= OC.grad_tol("pair") for v in res.values()), res


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def _toy_model():
    params, _b, s = OC.model_case("padded")
    return OC.make_model(params, dict(s, pad=0))


def _data():
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    return (SyntheticAutoDataset(n_cases=4, n_frames=5, height=32, width=32, seed=0),
            SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1))


KW = dict(batch_size=4, eval_batch_size=4, log_interval=2, eval_interval=1, plot_interval=0, lr=5e-3)


def test_train_auto_fused_objective_writes_both_histories_and_resumes(tmp_path):
    import json

    import torch

    from cfdbench_amd.harness.train_auto import train
    tr, dev = _data()
    torch.manual_seed(3)
    train(_toy_model(), tr, dev, tmp_path / "whole", num_epochs=3, fused=True, objective="rel_l2", **KW)
    torch.manual_seed(3)
    train(_toy_model(), tr, dev, tmp_path / "parts", num_epochs=2, fused=True, objective="rel_l2", **KW)
    state = torch.load(tmp_path / "parts" / "train_state.pt", map_location="cpu", weights_only=False)
    assert state["objective"] == "rel_l2" and len(state["train_objective"]) == len(state["train_losses"]) > 0
    with pytest.raises(RuntimeError, match="--objective rel_l2"):
        train(_toy_model(), tr, dev, tmp_path / "parts", num_epochs=3, fused=True, resume=True, **KW)
    train(_toy_model(), tr, dev, tmp_path / "parts", num_epochs=3, fused=True, objective="rel_l2", resume=True, **KW)
    for f in ("train_losses.json", "train_objective.json"):
        assert json.loads((tmp_path / "whole" / f).read_text()) == json.loads((tmp_path / "parts" / f).read_text()), f
    hist = json.loads((tmp_path / "whole" / "train_objective.json").read_text())["rel_l2"]
    nmse = json.loads((tmp_path / "whole" / "train_losses.json").read_text())
    assert len(hist) == len(nmse) and np.isfinite(hist).all() and np.mean(hist[-4:]) < np.mean(hist[:4])
    a = torch.load(tmp_path / "whole" / "ckpt-2" / "model.pt", map_location="cpu")
    b = torch.load(tmp_path / "parts" / "ckpt-2" / "model.pt", map_location="cpu")
    assert all(torch.equal(a[k], b[k]) for k in a)
    scores = json.loads((tmp_path / "whole" / "ckpt-2" / "scores.json").read_text())
    dev_scores = json.loads((tmp_path / "whole" / "ckpt-2" / "dev_scores.json").read_text())
    assert scores["dev_loss"] == float(np.mean(dev_scores["all"]["nmse"])) and "rel_l2" in dev_scores["mean"]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "eager"])
def test_train_auto_objective_with_the_other_options(tmp_path, fused):
    """Rollout windows of two, clipping, the guard, averaged weights and a frozen lifting layer (fused: with accumulation groups of two) on
    an objective: finite histories of equal length, model_ema.pt beside model.pt."""
    import json

    import torch

    from cfdbench_amd.harness.common import apply_trainable
    from cfdbench_amd.harness.train_auto import train
    tr, dev = _data()
    model = _toy_model()
    apply_trainable(model, "fc0", "")
    torch.manual_seed(4)
    train(model, tr, dev, tmp_path / "run", num_epochs=2, fused=fused, objective="nmse_sample", unroll_steps=2, max_grad_norm=1.0,
          skip_nonfinite=True, ema_decay=0.9, gradient_accumulation_steps=2 if fused else 1, **KW)
    hist = json.loads((tmp_path / "run" / "train_objective.json").read_text())["nmse_sample"]
    nmse = json.loads((tmp_path / "run" / "train_losses.json").read_text())
    assert len(hist) == len(nmse) > 0 and np.isfinite(hist).all() and np.isfinite(nmse).all()
    assert (tmp_path / "run" / "ckpt-1" / "model_ema.pt").exists() and (tmp_path / "run" / "ckpt-1" / "train_objective.json").exists()
