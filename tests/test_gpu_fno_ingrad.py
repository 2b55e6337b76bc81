"""MI355X: the FNO's gradients with respect to its inputs and case parameters -- through the C ABI (the checks of
tests/test_emul_fno_ingrad.py on the device), through Fno2d's autograd node, through cfdbench_amd.unroll and through train_auto
--unroll_steps."""
import numpy as np
import pytest

from tests import ingrad_checks as IC

pytestmark = pytest.mark.gpu

ABI_TOL = 1e-9    # C ABI against fp64
MODEL_TOL = 1e-8  # against the reference's fp32 fixtures (tests/test_gpu_model.py's bound on parameter gradients)


@pytest.fixture(scope="module")
def be():
    from tests.backends import TorchBackend
    return TorchBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_all(res, tol):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
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


# (B, C, L, H, W, m1, m2, p, cin, pad, kwargs): the emulator's shapes plus the benchmark's width at a batch that cuts several records
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
    "b500_c1_record_cut": (500, 1, 0, 33, 33, 2, 2, 12, 1, 0, {}),
    "64x64_w20_b5": (5, 20, 2, 64, 64, 12, 12, 5, 2, 0, {}),
}
WANTS = {"both": ("inputs", "case_params"), "inputs": ("inputs",), "case_params": ("case_params",)}


@pytest.mark.parametrize("want", list(WANTS))
@pytest.mark.parametrize("case", list(SMALL))
def test_small_shapes_vs_fp64(be, case, want):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    _assert_all(IC.check_small(be, B, C, L, H, W, m1, m2, p, cin, pad, want=WANTS[want], **kw), ABI_TOL)


@pytest.mark.parametrize("case", ["9x7_scalar_form", "64x64_w20_b5"])
def test_small_shape_through_the_phases(be, case):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    _assert_all(IC.check_small(be, B, C, L, H, W, m1, m2, p, cin, pad, route="phases"), ABI_TOL)


@pytest.mark.parametrize("shift", [4, 8])
@pytest.mark.parametrize("case", ["p8_cin3", "66x65_8byte_form", "64x64_w20_b5"])
def test_misaligned_buffers(be, case, shift):
    """Every tensor -- d_inputs and d_case_params among them -- `shift` bytes past a 16-byte boundary."""
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    with be.misaligned(shift):
        res = IC.check_small(be, B, C, L, H, W, m1, m2, p, cin, pad)
        assert be.allocations >= 10
    _assert_all(res, ABI_TOL)


@pytest.mark.parametrize("case", ["p8_cin3", "12x12_pad4", "c33", "64x64_w20_b5"])
def test_nothing_else_moves(be, case):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    res = IC.check_nothing_else_moves(be, B, C, L, H, W, m1, m2, p, cin, pad)
    assert res == dict(preds_sums=0.0, param_grads=0.0), res


def test_fused_step_with_null_pointers_still_defers(be):
    """What this checks is behaviour, not bits against a recording: fno_checks.run_fused_steps fills a zeroed struct (both pointers NULL)
    and the deferrals stay on.  Under flags = 7 the raw first gradient is still short of the nMSE normaliser count / sum (label mask)^2 =
    sums[3] / sums[2] -- times that factor it is the flags = 0 gradient -- while the predictions are the same bits and the parameters
    after two steps agree.  That the default step keeps its bits is what the unchanged suite (its fixtures and bitwise checks) holds."""
    params, batch = IC.small_case(3, 20, 2, 64, 64, 12, 12, 5, 2)
    out, layout = IC.F.run_fused_steps(be, params, batch, 2, 20, 64, 64, 5)
    a, b = out[0], out[7]
    factor = float(b["sums1"][3]) / float(b["sums1"][2])
    assert abs(factor - 1.0) > 1e-3, factor  # (so that a gradient without the deferral is told from one with it: nMSE >= 1e-6 apart)
    assert IC.nm(b["g1"], a["g1"]) > 1e-7, "flags = 7 no longer defers the normaliser"
    assert IC.nm(b["g1"] * np.float32(factor), a["g1"]) < 1e-9
    assert np.array_equal(a["preds1"], b["preds1"])
    assert IC.nm(b["flat"], a["flat"]) < 1e-9


@pytest.mark.parametrize("case", ["p8_cin3", "66x65_8byte_form", "64x64_w20_b5"])
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


@pytest.mark.parametrize("case", ["p8_cin3", "12x12_pad4", "64x64_w20_b5"])
def test_chain_rule_over_two_steps(be, case):
    B, C, L, H, W, m1, m2, p, cin, pad, kw = SMALL[case]
    _assert_all(IC.check_chain(be, B, C, L, H, W, m1, m2, p, cin, pad), ABI_TOL)


# ---- torch level -------------------------------------------------------------------------------------------------------------------
def _model_of(g):
    """(Fno2d on the device with the fixture's weights, its batch as device tensors, the fixture's shape record)."""
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn

    params, batch, s = IC.golden_case(g)
    model = Fno2d(s["cin"], s["cin"], s["p"], loss_name_to_fn("nmse"), s["L"], s["m1"], s["m2"], s["C"],
                  padding=s["pad"] or None).to(torch.device("cuda", 0))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model, {k: torch.from_numpy(v).cuda() for k, v in batch.items()}, s


def _offset_view(torch, t):
    """`t` as a contiguous view at a storage offset of one float (4 bytes off the allocation's alignment)."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = big[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == 1
    return v


@pytest.mark.parametrize("placement", ["contiguous", "offset_view"])
@pytest.mark.parametrize("name", ["fno_ingrad_c3", "fno_pad9_66x65"])
def test_fno2d_input_gradients_vs_reference_golden(name, placement):
    """inputs.grad and case_params.grad of Fno2d against the reference's (and its sampled parameter gradients), on plain tensors and on
    views at a storage offset."""
    import torch

    g = IC.load_golden(name)
    model, tb, s = _model_of(g)
    if placement == "offset_view":
        tb = {k: _offset_view(torch, v) for k, v in tb.items()}
    tb["inputs"].requires_grad_(True)
    tb["case_params"].requires_grad_(True)
    out = model(**tb)
    out["loss"]["nmse"].backward()
    res = {"g_inputs": IC.golden_field(g, "g_inputs", tb["inputs"].grad.cpu().numpy())}
    if "g_case_params" in g.files:
        res["g_case_params"] = IC.nm(tb["case_params"].grad.cpu().numpy(), g["g_case_params"])
    else:
        assert tb["case_params"].grad is not None and bool(torch.isfinite(tb["case_params"].grad).all())
    res.update(IC.golden_gsums(g, {k: v.grad.cpu().numpy() for k, v in model.named_parameters()}))
    _assert_all(res, MODEL_TOL)


def test_frozen_parameters_still_give_the_input_gradient():
    import torch

    g = IC.load_golden("fno_ingrad_c3")
    model, tb, s = _model_of(g)
    for q in model.parameters():
        q.requires_grad_(False)
    tb["inputs"].requires_grad_(True)
    out = model(**tb)
    assert out["preds"].requires_grad
    out["loss"]["nmse"].backward()
    assert all(q.grad is None for q in model.parameters()) and tb["case_params"].grad is None
    assert IC.golden_field(g, "g_inputs", tb["inputs"].grad.cpu().numpy()) < MODEL_TOL
    assert torch.isfinite(tb["inputs"].grad).all()


def test_no_grad_takes_the_inference_workspace(monkeypatch):
    """Under torch.no_grad() the call asks for the forward-only workspace whatever requires_grad says, and with grad mode on an input that
    requires a gradient is enough for the training one."""
    import torch

    from cfdbench_amd import _lib

    model, tb, s = _model_of(IC.load_golden("fno_ingrad_c3"))
    for q in model.parameters():
        q.requires_grad_(False)
    tb["inputs"].requires_grad_(True)
    api, asked = _lib.api(), []
    size = api.size

    def spy(name, *args):
        if name == "cfd_fno_workspace_bytes":
            asked.append(int(args[2]))
        return size(name, *args)

    monkeypatch.setattr(api, "size", spy)
    with torch.no_grad():
        out = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])
    assert asked == [0] and not out["preds"].requires_grad
    out = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])
    assert asked == [0, 1] and out["preds"].requires_grad
    torch.cuda.synchronize()


def test_unrolled_loss_vs_reference_golden():
    """cfdbench_amd.unroll.unrolled_loss, K = 3, against the reference's unrolled run (tools/make_golden_ingrad.py): the three predictions,
    the loss, inputs.grad, case_params.grad and the sampled parameter gradients -- the part of the parameter gradient that flows through
    the fed-back frames included."""
    import torch

    from cfdbench_amd.unroll import unrolled_loss

    g = IC.load_golden("fno_unroll3")
    model, tb, s = _model_of(g)
    K_, lseed = int(g["meta"][13]), int(g["meta"][14])
    _params, batch, _s = IC.golden_case(g)
    labels = [torch.from_numpy(a).cuda() for a in IC.unroll_labels(lseed, batch, K_)]
    tb["inputs"].requires_grad_(True)
    tb["case_params"].requires_grad_(True)
    loss, preds = unrolled_loss(model, tb["inputs"], labels, tb["case_params"], tb["mask"])
    loss.backward()
    assert len(preds) == K_
    res = {"preds": IC.golden_field(g, "preds", np.stack([q.detach().cpu().numpy() for q in preds]))}
    res.update(g_inputs=IC.golden_field(g, "g_inputs", tb["inputs"].grad.cpu().numpy()),
               g_case_params=IC.nm(tb["case_params"].grad.cpu().numpy(), g["g_case_params"]))
    res.update(IC.golden_gsums(g, {k: v.grad.cpu().numpy() for k, v in model.named_parameters()}))
    assert abs(loss.item() - float(g["loss"])) <= 5e-6 * abs(float(g["loss"]))
    _assert_all(res, MODEL_TOL)


# ---- harness -----------------------------------------------------------------------------------------------------------------------
def test_train_auto_unroll_steps(tmp_path):
    """train_auto --unroll_steps 3 on synthetic data: two epochs over the windows, the usual artefacts, a falling loss; the training state
    records unroll_steps and a one-step resume from it is refused."""
    import torch

    from cfdbench_amd.harness.args import Args, is_args_valid
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir, load_json
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train
    from cfdbench_amd.unroll import unroll_windows

    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--fno_hidden_dim", "8", "--fno_depth", "2",
                              "--lr", "0.005", "--output_dir", str(tmp_path), "--num_epochs", "2", "--batch_size", "4", "--eval_batch_size", "4",
                              "--eval_interval", "1", "--log_interval", "5", "--plot_interval", "0", "--unroll_steps", "3"])
    is_args_valid(args)
    out = get_output_dir(args, is_auto=True)
    tr = SyntheticAutoDataset(n_cases=6, n_frames=6, height=32, width=32, seed=0)
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    n_windows = len(unroll_windows(tr, 3)[0])
    assert n_windows == 6 * 3
    torch.manual_seed(0)
    model = init_model(args).cuda()
    losses = train(model, tr, dev, out, num_epochs=2, lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma, batch_size=4,
                   eval_batch_size=4, log_interval=5, eval_interval=1, plot_interval=0, unroll_steps=args.unroll_steps)
    assert len(losses) == 2 * ((n_windows + 3) // 4) and np.all(np.isfinite(losses))
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), "training through the rollout does not reduce the loss"
    for ep in (0, 1):
        d = out / f"ckpt-{ep}"
        assert (d / "model.pt").exists() and (d / "dev_scores.json").exists() and (d / "train_loss.json").exists()
        assert set(load_json(d / "scores.json")) == {"ep", "train_loss", "dev_loss", "time"}
    assert (out / "train_losses.json").exists() and (out / "train_state.pt").exists()
    # the run shares its directory with the one-step run of the same arguments: the state says which it was, and a resume as another refuses
    assert torch.load(out / "train_state.pt", map_location="cpu", weights_only=False)["unroll_steps"] == 3
    with pytest.raises(RuntimeError, match="unroll_steps"):
        train(model, tr, dev, out, num_epochs=3, lr=args.lr, batch_size=4, eval_batch_size=4, eval_interval=1, plot_interval=0, resume=True)
