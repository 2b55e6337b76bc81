"""MI355X: training through a K-step rollout window on the fused engine -- the call sequence over the C ABI (tests/window_checks.py, the
checks of tests/test_emul_fno_window.py plus the K = 3 fixture and the benchmark's width), FnoTrainEngine.accumulate_window / train_window,
and train_auto --fused 1 --unroll_steps K."""
import os

import numpy as np
import pytest

from tests import clip_checks as CC
from tests import fno_checks as F
from tests import ingrad_checks as IC
from tests import window_checks as WC

pytestmark = pytest.mark.gpu

HEADS = {"one_pass_head": True, "two_pass_head": False}


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


# ---- the sequence over the C ABI ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", list(HEADS))
def test_window_of_three_vs_reference_golden(be, head):
    """The reference's own unrolled run at the bound the eager window is held to (tests/test_gpu_fno_ingrad.py)."""
    res, loss_err = WC.check_golden(be, HEADS[head])
    print(head, res, "loss", loss_err)
    _assert_all(res, WC.MODEL_TOL)
    assert loss_err <= 5e-6


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("name", list(WC.CASES))
def test_window_vs_fp64(be, name, head):
    res = WC.check_small(be, name, HEADS[head])
    print(name, head, res)
    _assert_all(res, WC.ABI_TOL)


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("name", ["9x7_scalar_form", "12x12_pad4", "64x64_w20_b5"])
def test_two_windows_with_weight_one_half(be, name, head):
    _assert_all(WC.check_two_windows(be, name, HEADS[head]), WC.ABI_TOL)


@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("name", ["9x7_scalar_form", "64x64_w20_b5"])
def test_first_window_never_reads_the_accumulator_and_repeats_bitwise(be, name, head):
    WC.check_poisoned_accumulator_and_repeat(be, name, HEADS[head])


@pytest.mark.parametrize("head,flags", [("one_pass_head", 0), ("one_pass_head", 7), ("two_pass_head", 0)])
@pytest.mark.parametrize("name", ["9x7_scalar_form", "p8_cin3", "64x64_w20_b5"])
def test_detached_window_is_the_mean_of_the_one_step_gradients(be, name, head, flags):
    """flags = 7: the single-GPU engine's deferred passes, as `accumulate` runs them."""
    res, far = WC.check_detach(be, name, HEADS[head], flags)
    print(name, head, flags, res, "distance from the full gradient", far)
    _assert_all(res, WC.ABI_TOL)
    assert far > 1e3 * WC.ABI_TOL, f"the truncated gradient equals the full one ({far}): the flag does nothing"


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _model(params, s, cout=None):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    model = Fno2d(s["cin"], s["cin"] if cout is None else cout, s["p"], loss_name_to_fn("nmse"), s["L"], s["m1"], s["m2"], s["C"],
                  padding=s["pad"] or None).to(torch.device("cuda", 0))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model


def _dev(batch, labels):
    import torch
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    return (tb["inputs"], [torch.from_numpy(a).cuda() for a in labels], tb["case_params"], tb["mask"])


def _engine(params, s, **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    return FnoTrainEngine(_model(params, s), lr=1e-3, loss_name="nmse", **kw)


def _golden_window():
    g = IC.load_golden("fno_unroll3")
    params, batch, s = IC.golden_case(g)
    K_, lseed = int(g["meta"][13]), int(g["meta"][14])
    return g, params, s, _dev(batch, IC.unroll_labels(lseed, batch, K_)), K_


def _tensors_of(flat, params, L):
    layout, _n, _f = F.flat_layout(params, L)
    out = {}
    for q, v in params.items():
        sl = F.flat_slice(flat, layout, q)
        out[q] = sl.reshape(*v.shape, 2).view(np.complex64).reshape(v.shape) if np.iscomplexobj(v) else sl.reshape(v.shape)
    return out


@pytest.mark.parametrize("fused_head", [True, False], ids=list(HEADS))
def test_train_window_vs_reference_golden(fused_head):
    """train_window, K = 3: gradients() against the fixture's sampled parameter gradients, the predictions and, from the (K, 4) sums, the
    loss; one optimiser step was taken on it."""
    import torch
    g, params, s, win, K_ = _golden_window()
    eng = _engine(params, s, fused_head=fused_head)
    flat0 = eng.flat.data.clone()
    sums = eng.train_window(*win)
    assert tuple(sums.shape) == (K_, 4) and eng.step_count == 1 and not eng._accum_open
    preds = eng.preds_seq()
    assert len(preds) == K_
    res = {"preds": IC.golden_field(g, "preds", np.stack([p_.cpu().numpy() for p_ in preds]))}
    res.update(IC.golden_gsums(g, _tensors_of(eng.gradients().cpu().numpy(), params, s["L"])))
    rows = sums.cpu().numpy().astype(np.float64)
    loss = float(np.mean(rows[:, 0] / rows[:, 2]))
    print(res, loss, float(g["loss"]))
    _assert_all(res, WC.MODEL_TOL)
    assert abs(loss - float(g["loss"])) <= 5e-6 * abs(float(g["loss"]))
    assert np.all(rows[:, 3] == rows[0, 3]) and rows[0, 3] > 0
    assert not torch.equal(flat0, eng.flat.data)


def test_window_of_one_is_the_accumulate_call_bit_for_bit():
    import torch
    g, params, s, (x, labels, cp, mask), _ = _golden_window()
    a, b = _engine(params, s), _engine(params, s)
    for _ in range(2):
        sa = a.train_window(x, labels[:1], cp, mask)
        sb = b.accumulate(x, labels[0], cp, mask, weight=1.0, first=True)
        b.apply_accumulated()
        assert tuple(sa.shape) == (1, 4) and torch.equal(sa[0], sb)
    assert a.step_count == b.step_count == 2
    for q in ("data",):
        assert torch.equal(getattr(a.flat, q), getattr(b.flat, q))
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.preds_seq()[0], b.preds)


def test_train_window_with_clipping_reports_the_norm_of_the_window_gradient():
    """grad_norm() against the fp64 norm of gradients() -- the whole window's accumulator -- at tests/clip_checks.py's bound; with a
    threshold of half that norm the coefficient is 1 / 2 and reaches Adam."""
    import torch
    g, params, s, win, _ = _golden_window()
    probe = _engine(params, s, max_grad_norm=float("inf"))
    probe.train_window(*win)
    norm = float(probe.gradients().double().norm())
    assert abs(float(probe.grad_norm()) - norm) <= CC.CLIP_TOL * norm and float(probe.clip_coef()) == 1.0
    eng = _engine(params, s, max_grad_norm=0.5 * norm)
    eng.train_window(*win)
    assert abs(float(eng.grad_norm()) - norm) <= CC.CLIP_TOL * norm
    assert abs(float(eng.clip_coef()) - 0.5) <= 1e-5
    assert IC.nm(eng.exp_avg.cpu().numpy(), 0.5 * probe.exp_avg.cpu().numpy()) < 1e-9
    assert torch.equal(eng.gradients(), probe.gradients()), "the accumulator is left unclipped"


@pytest.mark.parametrize("detach", [False, True], ids=["full", "detach"])
def test_two_accumulated_windows_then_one_optimiser_step(detach):
    """accumulate_window twice (weight 1 / 2) + apply_accumulated: the accumulator is the mean of the two windows' own gradients -- each add
    rounds once, 2^-24 relative per pass, so nMSE <= (K 2^-24)^2 = 3e-14 (1e-12 asked) -- and ONE optimiser step was taken."""
    params, batch, labels, s, K_ = WC.case("64x64_w20_b5")
    _p, batch2, labels2, _s, _k = WC.case("64x64_w20_b5", bseed=52)
    w1, w2 = _dev(batch, labels), _dev(batch2, labels2)
    singles = []
    for w in (w1, w2):
        e = _engine(params, s)
        e.train_window(*w, detach=detach)
        singles.append(e.gradients().double().cpu().numpy())
    eng = _engine(params, s)
    eng.accumulate_window(*w1, weight=0.5, first=True, detach=detach)
    with pytest.raises(RuntimeError, match="accumulation group is open"):
        eng.train_step(w1[0], w1[1][0], w1[2], w1[3])
    eng.accumulate_window(*w2, weight=0.5, first=False, detach=detach)
    eng.apply_accumulated()
    assert eng.step_count == 1
    err = IC.nm(eng.gradients().cpu().numpy(), 0.5 * (singles[0] + singles[1]))
    assert err < 1e-12, err
    assert IC.nm(singles[0], singles[1]) > 1e-3
    with pytest.raises(RuntimeError, match="first=False"):
        eng.accumulate_window(*w1, weight=0.5, first=False)
    eng.train_step(w1[0], w1[1][0], w1[2], w1[3])  # (a closed group leaves the plain step as it was)
    assert eng.step_count == 2


def test_window_needs_matching_channel_counts():
    import torch

    from cfdbench_amd.engine import FnoTrainEngine
    (B, C, L, H, W, m1, m2, p, cin, pad), _ = WC.CASES["p8_cin3"]
    params, batch = IC.small_case(B, C, L, H, W, m1, m2, p, cin, pad, cout=2)
    s = dict(L=L, C=C, H=H, W=W, p=p, m1=m1, m2=m2, pad=pad, cin=cin)
    eng = FnoTrainEngine(_model(params, s, cout=2), lr=1e-3, loss_name="nmse")
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    with pytest.raises(ValueError, match="in_chan == out_chan"):
        eng.train_window(tb["inputs"], [tb["label"], tb["label"]], tb["case_params"], tb["mask"])
    assert eng.accum is None and not eng._accum_open and eng.step_count == 0
    eng.train_step(tb["inputs"], tb["label"], tb["case_params"], tb["mask"])
    torch.cuda.synchronize()


def test_bf16_storage_refuses_the_full_gradient_and_runs_the_truncated_one():
    import torch
    g, params, s, win, K_ = _golden_window()
    eng = _engine(params, s, act_dtype="bf16")
    with pytest.raises(ValueError, match="fp32 activation storage"):
        eng.train_window(*win)
    assert eng.accum is None and not eng._accum_open and eng.step_count == 0
    sums = eng.train_window(*win, detach=True)
    assert eng.step_count == 1 and tuple(sums.shape) == (K_, 4)
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(eng.flat.data).all()) and bool(torch.isfinite(eng.gradients()).all())
    fp32 = _engine(params, s)
    fp32.train_window(*win, detach=True)
    err = IC.nm(eng.gradients().cpu().numpy(), fp32.gradients().cpu().numpy())
    assert 0.0 < err < 1e-2, err  # (bf16-stored activations: close to the fp32-storage gradient, not equal to it)


def test_detached_engine_window_vs_fp64():
    """The engine's truncated window (deferred passes, one-pass head) against the fp64 mean of the one-step gradients."""
    name = "64x64_w20_b5"
    params, batch, labels, s, K_ = WC.case(name)
    eng = _engine(params, s)
    assert eng.defer_flags == 7
    eng.train_window(*_dev(batch, labels), detach=True)
    ref = WC.ref_detached(name)
    got = _tensors_of(eng.gradients().cpu().numpy(), params, s["L"])
    res = {q: IC.nm(got[q], ref["grads"][q]) for q in params}
    res.update({f"preds_{k + 1}": IC.nm(p_.cpu().numpy(), ref["preds"][k]) for k, p_ in enumerate(eng.preds_seq())})
    _assert_all(res, WC.ABI_TOL)


def _rccl_worker(port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_DP_ALWAYS_EXCHANGE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                      NCCL_SOCKET_IFNAME="lo")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        params, batch, labels, s, _ = WC.case("64x64_w20_b5")
        eng = _engine(params, s)
        assert eng.sync.exchange and eng.defer_flags == 0
        eng.train_window(*_dev(batch, labels))
        q.put((eng.gradients().cpu().numpy().copy(), [p_.cpu().numpy().copy() for p_ in eng.preds_seq()], eng.step_count))
    finally:
        dist.destroy_process_group()


def test_train_window_over_a_one_rank_rccl_group():
    """The data-parallel window (a one-rank RCCL group with the exchange forced on, as tests/test_gpu_dp.py runs it): the accumulator is
    all-reduced once, in apply_accumulated; the window against fp64."""
    import socket

    import torch.multiprocessing as mp
    sock = socket.socket()
    sock.bind(("127.0.0.1", 0))
    port = sock.getsockname()[1]
    sock.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_rccl_worker, args=(port, q))
    proc.start()
    try:
        flat, preds, steps = q.get(timeout=300)
    finally:
        proc.join(timeout=120)
        if proc.is_alive():
            proc.kill()
    assert proc.exitcode == 0 and steps == 1
    params, _batch, _labels, s, _ = WC.case("64x64_w20_b5")
    ref = WC.ref_full("64x64_w20_b5")
    got = _tensors_of(flat, params, s["L"])
    res = {q_: IC.nm(got[q_], ref["grads"][q_]) for q_ in params}
    res.update({f"preds_{k + 1}": IC.nm(p_, ref["preds"][k]) for k, p_ in enumerate(preds)})
    _assert_all(res, WC.ABI_TOL)


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "plain": [],
    "device_loader": ["--device_loader", "1"],
    "detach": ["--unroll_detach", "1"],
    "accumulation_and_clipping": ["--fused_accumulation_steps", "2", "--max_grad_norm", "1"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_train_auto_fused_unroll_steps(tmp_path, variant):
    """train_auto --fused 1 --unroll_steps 3 on synthetic data: two epochs over the windows, the usual artefacts, a falling loss; the
    training state records unroll_steps and unroll_detach, and a resume with either changed is refused."""
    import torch

    from cfdbench_amd.harness.args import Args, is_args_valid
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir, load_json
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train
    from cfdbench_amd.unroll import unroll_windows

    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--fno_hidden_dim", "8", "--fno_depth", "2",
                              "--lr", "0.005", "--output_dir", str(tmp_path), "--num_epochs", "2", "--batch_size", "4", "--eval_batch_size", "4",
                              "--eval_interval", "1", "--log_interval", "3", "--plot_interval", "0", "--fused", "1", "--unroll_steps", "3"]
                             + VARIANTS[variant])
    is_args_valid(args)
    out = get_output_dir(args, is_auto=True)
    tr = SyntheticAutoDataset(n_cases=6, n_frames=6, height=32, width=32, seed=0)
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    n_windows = len(unroll_windows(tr, 3)[0])
    assert n_windows == 6 * 3
    torch.manual_seed(0)
    model = init_model(args).cuda()
    kw = dict(lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma, batch_size=4, eval_batch_size=4, log_interval=3,
              eval_interval=1, plot_interval=0, fused=True, device_loader=bool(args.device_loader),
              gradient_accumulation_steps=args.fused_accumulation_steps, max_grad_norm=args.max_grad_norm)
    losses = train(model, tr, dev, out, num_epochs=2, unroll_steps=args.unroll_steps, unroll_detach=bool(args.unroll_detach), **kw)
    assert len(losses) == 2 * ((n_windows + 3) // 4) and np.all(np.isfinite(losses))
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), "training through the rollout does not reduce the loss"
    for ep in (0, 1):
        d = out / f"ckpt-{ep}"
        assert (d / "model.pt").exists() and (d / "dev_scores.json").exists() and (d / "train_loss.json").exists()
        assert set(load_json(d / "scores.json")) == {"ep", "train_loss", "dev_loss", "time"}
    assert (out / "train_losses.json").exists() and (out / "train_state.pt").exists()
    state = torch.load(out / "train_state.pt", map_location="cpu", weights_only=False)
    assert state["unroll_steps"] == 3 and state["unroll_detach"] == int(args.unroll_detach) and state["fused"]
    with pytest.raises(RuntimeError, match="unroll_detach"):
        train(model, tr, dev, out, num_epochs=3, resume=True, unroll_steps=3, unroll_detach=not args.unroll_detach, **kw)
    with pytest.raises(RuntimeError, match="unroll_steps"):
        train(model, tr, dev, out, num_epochs=3, resume=True, **kw)
