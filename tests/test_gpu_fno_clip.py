"""MI355X: gradient-norm clipping inside the fused FNO step's optimiser call -- the C-ABI rows of tests/test_emul_fno_clip.py on the device,
FnoTrainEngine(max_grad_norm=) against an unclipped engine, against the eager autograd path with torch.nn.utils.clip_grad_norm_, on the
flags = 0 routes and under graph replay, and train_auto --max_grad_norm."""
import os

import numpy as np
import pytest

from oracle import fno_oracle as O
from oracle import synth
from tests import clip_checks as CC

pytestmark = pytest.mark.gpu

C, L, P, H, W, B = 20, 2, 5, 64, 64, 4


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
@pytest.mark.parametrize("name", list(CC.CASES))
def test_threshold_that_does_not_bite_is_bitwise_the_unclipped_step(be, name):
    norm1 = CC.check_coef_one_is_bitwise(be, name, "inf", float("inf"))
    CC.check_coef_one_is_bitwise(be, name, "above", 1e3 * norm1)


@pytest.mark.parametrize("name", list(CC.CASES))
def test_clipped_step_against_the_rule(be, name):
    CC.check_clipped(be, name)


def test_bad_thresholds_are_refused_before_any_launch(be):
    got = CC.check_refusals(be)
    assert got == {repr(b): (-1, True) for b in (0.0, -1.0, float("nan"))}, got


def test_empty_buffer(be):
    pair, untouched = CC.check_empty(be)
    assert pair.tolist() == [0.0, 1.0] and untouched, (pair, untouched)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _make_model(torch):
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    params = synth.make_fno_params(301, C, L, 12, 12, P, spectral_gain=4.0)
    m = Fno2d(2, 2, P, loss_name_to_fn("nmse"), L, 12, 12, C).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return m


def _batch(torch, step):
    b = synth.make_batch(311 + step, B, H, W, P, border_mask=True)
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in b.items()}


def _engine(torch, **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    return FnoTrainEngine(_make_model(torch), lr=1e-3, loss_name="nmse", **kw)


def _steps(torch, eng, n, graph=False):
    for step in range(n):
        b = _batch(torch, step)
        (eng.train_step_graph if graph else eng.train_step)(b["inputs"], b["label"], b["case_params"], b["mask"])
    torch.cuda.synchronize()
    return eng.flat.data.cpu().numpy().copy()


def _first_norm(torch):
    eng = _engine(torch, max_grad_norm=float("inf"))
    _steps(torch, eng, 1)
    return float(eng.grad_norm())


def test_engine_measuring_only_is_bitwise_the_engine_without_clipping():
    import torch
    plain, measured = _engine(torch), _engine(torch, max_grad_norm=float("inf"))
    assert plain.clip is None and plain.gstruct.clip is None
    a, b = _steps(torch, plain, 3), _steps(torch, measured, 3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert float(measured.clip_coef()) == 1.0
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        plain.grad_norm()
    with pytest.raises(ValueError):
        _engine(torch, max_grad_norm=0.0)


def test_engine_grad_norm_is_the_norm_of_gradients():
    import torch
    eng = _engine(torch, max_grad_norm=float("inf"))
    _steps(torch, eng, 2)
    norm, ref = eng.grad_norm(), eng.gradients().double().norm()
    assert norm.dim() == 0 and norm.is_cuda and norm.data_ptr() == eng.clip.data_ptr()
    assert abs(float(norm) - float(ref)) <= 1e-6 * float(ref), (float(norm), float(ref))


def _eager(torch, max_norm, steps=3):
    model = _make_model(torch).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for step in range(steps):
        model(**_batch(torch, step))["loss"]["nmse"].backward()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)
        opt.step()
        opt.zero_grad()
    return np.concatenate([(torch.view_as_real(p_) if p_.is_complex() else p_).detach().reshape(-1).cpu().numpy() for p_ in model.abi_parameters()])


def _unpadded(eng):
    return np.concatenate([v.detach().cpu().numpy() for v in eng.flat.views])


def test_engine_clipped_against_the_eager_path():
    """Engine and eager autograd path (model(**batch), loss["nmse"].backward(), clip_grad_norm_, torch.optim.Adam) on the same weights,
    batches and threshold, three steps, clipped and unclipped: clipping adds one rounding, not a new error source -- the clipped pair's
    relative nMSE of the parameter deltas stays within a factor 2 of the unclipped pair's."""
    import torch
    start = _unpadded(_engine(torch)).astype(np.float64)
    max_norm = 0.5 * _first_norm(torch)
    res = {}
    for tag, thr in (("unclipped", None), ("clipped", max_norm)):
        eng = _engine(torch, max_grad_norm=thr)
        _steps(torch, eng, 3)
        if thr is not None:
            assert float(eng.clip_coef()) < 1.0
        res[tag] = O.rel_nmse(_unpadded(eng) - start, _eager(torch, thr) - start)
    print("engine vs eager, relative nMSE of the parameter deltas after 3 steps:", res, "max_grad_norm", max_norm)
    assert np.isfinite(res["unclipped"]) and res["unclipped"] > 0.0, res
    assert res["clipped"] <= 2.0 * res["unclipped"], res


def test_engine_clipped_without_deferrals_agrees_with_the_deferred_route():
    """fused_head = False runs flags = 0 (final gradients, cfd_fno_adam_step instead of cfd_adam_flat once clipping is on) -- the same
    parameters after two steps as the deferred route with the same threshold, at the 1e-11 of test_fused_train_step_with_deferred_launches."""
    import torch
    max_norm = 0.5 * _first_norm(torch)
    deferred, plain = _engine(torch, max_grad_norm=max_norm), _engine(torch, max_grad_norm=max_norm, fused_head=False)
    assert deferred.defer_flags == 7 and plain.defer_flags == 0
    a, b = _steps(torch, deferred, 2), _steps(torch, plain, 2)
    assert float(plain.clip_coef()) < 1.0
    assert O.rel_nmse(b, a) < 1e-11
    assert abs(float(plain.grad_norm()) - float(deferred.grad_norm())) <= 1e-5 * float(deferred.grad_norm())


def _rccl_worker(port, max_norm, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_DP_ALWAYS_EXCHANGE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                      NCCL_SOCKET_IFNAME="lo")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        eng = _engine(torch, max_grad_norm=max_norm)
        assert eng.sync.exchange and eng.defer_flags == 0
        flat = _steps(torch, eng, 2)
        q.put((flat, float(eng.grad_norm()), float(eng.clip_coef())))
    finally:
        dist.destroy_process_group()


def test_engine_clipped_data_parallel_step_agrees_with_the_deferred_route():
    """The data-parallel step (a one-rank RCCL group with the exchange forced on, as tests/test_gpu_dp.py runs it): the norm is taken after
    the all-reduce, inside cfd_fno_adam_step with flags = 0."""
    import socket

    import torch
    import torch.multiprocessing as mp
    max_norm = 0.5 * _first_norm(torch)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_rccl_worker, args=(port, max_norm, q))
    proc.start()
    try:
        flat, norm, coef = q.get(timeout=300)
    finally:
        proc.join(timeout=120)
        if proc.is_alive():
            proc.kill()
    assert proc.exitcode == 0
    deferred = _engine(torch, max_grad_norm=max_norm)
    a = _steps(torch, deferred, 2)
    assert coef < 1.0 and O.rel_nmse(flat, a) < 1e-11
    assert abs(norm - float(deferred.grad_norm())) <= 1e-5 * norm


def test_graph_replay_with_clipping_is_bitwise_the_plain_step():
    """train_step_graph twice (the first call captures, both replay) against two train_steps: Adam, and with it the clipping, runs outside
    the graph."""
    import torch
    max_norm = 0.5 * _first_norm(torch)
    plain, graphed = _engine(torch, max_grad_norm=max_norm), _engine(torch, max_grad_norm=max_norm)
    a, b = _steps(torch, plain, 2), _steps(torch, graphed, 2, graph=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert graphed._graph is not None and torch.equal(plain.clip[:2], graphed.clip[:2]) and float(graphed.clip_coef()) < 1.0


# ---- the trainers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [["--fused", "1"], [], ["--unroll_steps", "3"]], ids=["fused", "eager", "unroll3"])
def test_train_auto_max_grad_norm(tmp_path, capsys, extra):
    """train_auto --max_grad_norm on synthetic data, two epochs: the usual artefacts, a finite and falling loss, grad_norm in the log line."""
    import torch

    from cfdbench_amd.harness.args import Args, is_args_valid
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir, load_json
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train

    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--fno_hidden_dim", "8", "--fno_depth", "2",
                              "--lr", "0.005", "--output_dir", str(tmp_path), "--num_epochs", "2", "--batch_size", "4", "--eval_batch_size", "4",
                              "--eval_interval", "1", "--log_interval", "5", "--plot_interval", "0", "--max_grad_norm", "0.5", *extra])
    is_args_valid(args)
    out = get_output_dir(args, is_auto=True)
    tr = SyntheticAutoDataset(n_cases=6, n_frames=6, height=32, width=32, seed=0)
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    torch.manual_seed(0)
    model = init_model(args).cuda()
    losses = train(model, tr, dev, out, num_epochs=2, lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma, batch_size=4,
                   eval_batch_size=4, log_interval=5, eval_interval=1, plot_interval=0, fused=bool(args.fused), unroll_steps=args.unroll_steps,
                   max_grad_norm=args.max_grad_norm)
    assert len(losses) >= 10 and np.all(np.isfinite(losses))
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), "training with clipping does not reduce the loss"
    for ep in (0, 1):
        d = out / f"ckpt-{ep}"
        assert (d / "model.pt").exists() and (d / "dev_scores.json").exists() and (d / "train_loss.json").exists()
        assert set(load_json(d / "scores.json")) == {"ep", "train_loss", "dev_loss", "time"}
    assert (out / "train_state.pt").exists() and (out / "train_losses.json").exists()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "'nmse'" in ln]
    assert lines and all("'grad_norm'" in ln for ln in lines), lines
    assert all(np.isfinite(float(ln.split("'grad_norm': '")[1].split("'")[0])) for ln in lines)
