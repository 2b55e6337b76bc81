"""MI355X: skipping non-finite steps inside cfd_fno_adam_step (CFD_STEP_SKIP_NONFINITE) -- the C-ABI rows of
tests/test_emul_fno_guard.py on the device (tests/guard_checks.py), FnoTrainEngine(skip_nonfinite=True) on every route that ends in an
optimiser call (train_step, graph replay, AdamW on a frozen subset with clipping, accumulation groups, rollout windows, two data-parallel
ranks, checkpointed state), and train_auto --fused 1 --skip_nonfinite 1 on data with one NaN frame."""
import os
import socket

import numpy as np
import pytest

from oracle import synth
from tests import guard_checks as GC

pytestmark = pytest.mark.gpu

C, L, P, H, W, B, M = 8, 1, 5, 32, 32, 2, 8


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
@pytest.mark.parametrize("ns", [GC.FLAT_NS, (GC.FLAT_N_CAPPED,)], ids=["small", "capped_records"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_a_nonfinite_gradient_writes_nothing(be, misalign, ns):
    """(a); `capped_records`: n = 300 003, where k_gradsq runs at its cap of 256 workgroups."""
    assert GC.check_skip_flat(be, misalign, ns) == 4 * sum(3 * len(GC.bad_positions(n)) + 1 for n in ns)


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_finite_gradients_are_bitwise_the_call_without_the_bit(be, misalign):
    GC.check_finite_is_bitwise(be, misalign, GC.FLAT_NS + (GC.FLAT_N_CAPPED,))


@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_finite_nonfinite_finite_follows_the_rule_at_t_1_and_3(be, misalign):
    GC.check_sequence(be, misalign)


@pytest.mark.parametrize("kind", ["inf", "zero"], ids=["inf_in_label", "zero_label"])
def test_whole_steps_with_deferrals(be, kind):
    GC.check_deferred_steps(be, kind)


def test_the_bit_is_ignored_with_accumulate_and_skips_the_group_afterwards(be):
    GC.check_accumulate_ignores_the_bit(be)


def test_refusal_and_empty_buffer(be):
    assert GC.check_refusal(be) == (-1, True)
    assert GC.check_empty(be) == ([0.0, 1.0], (4.0, 3.0), True)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _make_model(torch, freeze=()):
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    m = Fno2d(2, 2, P, loss_name_to_fn("nmse"), L, M, M, C).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.make_fno_params(601, C, L, M, M, P, spectral_gain=4.0).items()})
    for k, p_ in m.named_parameters():
        if any(k.startswith(q + ".") for q in freeze):
            p_.requires_grad_(False)
    return m


def _engine(torch, freeze=(), **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    return FnoTrainEngine(_make_model(torch, freeze), lr=1e-3, loss_name="nmse", **kw)


def _batch(torch, i, bad=False, rank=0):
    """Batch i; `bad`: one NaN in its label."""
    b = synth.make_batch(611 + i + 100 * rank, B, H, W, P, border_mask=True)
    if bad:
        b["label"][0, 0, H // 2, W // 2] = np.nan
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in b.items()}


def _state(eng):
    """Copies of the flat parameters and both moments, as bit patterns."""
    import torch
    return [t.detach().clone().view(torch.int32) for t in (eng.flat.data, eng.exp_avg, eng.exp_avg_sq)]


def _same_state(torch, a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _step(torch, eng, route, i, bad=False):
    """One optimiser step of `route` on batch i (and its neighbours): the bad batch is the second of its group / the window's last label."""
    b = _batch(torch, i, bad and route not in ("group", "window"))
    if route == "graph":
        eng.train_step_graph(b["inputs"], b["label"], b["case_params"], b["mask"])
    elif route == "group":
        b2 = _batch(torch, i + 50, bad)
        for k, x in enumerate((b, b2)):
            eng.accumulate(x["inputs"], x["label"], x["case_params"], x["mask"], weight=0.5, first=k == 0)
        eng.apply_accumulated()
    elif route == "window":
        b2 = _batch(torch, i + 50, bad)
        eng.train_window(b["inputs"], [b["label"], b2["label"]], b["case_params"], b["mask"], detach=False)
    else:
        eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])


ROUTES = {"train_step": {}, "graph": {}, "adamw_frozen_clipped": dict(freeze=("blocks",), optimizer="adamw", weight_decay=0.1, max_grad_norm=0.5),
          "group": {}, "window": {}}


@pytest.mark.parametrize("route", list(ROUTES))
def test_engine_skips_the_bad_step_and_trains_on(route):
    """good / NaN label / good: the flat parameters and both moments keep their bits across the bad step, skipped_steps() == 1, the
    parameters are finite afterwards and the step count ran on.  The same sequence on an engine without the guard ends non-finite."""
    import torch
    kw = ROUTES[route]
    eng = _engine(torch, skip_nonfinite=True, **kw)
    assert eng.clip is not None and (eng.max_grad_norm is None) == ("max_grad_norm" not in kw)
    _step(torch, eng, route, 0)
    s1 = _state(eng)
    assert not bool(eng.last_step_skipped()) and float(eng.skipped_steps()) == 0.0 and float(eng.clip_coef()) > 0.0
    _step(torch, eng, route, 1, bad=True)
    assert _same_state(torch, _state(eng), s1), f"{route}: the skipped step changed parameters or moments"
    assert bool(eng.last_step_skipped()) and float(eng.skipped_steps()) == 1.0 == float(eng.consecutive_skipped())
    assert not np.isfinite(float(eng.grad_norm())) and float(eng.clip_coef()) == 0.0
    _step(torch, eng, route, 2)
    torch.cuda.synchronize()
    assert not _same_state(torch, _state(eng), s1) and bool(torch.isfinite(eng.flat.data).all()) and bool(torch.isfinite(eng.exp_avg_sq).all())
    assert float(eng.skipped_steps()) == 1.0 and float(eng.consecutive_skipped()) == 0.0 and eng.step_count == 3
    plain = _engine(torch, **kw)
    for i, bad in ((0, False), (1, True), (2, False)):
        _step(torch, plain, route, i, bad)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(plain.flat.data).all()), f"{route}: the unguarded engine survived the NaN batch"


def test_guarded_engine_without_skips_is_bitwise_the_unguarded_one():
    """Three clean steps: the guard costs a launch, not a bit -- against the engine that measures the norm (max_grad_norm = inf) and against
    the plain one."""
    import torch
    engines = [_engine(torch, skip_nonfinite=True), _engine(torch, max_grad_norm=float("inf")), _engine(torch)]
    for eng in engines:
        for i in range(3):
            _step(torch, eng, "train_step", i)
    torch.cuda.synchronize()
    for other in engines[1:]:
        assert _same_state(torch, _state(engines[0]), _state(other))
    assert float(engines[0].skipped_steps()) == 0.0


def test_state_dict_round_trip_keeps_the_count():
    import torch
    a = _engine(torch, skip_nonfinite=True)
    for i, bad in ((0, False), (1, True)):
        _step(torch, a, "train_step", i, bad)
    state = a.state_dict()
    assert state["skipped_steps"] == 1 and isinstance(state["skipped_steps"], int) and state["step_count"] == 2
    b = _engine(torch, skip_nonfinite=True)
    b.model.load_state_dict(a.model.state_dict())
    b.load_state_dict(state)
    assert float(b.skipped_steps()) == 1.0 and float(b.consecutive_skipped()) == 0.0
    for eng in (a, b):
        _step(torch, eng, "train_step", 2)
    torch.cuda.synchronize()
    assert _same_state(torch, _state(a), _state(b)) and float(b.skipped_steps()) == 1.0
    # an engine without the guard writes and reads the states it always did; a state without the key means 0
    plain = _engine(torch)
    assert "skipped_steps" not in plain.state_dict()
    plain.load_state_dict(state)
    b.load_state_dict(plain.state_dict())
    assert float(b.skipped_steps()) == 0.0
    with pytest.raises(RuntimeError, match="skip_nonfinite"):
        plain.skipped_steps()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dp_worker(rank, world, port, overlap, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = _engine(torch, skip_nonfinite=True, overlap=overlap)
        assert eng.sync.world == world and eng.sync.exchange
        states, skipped = [], []
        for i, bad in ((0, False), (1, True), (2, False)):
            b = _batch(torch, i, bad and rank == 0, rank)  # only rank 0's batch is bad
            eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
            torch.cuda.synchronize()
            states.append([t.cpu().numpy() for t in _state(eng)])
            skipped.append((bool(eng.last_step_skipped()), float(eng.skipped_steps())))
        q.put((rank, states, skipped))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("overlap", [True, False], ids=["overlapped", "single_exchange"])
def test_two_ranks_skip_together(overlap):
    """Two processes on one GPU over a host-staged group (tests/test_gpu_dp.py's set-up): only rank 0's second batch is bad; both ranks
    decide on the reduced gradient, skip that step, and their parameters and moments stay identical."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, overlap, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=300) for _ in procs), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    (_, s0, k0), (_, s1, k1) = res
    assert k0 == k1 == [(False, 0.0), (True, 1.0), (False, 1.0)], (k0, k1)
    for step in range(3):
        for a, b in zip(s0[step], s1[step]):
            assert np.array_equal(a, b), f"step {step + 1}: the replicas diverged"
    for a, b in zip(s0[0], s0[1]):
        assert np.array_equal(a, b), "the skipped step changed rank 0's state"
    assert not np.array_equal(s0[2][0], s0[1][0]) and np.isfinite(s0[2][0].view(np.float32)).all()


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def test_train_auto_survives_a_nan_frame(tmp_path, capsys):
    """train_auto --fused 1 --skip_nonfinite 1 on synthetic data with one NaN frame (one item's label, the next item's input): the run
    finishes, model.pt is finite, the skipped count in train_state.pt lies between 1 and 2 per epoch, the loss history holds applied steps
    only.  The same run without the flag ends with non-finite weights."""
    import torch

    from cfdbench_amd.harness.args import Args, is_args_valid
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train

    epochs = 2
    tr = SyntheticAutoDataset(n_cases=4, n_frames=5, height=32, width=32, seed=0)
    tr.all_features[1][2, 0, 16, 16] = np.nan
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    finite = {}
    for flag in (1, 0):
        torch.manual_seed(3)
        args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--fno_hidden_dim", "8", "--fno_depth", "1",
                                  "--lr", "0.005", "--output_dir", str(tmp_path / f"flag{flag}"), "--num_epochs", str(epochs), "--batch_size", "4",
                                  "--eval_batch_size", "4", "--eval_interval", "1", "--log_interval", "2", "--plot_interval", "0", "--fused", "1",
                                  "--skip_nonfinite", str(flag)])
        is_args_valid(args)
        out = get_output_dir(args, is_auto=True)
        model = init_model(args).cuda()
        losses = train(model, tr, dev, out, num_epochs=epochs, lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma, batch_size=4,
                       eval_batch_size=4, log_interval=2, eval_interval=1, plot_interval=0, fused=True, skip_nonfinite=bool(flag),
                       max_consecutive_skips=args.max_consecutive_skips)
        ckpt = torch.load(out / f"ckpt-{epochs - 1}" / "model.pt", map_location="cpu")
        finite[flag] = all(bool(torch.isfinite(torch.view_as_real(v) if v.is_complex() else v).all()) for v in ckpt.values())
        state = torch.load(out / "train_state.pt", map_location="cpu", weights_only=False)
        if flag:
            n = state["skipped_steps"]
            assert 1 <= n <= 2 * epochs and state["optimizer"]["skipped_steps"] == n
            assert len(losses) == epochs * 4 - n and np.all(np.isfinite(losses))
            text = capsys.readouterr().out
            assert "'skipped': " in text and "'nmse_applied': " in text
        else:
            assert "skipped_steps" not in state and "skipped_steps" not in state["optimizer"]
    assert finite == {1: True, 0: False}, finite


def test_train_auto_stops_a_run_that_skips_everything(tmp_path):
    """Every label is NaN: with --max_consecutive_skips 3 the fused run raises at its first log interval past three skips, naming count and
    step, before any checkpoint is written."""
    import torch

    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train
    tr = SyntheticAutoDataset(n_cases=4, n_frames=5, height=32, width=32, seed=0)
    for f in tr.all_features:
        f[:, 0, 16, 16] = np.nan
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    torch.manual_seed(3)
    model = _make_model(torch)
    with pytest.raises(RuntimeError, match=r"4 optimiser steps in a row.*epoch 0, step 3"):
        train(model, tr, dev, tmp_path / "run", num_epochs=2, batch_size=4, eval_batch_size=4, log_interval=2, eval_interval=1, plot_interval=0,
              fused=True, skip_nonfinite=True, max_consecutive_skips=3)
    assert not (tmp_path / "run" / "train_state.pt").exists()
    assert bool(torch.isfinite(model.abi_parameters()[0]).all())
