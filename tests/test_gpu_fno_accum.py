"""MI355X: gradient accumulation over micro-batches in the fused FNO step -- the C-ABI rows of tests/test_emul_fno_accum.py on the device,
FnoTrainEngine.accumulate / apply_accumulated against the eager autograd path ((nmse / 3).backward() x 3 + torch.optim.Adam), with
clipping, under a one-rank RCCL group, and train(fused=True, gradient_accumulation_steps=2)."""
import os

import numpy as np
import pytest

from oracle import fno_oracle as O
from oracle import synth
from tests import accum_checks as AC

pytestmark = pytest.mark.gpu

C, L, P, H, W, B = 20, 2, 5, 64, 64, 4
N_MICRO, N_STEPS = 3, 2


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
@pytest.mark.parametrize("name", list(AC.CASES))
def test_init_with_scale_one_copies_the_gradient_bit_for_bit(be, name):
    AC.check_init_exact(be, name)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_init_finishes_the_deferred_work_and_touches_nothing_else(be, name):
    AC.check_init_deferred(be, name)


@pytest.mark.parametrize("name", list(AC.CASES))
def test_sum_over_micro_batches_then_adam_on_the_accumulator(be, name):
    AC.check_sum_and_adam(be, name)


def test_misaligned_placement_gives_the_aligned_bits(be):
    AC.check_misaligned_gives_the_aligned_bits(be)


def test_refusals_before_any_launch(be):
    got = AC.check_refusals(be)
    assert got == {k: (-1, True) for k in ("init_alone", "null_param", "null_grad")}, got


def test_empty_buffer_launches_nothing(be):
    assert AC.check_empty(be)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _make_model(torch):
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    params = synth.make_fno_params(401, C, L, 12, 12, P, spectral_gain=4.0)
    m = Fno2d(2, 2, P, loss_name_to_fn("nmse"), L, 12, 12, C).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return m


def _batch(torch, i):
    b = synth.make_batch(411 + i, B, H, W, P, border_mask=True)
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in b.items()}


def _engine(torch, **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    return FnoTrainEngine(_make_model(torch), lr=1e-3, loss_name="nmse", **kw)


def _accumulated_steps(torch, eng):
    """N_STEPS optimiser steps of N_MICRO micro-batches each; returns the grad_norm() of every step where the engine clips."""
    norms = []
    for step in range(N_STEPS):
        for k in range(N_MICRO):
            b = _batch(torch, step * N_MICRO + k)
            eng.accumulate(b["inputs"], b["label"], b["case_params"], b["mask"], weight=1.0 / N_MICRO, first=k == 0)
        eng.apply_accumulated()
        if eng.clip is not None:
            norms.append(float(eng.grad_norm()))
    torch.cuda.synchronize()
    return norms


def _eager(torch, max_norm=None):
    model = _make_model(torch).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    norms = []
    for step in range(N_STEPS):
        for k in range(N_MICRO):
            (model(**_batch(torch, step * N_MICRO + k))["loss"]["nmse"] / N_MICRO).backward()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm)))
        opt.step()
        opt.zero_grad()
    return model, norms


def _tensors(model):
    import torch
    return {k: (torch.view_as_real(v) if v.is_complex() else v).detach().cpu().numpy() for k, v in model.state_dict().items()}


def test_engine_accumulation_against_the_eager_path():
    """Two optimiser steps of three micro-batches against autograd (nmse / 3).backward() x 3 + torch.optim.Adam: every parameter within the
    1e-9 of test_fused_and_autograd_paths_agree; an engine that never accumulates holds no accumulator."""
    import torch
    eng = _engine(torch)
    assert eng.accum is None and eng.defer_flags == 7
    _accumulated_steps(torch, eng)
    assert eng.step_count == N_STEPS and eng.accum is not None and eng.gradients() is eng.accum
    twin, _ = _eager(torch)
    ref = _tensors(twin)
    for k, v in _tensors(eng.model).items():
        err = O.rel_nmse(v, ref[k])
        assert err < 1e-9, (k, err)


def test_engine_accumulation_with_clipping_reports_the_norm_of_the_accumulated_gradient():
    """max_grad_norm: grad_norm() of every step against clip_grad_norm_'s return value on the twin.  Bound: both sides hold each
    micro-batch's gradient to a relative nMSE of 1e-11 against fp64, i.e. 3.2e-6 relative per side; the norm of their mean differs by no
    more than that per side, and torch takes its norm in fp32: 1e-5."""
    import torch
    probe = _engine(torch, max_grad_norm=float("inf"))
    first, last = _accumulated_steps(torch, probe)
    assert abs(last - float(probe.gradients().double().norm())) <= 1e-6 * last  # (gradients(): the last step's accumulator)
    max_norm = 0.5 * first
    eng = _engine(torch, max_grad_norm=max_norm)
    norms = _accumulated_steps(torch, eng)
    assert float(eng.clip_coef()) < 1.0
    twin, ref_norms = _eager(torch, max_norm)
    print("grad_norm engine", norms, "twin", ref_norms)
    for a, b in zip(norms, ref_norms):
        assert abs(a - b) <= 1e-5 * b, (norms, ref_norms)
    ref = _tensors(twin)
    print("clipped, parameters against the twin:", {k: O.rel_nmse(v, ref[k]) for k, v in _tensors(eng.model).items()})


def test_engine_accumulation_misuse_raises():
    import torch
    eng = _engine(torch)
    b = _batch(torch, 0)
    args = (b["inputs"], b["label"], b["case_params"], b["mask"])
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        eng.apply_accumulated()
    with pytest.raises(RuntimeError, match="first=False"):
        eng.accumulate(*args, weight=0.5, first=False)
    eng.accumulate(*args, weight=0.5, first=True)
    with pytest.raises(RuntimeError, match="accumulation group is open"):
        eng.train_step(*args)
    with pytest.raises(RuntimeError, match="accumulation group is open"):
        eng.optimizer_step()
    eng.accumulate(*args, weight=0.5, first=False)
    eng.apply_accumulated()
    with pytest.raises(RuntimeError, match="nothing accumulated"):
        eng.apply_accumulated()
    eng.train_step(*args)  # (a closed group leaves the plain step as it was)
    assert eng.step_count == 2 and eng.gradients() is not eng.accum
    torch.cuda.synchronize()


def test_engine_accumulation_with_bf16_activation_storage():
    """act_dtype passes through: the accumulated step on bf16-stored activations equals a plain train_step on the same single micro-batch
    with weight 1 to fp32 round-off of the scale (same kernels, the normaliser applied by the accumulate call instead of Adam)."""
    import torch
    a, b_ = _engine(torch, act_dtype="bf16"), _engine(torch, act_dtype="bf16")
    b = _batch(torch, 0)
    args = (b["inputs"], b["label"], b["case_params"], b["mask"])
    a.train_step(*args)
    b_.accumulate(*args, weight=1.0, first=True)
    b_.apply_accumulated()
    torch.cuda.synchronize()
    # Adam's first step is lr * g / (|g| + eps): compare the first moments, which carry the gradient itself
    assert O.rel_nmse(b_.exp_avg.cpu().numpy(), a.exp_avg.cpu().numpy()) < 1e-13


def _rccl_worker(port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_DP_ALWAYS_EXCHANGE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                      NCCL_SOCKET_IFNAME="lo")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        eng = _engine(torch)
        assert eng.sync.exchange and eng.defer_flags == 0
        _accumulated_steps(torch, eng)
        q.put(eng.flat.data.cpu().numpy().copy())
    finally:
        dist.destroy_process_group()


def test_engine_accumulation_over_a_one_rank_rccl_group():
    """The data-parallel accumulated step (a one-rank RCCL group with the exchange forced on, as tests/test_gpu_dp.py runs it): one
    all-reduce of the accumulator per optimiser step, passes without deferrals -- within 1e-9 of the single-process run."""
    import socket

    import torch
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    proc = ctx.Process(target=_rccl_worker, args=(port, q))
    proc.start()
    try:
        flat = q.get(timeout=300)
    finally:
        proc.join(timeout=120)
        if proc.is_alive():
            proc.kill()
    assert proc.exitcode == 0
    eng = _engine(torch)
    _accumulated_steps(torch, eng)
    assert O.rel_nmse(flat, eng.flat.data.cpu().numpy()) < 1e-9


# ---- the trainer -----------------------------------------------------------------------------------------------------------------
def test_train_fused_with_accumulation_equals_the_loop_by_hand(tmp_path):
    """train(fused=True, gradient_accumulation_steps=2) over five batches (groups of 2, 2, 1) against accumulate / apply_accumulated by
    hand on the same initial weights and shuffle: the same bits; one loss entry per micro-batch."""
    import torch
    from torch.utils.data import DataLoader

    from cfdbench_amd.engine import FnoTrainEngine
    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import collate_fn, train
    args = Args(model="fno", data_name="cavity_bc", loss_name="nmse", fno_hidden_dim=8, fno_depth=2, lr=1e-3, output_dir=str(tmp_path),
                batch_size=4, plot_interval=0, fused=1, fused_accumulation_steps=2)
    tr = SyntheticAutoDataset(n_cases=4, n_frames=6, height=64, width=64, seed=0)
    dev = SyntheticAutoDataset(n_cases=2, n_frames=3, height=64, width=64, seed=1)
    assert len(DataLoader(tr, batch_size=4)) == 5
    torch.manual_seed(0)
    m1 = init_model(args).cuda()
    losses = train(m1, tr, dev, tmp_path / "run", num_epochs=1, lr=1e-3, batch_size=4, eval_interval=10, plot_interval=0, fused=True,
                   gradient_accumulation_steps=2)
    assert len(losses) == 5 and np.all(np.isfinite(losses))
    torch.manual_seed(0)
    m2 = init_model(args).cuda()
    eng = FnoTrainEngine(m2, lr=1e-3, loss_name="nmse")
    m2.train()
    by_hand = []
    for step, batch in enumerate(DataLoader(tr, batch_size=4, shuffle=True, collate_fn=collate_fn)):
        sums = eng.accumulate(batch["inputs"], batch["label"], batch["case_params"], batch["mask"], weight=1.0 if step == 4 else 0.5,
                              first=step % 2 == 0)
        by_hand.append(float(sums[0] / sums[2]))
        if step in (1, 3, 4):
            eng.apply_accumulated()
    assert eng.step_count == 3
    assert losses == by_hand
    for (k, a), b in zip(m1.state_dict().items(), m2.state_dict().values()):
        assert torch.equal(a, b), k
