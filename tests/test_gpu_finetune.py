"""MI355X: fine-tuning on the fused FNO step -- the C-ABI rows of tests/test_emul_finetune.py on the device (decoupled weight decay inside
cfd_fno_adam_step, whole steps over a trainable subset), FnoTrainEngine on models with frozen parameters (frozen tensors bitwise untouched,
the trained ones against the fp64 oracle and the eager autograd path, the backward-phase calls it issues, accumulation, rollout windows,
clipping, graph replay, checkpointed state), FnoTrainEngine(optimizer="adamw") against torch.optim.AdamW, and train_auto --train_only
--optimizer adamw --init_from."""
import os

import numpy as np
import pytest

from oracle import fno_oracle as O
from oracle import synth
from tests import finetune_checks as FT
from tests import fno_checks as F

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
@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_adamw_bit_on_flat_buffers(be, misalign, clip):
    FT.check_adamw_flat(be, misalign, clip)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "misaligned"])
def test_adamw_bit_beside_the_deferral_flags(be, misalign, clip):
    FT.check_adamw_deferred(be, misalign, clip)


@pytest.mark.parametrize("subset", ["head", "last_block_head", "fc0_head", "spectral"])
@pytest.mark.parametrize("shape", list(FT.SHAPES))
def test_frozen_subset_steps(be, shape, subset):
    FT.check_subset(be, shape, subset)


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _params():
    return synth.make_fno_params(501, C, L, 12, 12, P, spectral_gain=4.0)


def _make_model(torch, freeze=()):
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    m = Fno2d(2, 2, P, loss_name_to_fn("nmse"), L, 12, 12, C).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in _params().items()})
    for k, p_ in m.named_parameters():
        if any(k == q or k.startswith(q + ".") for q in freeze):
            p_.requires_grad_(False)
    return m


def _host_batch(i):
    return synth.make_batch(511 + i, B, H, W, P, border_mask=True)


def _batch(torch, i):
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in _host_batch(i).items()}


def _engine(torch, freeze=(), **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    return FnoTrainEngine(_make_model(torch, freeze), lr=1e-3, loss_name="nmse", **kw)


def _tensors(model):
    import torch
    return {k: (torch.view_as_real(v) if v.is_complex() else v).detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _steps(torch, eng, n, graph=False):
    for i in range(n):
        b = _batch(torch, i)
        (eng.train_step_graph if graph else eng.train_step)(b["inputs"], b["label"], b["case_params"], b["mask"])
    torch.cuda.synchronize()


def _assert_frozen_bitwise(model, before, frozen_prefixes):
    after = _tensors(model)
    hit = 0
    for k in before:
        if any(k.startswith(q + ".") for q in frozen_prefixes):
            assert np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)), f"the frozen tensor {k} changed"
            hit += 1
        else:
            assert not np.array_equal(after[k], before[k]), f"the trainable tensor {k} did not move"
    assert hit
    return after


class _Counting:
    """Stands in for the engine's bound C ABI: counts the entry points called, then calls them."""

    def __init__(self, api):
        self._api, self.names = api, []

    def call(self, name, *a):
        self.names.append(name)
        return self._api.call(name, *a)

    def __getattr__(self, k):
        return getattr(self._api, k)


def test_frozen_blocks_stay_bitwise_and_the_rest_follows_the_oracle():
    """model.blocks.requires_grad_(False), three train_steps: the blocks keep their bits (the engine of before this feature stepped them),
    fc0 and the head follow three fp64 oracle steps -- first on the Adam bound of the C-ABI rows."""
    import torch
    eng = _engine(torch, freeze=("blocks",))
    assert not eng.all_trainable and eng.last_phase == L + 1 and eng.defer_flags == 7
    assert eng.trainable_names == ["fc0.weight", "fc0.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    assert eng.flat.numel == eng.exp_avg.numel() == sum((p_.numel() + 3) // 4 * 4 for p_ in eng.model.parameters() if p_.requires_grad)
    before = _tensors(eng.model)
    _steps(torch, eng, 3)
    after = _assert_frozen_bitwise(eng.model, before, ("blocks",))
    _g1, p64 = FT.oracle_train(_params(), [_host_batch(i) for i in range(3)], L, eng.trainable_names)
    got = np.concatenate([after[k].reshape(-1).astype(np.float64) - before[k].reshape(-1) for k in eng.trainable_names])
    want = np.concatenate([F.flat_view(p64[k]) - before[k].reshape(-1).astype(np.float64) for k in eng.trainable_names])
    err = O.rel_nmse(got, want)
    print("frozen blocks, parameter deltas of three steps against the oracle:", err)
    assert err <= FT.ADAM_TOL, err


@pytest.mark.parametrize("freeze,phases", [(("fc0", "blocks"), 0), (("fc0", "blocks.0"), 1), (("blocks",), L + 1), (("fc0", "fc1", "fc2"), L),
                                           (("fc0", "blocks.1", "fc1", "fc2"), L), ((), L + 1)],
                         ids=["head", "last_block_head", "fc0_head", "blocks", "block0", "all"])
def test_backward_phase_calls_follow_the_rule(freeze, phases):
    """The head-only engine issues no cfd_fno_backward_phase* call at all: forward with the one-pass head, then the optimiser.  The others
    stop behind the phase of their shallowest trainable tensor (last_backward_phase)."""
    import torch
    from cfdbench_amd.engine import last_backward_phase
    eng = _engine(torch, freeze=freeze)
    mask = [p_.requires_grad for p_ in eng.model.abi_parameters()]
    assert eng.last_phase == last_backward_phase(mask, L) == phases
    eng.api = _Counting(eng.api)
    before = _tensors(eng.model)
    _steps(torch, eng, 2)
    names = eng.api.names
    assert sum(n.startswith("cfd_fno_backward") for n in names) == 2 * phases, names
    assert names.count("cfd_fno_forward_train_f") == 2 and sum(n in ("cfd_fno_adam_step", "cfd_adam_flat") for n in names) == 2
    assert len(names) == 2 * (2 + phases), names
    if freeze:
        _assert_frozen_bitwise(eng.model, before, freeze)


def _twin_steps(torch, freeze, n, opt_cls=None, **opt_kw):
    model = _make_model(torch, freeze).train()
    opt = (opt_cls or torch.optim.Adam)([p_ for p_ in model.parameters() if p_.requires_grad], lr=1e-3, **opt_kw)
    for i in range(n):
        model(**_batch(torch, i))["loss"]["nmse"].backward()
        opt.step()
        opt.zero_grad()
    return model


def _assert_close(model, twin, tol=1e-9, what=""):
    ref = _tensors(twin)
    errs = {k: O.rel_nmse(v, ref[k]) for k, v in _tensors(model).items()}
    print(what, "parameters against the twin:", errs)
    for k, e in errs.items():
        assert e < tol, (what, k, e)


def test_frozen_engine_against_the_eager_path_on_every_route():
    """Two steps of last block + head against autograd with the same requires_grad flags (the 1e-9 of test_fused_and_autograd_paths_agree):
    the plain step, the two-pass head (fused_head=False: the phase entries instead of cfd_fno_backward), and graph replay, which is
    bitwise the plain step."""
    import torch
    freeze = ("fc0", "blocks.0")
    twin = _twin_steps(torch, freeze, 2)
    plain = _engine(torch, freeze)
    _steps(torch, plain, 2)
    _assert_close(plain.model, twin, what="fused head")
    two_pass = _engine(torch, freeze, fused_head=False)
    assert two_pass.defer_flags == 0
    two_pass.api = _Counting(two_pass.api)
    _steps(torch, two_pass, 2)
    assert "cfd_fno_backward" not in two_pass.api.names and two_pass.api.names.count("cfd_fno_backward_phase_ex") == 2 * 2
    _assert_close(two_pass.model, twin, what="two-pass head")
    graphed = _engine(torch, freeze)
    _steps(torch, graphed, 2, graph=True)
    assert graphed._graph is not None
    assert np.array_equal(graphed.flat.data.cpu().numpy().view(np.uint32), plain.flat.data.cpu().numpy().view(np.uint32))


def test_accumulation_and_windows_with_clipping_on_a_frozen_engine():
    """accumulate x 2 + apply_accumulated, then train_window(K = 2) with the full gradient and with detach, all with a clipping threshold
    that bites, on last block + head: frozen tensors bitwise untouched; grad_norm() is clip_grad_norm_'s over the trainable parameters of
    the eager twin (1e-5: tests/test_gpu_fno_accum.py states the bound), and the parameters follow the twin."""
    import torch
    from cfdbench_amd.unroll import unrolled_loss
    freeze = ("fc0", "blocks.0")
    probe = _engine(torch, freeze, max_grad_norm=float("inf"))
    _steps(torch, probe, 1)
    max_norm = 0.5 * float(probe.grad_norm())
    assert abs(float(probe.grad_norm()) - float(probe.gradients().double().norm())) <= 1e-6 * float(probe.grad_norm())
    assert probe.gradients().numel() == probe.flat.numel  # (the compact gradient: the norm is the trainable subset's)

    eng = _engine(torch, freeze, max_grad_norm=max_norm)
    twin = _make_model(torch, freeze).train()
    opt = torch.optim.Adam([p_ for p_ in twin.parameters() if p_.requires_grad], lr=1e-3)
    before = _tensors(eng.model)
    norms, ref_norms = [], []

    def twin_step(loss):
        loss.backward()
        ref_norms.append(float(torch.nn.utils.clip_grad_norm_([p_ for p_ in twin.parameters() if p_.requires_grad], max_norm)))
        opt.step()
        opt.zero_grad()

    # one group of two micro-batches
    bs = [_batch(torch, i) for i in range(2)]
    for k, b in enumerate(bs):
        eng.accumulate(b["inputs"], b["label"], b["case_params"], b["mask"], weight=0.5, first=k == 0)
    eng.apply_accumulated()
    norms.append(float(eng.grad_norm()))
    twin_step(sum(twin(**b)["loss"]["nmse"] for b in bs) / 2)
    # two windows of two steps: the full gradient (step 2 hands back d loss / d inputs: every phase), then the truncated one
    for i, detach in ((2, False), (3, True)):
        b, b2 = _batch(torch, i), _batch(torch, i + 10)
        labels = [b["label"], b2["label"]]
        eng.train_window(b["inputs"], labels, b["case_params"], b["mask"], detach=detach)
        norms.append(float(eng.grad_norm()))
        twin_step(unrolled_loss(twin, b["inputs"], labels, b["case_params"], b["mask"], detach=detach)[0])
    torch.cuda.synchronize()
    assert float(eng.clip_coef()) < 1.0
    _assert_frozen_bitwise(eng.model, before, freeze)
    print("grad_norm engine", norms, "twin", ref_norms)
    for a, b_ in zip(norms, ref_norms):
        assert abs(a - b_) <= 1e-5 * b_, (norms, ref_norms)
    _assert_close(eng.model, twin, what="accumulate + windows, clipped")


def test_state_dict_round_trip_and_mismatch():
    import torch
    freeze = ("fc0", "blocks")
    a = _engine(torch, freeze)
    _steps(torch, a, 2)
    state = a.state_dict()
    assert state["trainable"] == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"] and state["numel"] == a.flat.numel
    b = _engine(torch, freeze)
    b.model.load_state_dict(a.model.state_dict())
    b.load_state_dict(state)
    for eng in (a, b):
        bt = _batch(torch, 2)
        eng.train_step(bt["inputs"], bt["label"], bt["case_params"], bt["mask"])
    torch.cuda.synchronize()
    assert torch.equal(a.flat.data, b.flat.data) and torch.equal(a.exp_avg_sq, b.exp_avg_sq) and b.step_count == 3
    with pytest.raises(ValueError, match="trainable"):
        _engine(torch, ("blocks",)).load_state_dict(state)
    with pytest.raises(ValueError, match="trainable"):
        _engine(torch).load_state_dict(state)
    full = _engine(torch)
    old = {k: v for k, v in full.state_dict().items() if k != "trainable"}  # a state written before the key existed
    full.load_state_dict(old)
    with pytest.raises(ValueError, match="trainable"):
        a.load_state_dict(old)


def test_trainable_argument_and_refusals():
    import torch
    from cfdbench_amd.engine import FnoTrainEngine
    eng = FnoTrainEngine(_make_model(torch), lr=1e-3, trainable={"fc1", "fc2"})
    assert eng.last_phase == 0 and eng.defer_flags == 1 and [k for k, p_ in eng.model.named_parameters() if p_.requires_grad] == eng.trainable_names
    over = FnoTrainEngine(_make_model(torch, ("blocks",)), lr=1e-3, trainable={"blocks.1"})  # the argument overrides requires_grad
    assert over.trainable_names == [f"blocks.1.{t}" for t in ("conv0.weights1", "conv0.weights2", "w0.weight", "w0.bias")] and over.defer_flags == 3
    with pytest.raises(ValueError, match="nothing is trainable"):
        FnoTrainEngine(_make_model(torch, ("fc0", "blocks", "fc1", "fc2")), lr=1e-3)
    with pytest.raises(ValueError, match="matches no parameter"):
        FnoTrainEngine(_make_model(torch), lr=1e-3, trainable={"fc9"})
    with pytest.raises(ValueError, match="optimizer"):
        FnoTrainEngine(_make_model(torch), lr=1e-3, optimizer="sgd")
    full = _engine(torch)
    assert full.all_trainable and full.defer_flags == 7 and full.flat.sink is None and full.last_phase == L + 1


@pytest.mark.parametrize("freeze", [(), ("fc0", "blocks.0")], ids=["all", "last_block_head"])
def test_adamw_step_against_torch_adamw(freeze):
    """One AdamW step (weight_decay = 0.1), fused against eager torch.optim.AdamW, at the 1e-9 of the Adam parity tests; the decay alone
    moves a parameter by lr * wd = 1e-4 of itself, 1e-8 in this measure, so an engine that ignored it would miss the bound.  The
    optimiser call is cfd_fno_adam_step, and a second step keeps the parity (the moments are the undecayed gradient's)."""
    import torch
    eng = _engine(torch, freeze, optimizer="adamw", weight_decay=0.1)
    eng.api = _Counting(eng.api)
    _steps(torch, eng, 1)
    _assert_close(eng.model, _twin_steps(torch, freeze, 1, torch.optim.AdamW, weight_decay=0.1), what="adamw, one step")
    plain = _engine(torch, freeze)
    _steps(torch, plain, 1)
    ref = _tensors(plain.model)
    worst = max(O.rel_nmse(v, ref[k]) for k, v in _tensors(eng.model).items() if not any(k.startswith(q + ".") for q in freeze))
    assert worst > 1e-9, worst  # (the decay is visible in this measure)
    b = _batch(torch, 1)
    eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
    torch.cuda.synchronize()
    assert "cfd_adam_flat" not in eng.api.names and eng.api.names.count("cfd_fno_adam_step") == 2
    _assert_close(eng.model, _twin_steps(torch, freeze, 2, torch.optim.AdamW, weight_decay=0.1), what="adamw, two steps")


def _rccl_worker(port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_DP_ALWAYS_EXCHANGE="1", HSA_ENABLE_IPC_MODE_LEGACY="0",
                      NCCL_SOCKET_IFNAME="lo")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        eng = _engine(torch, ("fc0", "blocks.0"))
        assert eng.sync.exchange and eng.overlap and eng.defer_flags == 0 and not eng.all_trainable
        seen = []
        reduce = eng.sync.reduce_slice_async
        eng.sync.reduce_slice_async = lambda flat, a, b: (seen.append((flat.data_ptr(), a, b)), reduce(flat, a, b))[1]
        _steps(torch, eng, 2)
        # one all-reduce of the compact gradient per step, behind the pass (the per-phase exchange is the all-trainable engine's)
        assert seen == [(eng.flat.grad.data_ptr(), 0, eng.flat.numel)] * 2, seen
        q.put(eng.flat.data.cpu().numpy().copy())
    finally:
        dist.destroy_process_group()


def test_frozen_engine_over_a_one_rank_rccl_group():
    """Data-parallel with a frozen subset (a one-rank RCCL group with the exchange forced on, as tests/test_gpu_dp.py runs it): one
    all-reduce of the compact gradient after the pass, passes without deferrals -- within 1e-9 of the single-process run."""
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
    eng = _engine(torch, ("fc0", "blocks.0"))
    _steps(torch, eng, 2)
    assert flat.size == eng.flat.numel and O.rel_nmse(flat, eng.flat.data.cpu().numpy()) < 1e-9


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def test_train_auto_fine_tunes_the_head_from_another_runs_weights(tmp_path, capsys):
    """train_auto --fused 1 --train_only fc1,fc2 --optimizer adamw --init_from on synthetic data, two epochs: the checkpoint's frozen
    tensors are bitwise those of the weights it started from, the head moved, the loss is finite."""
    import torch

    from cfdbench_amd.harness.args import Args, is_args_valid
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import apply_trainable, get_output_dir
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train

    torch.manual_seed(3)
    base = ["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--fno_hidden_dim", "8", "--fno_depth", "2", "--lr", "0.005",
            "--output_dir", str(tmp_path), "--num_epochs", "2", "--batch_size", "4", "--eval_batch_size", "4", "--eval_interval", "1",
            "--log_interval", "5", "--plot_interval", "0"]
    donor = init_model(Args().parse_args(base))
    init = {k: v.detach().clone() for k, v in donor.state_dict().items()}
    torch.save(init, tmp_path / "pretrained.pt")
    args = Args().parse_args(base + ["--fused", "1", "--train_only", "fc1,fc2", "--optimizer", "adamw", "--weight_decay", "0.01",
                                     "--init_from", str(tmp_path / "pretrained.pt")])
    is_args_valid(args)
    out = get_output_dir(args, is_auto=True)
    tr = SyntheticAutoDataset(n_cases=6, n_frames=6, height=32, width=32, seed=0)
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    model = init_model(args).cuda()  # (other weights than the donor's: --init_from must replace them)
    left = apply_trainable(model, args.freeze, args.train_only)
    assert left == ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    losses = train(model, tr, dev, out, num_epochs=2, lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma, batch_size=4,
                   eval_batch_size=4, log_interval=5, eval_interval=1, plot_interval=0, fused=True, optimizer_kind=args.optimizer,
                   weight_decay=args.weight_decay, init_from=args.init_from)
    assert len(losses) >= 10 and np.all(np.isfinite(losses))
    assert "Loading checkpoint from" in capsys.readouterr().out
    ckpt = torch.load(out / "ckpt-1" / "model.pt", map_location="cpu")
    for k, v in init.items():
        same = torch.equal(torch.view_as_real(ckpt[k]) if v.is_complex() else ckpt[k], torch.view_as_real(v) if v.is_complex() else v)
        assert same == (not k.startswith(("fc1.", "fc2."))), k
    state = torch.load(out / "train_state.pt", map_location="cpu", weights_only=False)
    assert state["optimizer"]["trainable"] == left
