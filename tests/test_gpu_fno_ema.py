"""MI355X: the exponential moving average of the weights inside cfd_fno_adam_step_ema -- the C-ABI rows of tests/test_emul_fno_ema.py on
the device (tests/ema_checks.py), and FnoTrainEngine(ema_decay=) on every route that ends in an optimiser call: train_step, warm-up, a
frozen subset, AdamW with clipping, accumulation groups, rollout windows, skipped steps, graph replay, a one-rank data-parallel group,
averaged(), ema_state_dict() and the checkpointed state, and the placements of the new entry's row of the alignment table
(tests/ema_checks.py: register_alignment_row)."""
import os
import socket

import numpy as np
import pytest

from oracle import fno_oracle as O
from oracle import synth
from tests import ema_checks as EC

pytestmark = pytest.mark.gpu
ROW = EC.register_alignment_row()  # (while pytest collects: tests/align_checks.py's table has the new entry's row before any test runs)

# tiny: tests/test_gpu_fno_guard.py's model; deferring: the smallest shape on which the step defers the normaliser and the fc0 rows to the
# optimiser launch (64 x 64, C = 20: the job workgroups of k_adam_f update the average's fc0 ranges)
SHAPES = {"tiny": dict(C=8, L=1, H=32, W=32, M=8), "deferring": dict(C=20, L=2, H=64, W=64, M=12)}
P, B, DECAY, STEPS = 5, 2, 0.9, 5


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
@pytest.mark.parametrize("n", EC.FLAT_NS)
def test_the_average_follows_the_rule(be, n):
    assert EC.check_rule_flat(be, n) <= 1.0


@pytest.mark.parametrize("n", EC.FLAT_NS)
def test_no_other_bit_moves(be, n):
    EC.check_no_other_bit_moves(be, n)


def test_misplaced_buffers_give_the_aligned_bits(be):
    EC.check_misplaced(be, EC.FLAT_NS)


@pytest.mark.parametrize("placement", ["all0", "all4", "all8", "each4"])
def test_row_of_the_alignment_table(be, placement):
    """Every buffer shifted by 4 and by 8 bytes, and each buffer alone -- the average among them -- by 4: the aligned run's bits."""
    from tests import align_checks as A
    assert placement in A.placements(ROW, False)
    A.run_row(be, ROW, placement)


@pytest.mark.parametrize("clip", [False, True], ids=["job_in_adam", "job_in_gradsq"])
def test_the_lifting_layers_rows(be, clip):
    EC.check_stem_rows(be, clip)


def test_a_skipped_step_keeps_the_average(be):
    EC.check_guard(be)


def test_accumulate_ignores_the_average(be):
    EC.check_accumulate_ignores_the_ema(be)


def test_bad_decays_are_refused_before_any_launch_and_empty_buffers_write_nothing(be):
    assert EC.check_bad_decay(be) == {str(d): (-1, True) for d in EC.BAD_DECAYS}
    assert EC.check_empty(be) == (True, [0.0, 1.0])


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _make_model(torch, shape="tiny", freeze=()):
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    s = SHAPES[shape]
    m = Fno2d(2, 2, P, loss_name_to_fn("nmse"), s["L"], s["M"], s["M"], s["C"]).cuda()
    params = synth.make_fno_params(701, s["C"], s["L"], s["M"], s["M"], P, spectral_gain=4.0)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    for k, p_ in m.named_parameters():
        if any(k.startswith(q + ".") for q in freeze):
            p_.requires_grad_(False)
    return m


class _Counting:
    """Stands in for the engine's api: the names of the C calls it makes."""

    def __init__(self, api):
        self._api, self.names = api, []

    def __getattr__(self, name):
        return getattr(self._api, name)

    def call(self, name, *args):
        self.names.append(name)
        return self._api.call(name, *args)


def _engine(torch, shape="tiny", freeze=(), **kw):
    from cfdbench_amd.engine import FnoTrainEngine
    eng = FnoTrainEngine(_make_model(torch, shape, freeze), lr=1e-3, loss_name="nmse", **kw)
    eng.api = _Counting(eng.api)
    return eng


def _batch(torch, i, shape="tiny", bad=False):
    s = SHAPES[shape]
    b = synth.make_batch(711 + i, B, s["H"], s["W"], P, border_mask=True)
    if bad:
        b["label"][0, 0, s["H"] // 2, s["W"] // 2] = np.nan
    return {k: torch.from_numpy(v.copy()).cuda() for k, v in b.items()}


def _bits(torch, *tensors):
    return [t.detach().clone().view(torch.int32) for t in tensors]


def _state(torch, eng):
    return _bits(torch, eng.flat.data, eng.exp_avg, eng.exp_avg_sq)


def _same(torch, a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def _step(torch, eng, route, i, shape="tiny", bad=False):
    """One optimiser step of `route` on batch i; the bad batch is the second of its group / the window's last label."""
    b = _batch(torch, i, shape, bad and route not in ("group", "window"))
    if route == "graph":
        eng.train_step_graph(b["inputs"], b["label"], b["case_params"], b["mask"])
    elif route == "group":
        b2 = _batch(torch, i + 50, shape, bad)
        for k, x in enumerate((b, b2)):
            before = _bits(torch, eng.ema)
            eng.accumulate(x["inputs"], x["label"], x["case_params"], x["mask"], weight=0.5, first=k == 0)
            assert _same(torch, _bits(torch, eng.ema), before), "an accumulate call touched the average"
        eng.apply_accumulated()
    elif route == "window":
        b2 = _batch(torch, i + 50, shape, bad)
        before = _bits(torch, eng.ema)
        eng.accumulate_window(b["inputs"], [b["label"], b2["label"]], b["case_params"], b["mask"], weight=1.0, first=True, detach=False)
        assert _same(torch, _bits(torch, eng.ema), before), "the window's accumulate calls touched the average"
        eng.apply_accumulated()
    else:
        eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])


def _follow(torch, eng, route, shape="tiny", steps=STEPS):
    """`steps` optimiser steps; after each, the average against the rule from its own snapshot before the step and the parameters after
    it, with the decay of that step as the fp32 the call took.  Returns the worst figure in units of the bound."""
    worst = 0.0
    for i in range(steps):
        prev = eng.ema.detach().cpu().numpy().copy()
        _step(torch, eng, route, i, shape)
        torch.cuda.synchronize()
        d = float(np.float32(eng.ema_decay_at(eng.step_count)))
        now = eng.ema.detach().cpu().numpy()
        worst = max(worst, EC.rule_error(now, prev, eng.flat.data.detach().cpu().numpy(), d))
        assert not np.array_equal(now, prev)
    assert eng.step_count == steps
    return worst


VARIANTS = {"plain": {}, "warmup": dict(ema_warmup=True), "frozen": dict(freeze=("blocks",)),
            "adamw_clipped": dict(optimizer="adamw", weight_decay=0.1, max_grad_norm=0.5)}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_engine_average_follows_the_rule_and_moves_no_other_bit(variant, shape):
    """Five steps with the average against five without: parameters and both moments bitwise equal; the average obeys the rule at every
    step (warm-up: d_t = min(d, (1 + t) / (10 + t))); the optimiser call is the new entry point, as often as there were steps; a frozen
    subset's average is as compact as its flat buffer."""
    import torch
    kw = VARIANTS[variant]
    eng = _engine(torch, shape, ema_decay=DECAY, **kw)
    assert eng.ema.numel() == eng.flat.numel and eng.ema.data_ptr() != eng.flat.data.data_ptr() and torch.equal(eng.ema, eng.flat.data)
    if variant == "frozen":
        assert not eng.all_trainable and eng.ema.numel() < sum(p_.numel() * (2 if p_.is_complex() else 1) for p_ in eng.model.parameters())
    if variant == "warmup":
        assert [eng.ema_decay_at(t) for t in (1, 2, 100)] == [2.0 / 11.0, 3.0 / 12.0, DECAY]
    else:
        assert eng.ema_decay_at(1) == DECAY
    assert _follow(torch, eng, "train_step", shape) <= 1.0
    assert eng.api.names.count("cfd_fno_adam_step_ema") == STEPS and not {"cfd_fno_adam_step", "cfd_adam_flat"} & set(eng.api.names)
    plain = _engine(torch, shape, **{k: v for k, v in kw.items() if k != "ema_warmup"})
    for i in range(STEPS):
        _step(torch, plain, "train_step", i, shape)
    torch.cuda.synchronize()
    assert plain.ema is None and "cfd_fno_adam_step_ema" not in plain.api.names
    assert _same(torch, _state(torch, eng), _state(torch, plain)), "the average changed parameters or moments"


@pytest.mark.parametrize("route", ["group", "window", "graph"])
def test_engine_routes(route):
    """An accumulation group of 2 and a K = 2 window: the average changes only in apply_accumulated; graph replay: the call sits outside
    the replay.  Each against the same route without the average, bit for bit."""
    import torch
    eng = _engine(torch, ema_decay=DECAY)
    assert _follow(torch, eng, route, steps=3) <= 1.0
    assert eng.api.names.count("cfd_fno_adam_step_ema") == 3
    plain = _engine(torch)
    for i in range(3):
        b = _batch(torch, i)
        if route == "graph":
            plain.train_step_graph(b["inputs"], b["label"], b["case_params"], b["mask"])
        elif route == "group":
            b2 = _batch(torch, i + 50)
            for k, x in enumerate((b, b2)):
                plain.accumulate(x["inputs"], x["label"], x["case_params"], x["mask"], weight=0.5, first=k == 0)
            plain.apply_accumulated()
        else:
            plain.train_window(b["inputs"], [b["label"], _batch(torch, i + 50)["label"]], b["case_params"], b["mask"], detach=False)
    torch.cuda.synchronize()
    assert _same(torch, _state(torch, eng), _state(torch, plain))


def test_a_skipped_step_leaves_the_engines_average():
    """good / NaN label / good with skip_nonfinite: over the bad step the average keeps its bits with the parameters, step_count runs on,
    and the third step's decay under warm-up is that of t = 3."""
    import torch
    eng = _engine(torch, ema_decay=DECAY, ema_warmup=True, skip_nonfinite=True)
    _step(torch, eng, "train_step", 0)
    s1, e1 = _state(torch, eng), _bits(torch, eng.ema)
    _step(torch, eng, "train_step", 1, bad=True)
    assert bool(eng.last_step_skipped()) and eng.step_count == 2
    assert _same(torch, _state(torch, eng), s1) and _same(torch, _bits(torch, eng.ema), e1), "the skipped step changed the average"
    prev = eng.ema.detach().cpu().numpy().copy()
    _step(torch, eng, "train_step", 2)
    torch.cuda.synchronize()
    assert not bool(eng.last_step_skipped()) and eng.step_count == 3 and eng.ema_decay_at(3) == 4.0 / 13.0
    now, p = eng.ema.detach().cpu().numpy(), eng.flat.data.detach().cpu().numpy()
    assert EC.rule_error(now, prev, p, float(np.float32(4.0 / 13.0))) <= 1.0 and np.isfinite(now).all()
    assert EC.rule_error(now, prev, p, float(np.float32(3.0 / 12.0))) > 1.0  # (the figure tells t = 3 from the second applied step)


def test_optimizer_step_needs_its_pass_and_bad_decays_are_refused():
    import torch
    eng = _engine(torch, ema_decay=DECAY)
    with pytest.raises(RuntimeError, match="ema_decay"):
        eng.optimizer_step()
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            _engine(torch, ema_decay=bad)
    plain = _engine(torch)
    for call in (plain.averaged().__enter__, plain.ema_state_dict, lambda: plain.ema_decay_at(1)):
        with pytest.raises(RuntimeError, match="without ema_decay"):
            call()


def test_averaged_swaps_the_weights_in_and_back():
    """Inside averaged() the model predicts what a fresh Fno2d loaded from ema_state_dict() predicts (reference keys, complex64 spectral
    weights; frozen tensors from the model); afterwards the trained weights are back bit for bit, at the same addresses; it raises inside
    an open group, and an optimiser step inside it raises."""
    import torch
    eng = _engine(torch, freeze=("fc0",), ema_decay=0.5)
    for i in range(3):
        _step(torch, eng, "train_step", i)
    sd = eng.ema_state_dict()
    assert list(sd) == list(eng.model.state_dict()) and all(v.dtype == eng.model.state_dict()[k].dtype for k, v in sd.items())
    assert any(v.dtype == torch.complex64 for v in sd.values())
    assert torch.equal(sd["fc0.weight"], eng.model.state_dict()["fc0.weight"]) and not torch.equal(sd["fc1.weight"], eng.model.state_dict()["fc1.weight"])
    fresh = _make_model(torch)
    fresh.load_state_dict(sd)
    b = _batch(torch, 9)
    eng.model.eval(), fresh.eval()
    with torch.no_grad():
        want = fresh(**b)["preds"].cpu().numpy()
        trained = eng.model(**b)["preds"].cpu().numpy()
        before, ptrs = _state(torch, eng), [p_.data_ptr() for p_ in eng.model.parameters()]
        with eng.averaged() as m:
            assert m is eng.model and torch.equal(eng.flat.data, eng.ema)
            got = eng.model(**b)["preds"].cpu().numpy()
            with pytest.raises(RuntimeError, match="averaged"):
                eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
        after = eng.model(**b)["preds"].cpu().numpy()
    assert O.rel_nmse(got, want) <= 1e-12 and O.rel_nmse(got, trained) > 1e-9
    assert _same(torch, _state(torch, eng)[:1], before[:1]) and ptrs == [p_.data_ptr() for p_ in eng.model.parameters()]
    assert np.array_equal(after, trained)
    eng.model.train()
    eng.accumulate(b["inputs"], b["label"], b["case_params"], b["mask"], weight=1.0, first=True)
    with pytest.raises(RuntimeError, match="accumulation group is open"):
        with eng.averaged():
            pass
    eng.apply_accumulated()


def test_state_dict_round_trip_continues_bitwise():
    import torch
    a = _engine(torch, ema_decay=DECAY, ema_warmup=True)
    for i in range(3):
        _step(torch, a, "train_step", i)
    state = a.state_dict()
    assert state["ema_decay"] == DECAY and state["ema"].data_ptr() != a.ema.data_ptr() and torch.equal(state["ema"], a.ema)
    b = _engine(torch, ema_decay=DECAY, ema_warmup=True)
    b.model.load_state_dict(a.model.state_dict())
    b.load_state_dict(state)
    for eng in (a, b):
        for i in (3, 4):
            _step(torch, eng, "train_step", i)
    torch.cuda.synchronize()
    assert _same(torch, _state(torch, a) + _bits(torch, a.ema), _state(torch, b) + _bits(torch, b.ema))
    # an engine without the average writes the state it always did; loading such a state restarts the average from the loaded weights
    plain = _engine(torch)
    assert "ema" not in plain.state_dict() and "ema_decay" not in plain.state_dict()
    plain.load_state_dict(state)
    c = _engine(torch, ema_decay=DECAY)
    c.model.load_state_dict(a.model.state_dict())
    c.load_state_dict(plain.state_dict())
    assert torch.equal(c.ema, c.flat.data) and torch.equal(c.flat.data, a.flat.data)


def _dp_worker(port, q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), CFDBENCH_DP_ALWAYS_EXCHANGE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        out = {}
        for overlap in (True, False):
            eng = _engine(torch, ema_decay=DECAY, overlap=overlap)
            assert eng.sync.exchange and eng.defer_flags == 0
            worst = _follow(torch, eng, "train_step", steps=3)
            out[overlap] = (worst, eng.api.names.count("cfd_fno_adam_step_ema"), eng.flat.data.cpu().numpy(), eng.ema.cpu().numpy())
        q.put(out)
    finally:
        dist.destroy_process_group()


def test_exchange_route_over_a_one_rank_group():
    """A one-rank gloo group with the exchange forced on (CFDBENCH_DP_ALWAYS_EXCHANGE=1), overlapped and single exchange: the optimiser
    call behind the all-reduce is the new entry, the average obeys the rule, and both exchanges give the same bits."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
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
    for overlap in (True, False):
        assert out[overlap][0] <= 1.0 and out[overlap][1] == 3
    assert np.array_equal(out[True][2], out[False][2]) and np.array_equal(out[True][3], out[False][3])


# ---- the trainer -------------------------------------------------------------------------------------------------------------------
def test_train_auto_fused_writes_and_resumes_the_average(tmp_path):
    """train_auto --fused 1 --ema_decay 0.9 --ema_eval 1 on synthetic data: model_ema.pt beside model.pt with the reference's keys, loadable
    through load_ckpt; three epochs at once equal two plus a resumed third, bit for bit, in both files."""
    import torch

    from cfdbench_amd.harness.common import load_ckpt
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train
    tr = SyntheticAutoDataset(n_cases=4, n_frames=5, height=32, width=32, seed=0)
    dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
    kw = dict(batch_size=4, eval_batch_size=4, log_interval=100, eval_interval=1, plot_interval=0, fused=True, lr=5e-3, ema_decay=0.9,
              ema_eval=True)
    torch.manual_seed(3)
    train(_make_model(torch), tr, dev, tmp_path / "whole", num_epochs=3, **kw)
    torch.manual_seed(3)
    train(_make_model(torch), tr, dev, tmp_path / "parts", num_epochs=2, **kw)
    state = torch.load(tmp_path / "parts" / "train_state.pt", map_location="cpu", weights_only=False)
    assert state["optimizer"]["ema_decay"] == 0.9 and state["optimizer"]["ema"].numel() == state["optimizer"]["numel"]
    train(_make_model(torch), tr, dev, tmp_path / "parts", num_epochs=3, resume=True, **kw)
    keys = list(_make_model(torch).state_dict())
    for ep in range(3):
        for f in ("model.pt", "model_ema.pt"):
            a = torch.load(tmp_path / "whole" / f"ckpt-{ep}" / f, map_location="cpu")
            b = torch.load(tmp_path / "parts" / f"ckpt-{ep}" / f, map_location="cpu")
            assert list(a) == keys and all(torch.equal(a[k], b[k]) for k in keys), (ep, f)
    w, e = (torch.load(tmp_path / "whole" / "ckpt-2" / f, map_location="cpu") for f in ("model.pt", "model_ema.pt"))
    assert any(not torch.equal(w[k], e[k]) for k in keys)
    m = _make_model(torch)
    load_ckpt(m, tmp_path / "whole" / "ckpt-2" / "model_ema.pt")
    assert all(torch.equal(m.state_dict()[k].cpu(), e[k]) for k in keys)
