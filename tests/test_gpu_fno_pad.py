"""MI355X: the FNO with domain padding (cfd_fno_shape.pad, cfdbench_amd/csrc/pad.hip) against the padded fp64 oracle of tests/pad_checks.py
and the reference, through the C ABI and through Fno2d(padding=p) / FnoTrainEngine / FnoRollout / the harness (same checks as
tests/test_emul_fno_pad.py, at device batch and channel counts)."""
from pathlib import Path

import numpy as np
import pytest

from tests import kernel_checks as K
from tests import pad_checks as PC

pytestmark = pytest.mark.gpu

SHAPES = PC.SHAPES
USUAL = [PC.SHAPES[3], PC.SHAPES[5]]  # (60, 60, 4) on the 64 x 64 plan, (64, 64, 8) on 72 x 72


@pytest.fixture(scope="module")
def be():
    from tests.backends import TorchBackend
    return TorchBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_all(res, tol=K.TOL):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


@pytest.mark.parametrize("H,W,pad,m1,m2", SHAPES)
def test_fno_pad_vs_oracle(be, H, W, pad, m1, m2):
    """Whole model at width 20: forward under both workspaces, loss and every parameter gradient."""
    PC.accept_vs_oracle(PC.check_fno_pad_vs_oracle(be, 3, 20, 2, H, W, pad, m1, m2))


@pytest.mark.parametrize("C", [32, 40])
@pytest.mark.parametrize("H,W,pad,m1,m2", USUAL)
def test_fno_pad_vs_oracle_widths(be, H, W, pad, m1, m2, C):
    """Width 32 (one-workgroup FnoBlock) and 40 (wide route)."""
    PC.accept_vs_oracle(PC.check_fno_pad_vs_oracle(be, 3, C, 2, H, W, pad, m1, m2))


@pytest.mark.parametrize("H,W,pad,m1,m2", [PC.SHAPES[2], PC.SHAPES[5]])
def test_fno_pad_vs_oracle_channel_route(be, H, W, pad, m1, m2):
    """in_chan 3 / out_chan 3: the head's channel route behind the crop."""
    PC.accept_vs_oracle(PC.check_fno_pad_vs_oracle(be, 3, 20, 2, H, W, pad, m1, m2, cin=3, cout=3))


@pytest.mark.parametrize("which", ["mse", "nmse"])
@pytest.mark.parametrize("H,W,pad,m1,m2", SHAPES)
def test_pad_train_step_ignores_deferrals(be, H, W, pad, m1, m2, which):
    res = PC.check_pad_train_step(be, 3, 20, 2, H, W, pad, m1, m2, which=which)
    assert res.pop("bitwise") == 0.0
    _assert_all(res, 1e-9)


@pytest.mark.parametrize("C", [32, 40])
@pytest.mark.parametrize("H,W,pad,m1,m2", USUAL)
def test_pad_train_step_widths(be, H, W, pad, m1, m2, C):
    res = PC.check_pad_train_step(be, 3, C, 2, H, W, pad, m1, m2, which="nmse")
    assert res.pop("bitwise") == 0.0
    _assert_all(res, 1e-9)


@pytest.mark.parametrize("H,W,pad,m1,m2", SHAPES)
def test_pad_band_written_on_every_call(be, H, W, pad, m1, m2):
    res = PC.check_pad_dirty(be, 3, 20, 2, H, W, pad, m1, m2)
    assert res.pop("second_run") == 0.0 and res.pop("finite_fill") == 0.0, res
    _assert_all(res)


def test_pad_misaligned(be):
    assert PC.check_pad_misaligned(be, B=3, C=20) >= 1


@pytest.mark.parametrize("H,W,pad,m1,m2", SHAPES)
def test_pad_zero_spectral_equals_unpadded(be, H, W, pad, m1, m2):
    _assert_all(PC.check_pad_zero_spectral(be, 3, 20, 2, H, W, pad, m1, m2))


def test_pad_refusals(be):
    res = PC.check_pad_refusals(be, C=20)
    assert all(v is True for v in res.values()), res


def test_pad_zero_is_the_unpadded_call(be):
    res = PC.check_pad_zero_is_unpadded(be, B=3, C=20)
    assert all(res.values()), res


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _model(C, L, m1, m2, pad, p=5, seed=41, gain=4.0):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    from oracle import synth

    params = synth.make_fno_params(seed, C, L, m1, m2, p, spectral_gain=gain)
    model = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, m1, m2, C, padding=pad).to(torch.device("cuda", 0))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model, params


def _golden(name):
    return np.load(Path(__file__).resolve().parent / "golden" / f"{name}.npz")


@pytest.mark.parametrize("name", ["fno_pad8_64x64", "fno_pad9_66x65"])
def test_fno2d_pad_vs_reference_golden(name):
    """Fno2d(padding=p) against the reference's (tools/make_golden_pad.py): predictions, the four losses and sampled gradient entries."""
    import torch

    from oracle import fno_oracle as O
    from oracle import synth

    g = _golden(name)
    pseed, bseed, B, C, L, H, W, p, border, m1, m2, pad = [int(v) for v in g["meta"]]
    model, _p = _model(C, L, m1, m2, pad, p, pseed, float(g["gain"]))
    assert model.abi_config()["padding"] == pad
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=bool(border))
    out = model(**{k: torch.from_numpy(v).cuda() for k, v in batch.items()})
    out["loss"]["nmse"].backward()
    assert out["preds"].shape == (B, 2, H, W)
    assert O.rel_nmse(out["preds"].detach().cpu().numpy(), g["preds"]) < K.TOL
    for k in ("mse", "rmse", "mae", "nmse"):
        assert abs(out["loss"][k].item() - float(g[f"loss_{k}"])) <= 5e-6 * abs(float(g[f"loss_{k}"]))
    grads = dict(model.named_parameters())
    n = 0
    for key in g.files:
        if key.startswith("gsum::") and key.endswith("::vals"):
            k = key.split("::")[1]
            got = grads[k].grad.cpu().numpy().reshape(-1)[g[f"gsum::{k}::idx"]]
            assert O.rel_nmse(got, g[key]) < 1e-6, k
            n += 1
    assert n == len(grads)


@pytest.mark.parametrize("C", [20, 40])
def test_fno_train_engine_pad_matches_autograd(C):
    """FnoTrainEngine's fused step at (60, 60, pad 4) against Fno2d's autograd gradients; two engines from the same state take
    bitwise-equal steps."""
    import torch

    from cfdbench_amd.engine import FnoTrainEngine
    from oracle import synth

    b = {k: torch.from_numpy(v).cuda() for k, v in synth.make_batch(43, 4, 60, 60, 5, border_mask=True).items()}
    ref, _p = _model(C, 2, 12, 12, 4)
    out = ref(**b)
    out["loss"]["nmse"].backward()
    want = {n: (torch.view_as_real(q.grad) if q.is_complex() else q.grad).detach().cpu().numpy().reshape(-1) for n, q in ref.named_parameters()}
    flats = []
    for _ in range(2):
        model, _p = _model(C, 2, 12, 12, 4)
        eng = FnoTrainEngine(model, lr=1e-3, loss_name="nmse")
        eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
        torch.cuda.synchronize()
        g = eng.gradients().cpu().numpy()
        names = {id(q): n for n, q in model.named_parameters()}
        for q, off in zip(eng.flat.params, eng.flat.offsets):
            n = names[id(q)]
            assert K.nm(g[off:off + want[n].size], want[n]) < 1e-9, n
        flats.append(eng.flat.data.detach().clone())
    assert torch.equal(flats[0], flats[1])


@pytest.mark.parametrize("H,W,pad", [(64, 64, 8), (70, 76, 12)])
def test_fno2d_pad_inference_and_rollout(H, W, pad):
    """Fno2d(padding=p) under no_grad against the padded oracle; two calls bitwise equal; FnoRollout's captured graph bitwise equal to
    generate_many over 3 steps."""
    import torch

    from cfdbench_amd.rollout import FnoRollout
    from oracle import synth
    from tests import chan_checks as CK

    L, p, steps = 2, 5, 3
    model, params = _model(20, L, 12, 12, pad)
    batch = synth.make_batch(42, 3, H, W, p, border_mask=True)
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    with torch.no_grad():
        preds = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        again = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        frames = model.generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
        gframes = FnoRollout(model).generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
    torch.cuda.synchronize()
    p64, b64 = CK._to64(params, batch)
    cur = b64["inputs"]
    assert torch.equal(preds, again)
    assert len(frames) == len(gframes) == steps
    for t, (a, g) in enumerate(zip(frames, gframes)):
        cur = PC.oracle_forward(p64, cur, b64["case_params"], b64["mask"], None, L, pad)["preds"]
        if t == 0:
            assert K.nm(preds.cpu().numpy(), cur) < K.TOL
        assert torch.equal(a, g)
        assert K.nm(a.cpu().numpy(), cur) < K.TOL, t


def test_one_padded_model_serves_several_grids():
    """One Fno2d(padding=8) evaluated at 64 x 64, at 66 x 65 and at 64 x 64 again: each against the padded oracle, the first and the third
    bitwise equal."""
    import torch

    from oracle import synth
    from tests import chan_checks as CK

    L, p, pad = 2, 5, 8
    model, params = _model(20, L, 12, 12, pad)
    outs = []
    for seed, H, W in ((44, 64, 64), (45, 66, 65), (44, 64, 64)):
        batch = synth.make_batch(seed, 2, H, W, p, border_mask=True)
        tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        with torch.no_grad():
            preds = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        torch.cuda.synchronize()
        p64, b64 = CK._to64(params, batch)
        ref = PC.oracle_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], None, L, pad)
        assert preds.shape == (2, 2, H, W)
        assert K.nm(preds.cpu().numpy(), ref["preds"]) < K.TOL, (H, W)
        outs.append(preds.clone())
    assert torch.equal(outs[0], outs[2])


def test_padding_argument_values():
    """padding=0 (the reference returns empty tensors) and negatives raise ValueError; state_dict keys and shapes do not depend on padding."""
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn

    with pytest.raises(ValueError, match="empty"):
        Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 2, 12, 12, 20, padding=0)
    with pytest.raises(ValueError):
        Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 2, 12, 12, 20, padding=-1)
    a = Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 2, 12, 12, 20)
    b = Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 2, 12, 12, 20, padding=8)
    assert a.abi_config()["padding"] == 0 and b.abi_config()["padding"] == 8
    assert {k: tuple(v.shape) for k, v in a.state_dict().items()} == {k: tuple(v.shape) for k, v in b.state_dict().items()}


def test_rollout_bf16_refused_with_padding():
    import torch

    from cfdbench_amd._capi import CfdError
    from cfdbench_amd.rollout import FnoRollout
    from oracle import synth

    model, _p = _model(20, 2, 12, 12, 4)
    tb = {k: torch.from_numpy(v).cuda() for k, v in synth.make_batch(46, 2, 60, 60, 5, border_mask=True).items()}
    with pytest.raises(CfdError):
        with torch.no_grad():
            FnoRollout(model, dtype="bf16").generate_many(tb["inputs"], tb["case_params"], tb["mask"], 2)
    torch.cuda.synchronize()


def test_train_auto_pad_fused_and_autograd(tmp_path):
    """train_auto at --fno_padding 8 on a 32 x 32 synthetic dataset, autograd (--fused 0) and fused (--fused 1): one epoch, artefacts
    written under a directory that names the padding; the two paths' per-step losses agree."""
    import torch

    from cfdbench_amd.harness.args import Args, is_args_valid
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import train

    losses = {}
    for fused in (0, 1):
        args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--loss_name", "nmse", "--fno_hidden_dim", "20", "--fno_depth", "2",
                                  "--lr", "0.001", "--output_dir", str(tmp_path / f"f{fused}"), "--num_epochs", "1", "--batch_size", "4",
                                  "--eval_batch_size", "4", "--eval_interval", "1", "--log_interval", "5", "--plot_interval", "0",
                                  "--fused", str(fused), "--fno_padding", "8"])
        is_args_valid(args)
        out = get_output_dir(args, is_auto=True)
        assert out.name.endswith("_pad8")
        tr = SyntheticAutoDataset(n_cases=4, n_frames=4, height=32, width=32, seed=0)
        dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=32, width=32, seed=1)
        torch.manual_seed(0)
        model = init_model(args).cuda()
        assert model.padding == 8
        losses[fused] = train(model, tr, dev, out, num_epochs=1, lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma,
                              batch_size=4, eval_batch_size=4, log_interval=5, eval_interval=1, fused=bool(fused), plot_interval=0)
        assert (out / "train_losses.json").exists()
    a, b = np.asarray(losses[0], dtype=np.float64), np.asarray(losses[1], dtype=np.float64)
    assert a.shape == b.shape and np.all(np.isfinite(a))
    assert np.max(np.abs(a - b) / np.abs(a)) < 1e-4
