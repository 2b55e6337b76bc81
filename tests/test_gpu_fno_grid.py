"""MI355X: the FNO on grids wider than 80 columns, up to 128 x 128 -- many-modes plans whatever their mode counts
(cfdbench_amd/csrc/dft_many.hip) -- against the fp64 oracle and the reference, through the C ABI and through Fno2d / FnoTrainEngine /
FnoRollout / the harness (same kernel checks as tests/test_emul_fno_grid.py, at device image counts)."""
from pathlib import Path

import numpy as np
import pytest

from tests import grid_checks as G
from tests import kernel_checks as K
from tests import modes_checks as MK

pytestmark = pytest.mark.gpu

SHAPES = G.SHAPES
BIG = [(96, 96, 12, 12), (128, 128, 64, 65)]


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


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_spectral_fwd_bwd_grid(be, H, W, m1, m2):
    _assert_all(K.check_spectral(be, 8, 20, 20, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_idft_epilogues_and_gelu_dft_grid(be, H, W, m1, m2):
    """8 images (work items cut small to fill the grid), and at two shapes 1100: over twice the 512 persistent workgroups of a launch,
    so that every workgroup takes a second item."""
    _assert_all(K.check_idft_epilogues(be, 1100 if (H, W, m1, m2) in BIG else 8, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2", BIG)
@pytest.mark.parametrize("C", [20, 32])
def test_mix_and_spectral_wgrad_grid(be, H, W, m1, m2, C):
    _assert_all(K.check_mix_wgrad(be, 130, C, C, m1, m2, H, W))


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_block_grid(be, H, W, m1, m2):
    _assert_all(K.check_block(be, 8, 32, 32, H, W, m1, m2))


@pytest.mark.parametrize("H,W,m1,m2,C", [(96, 96, 12, 12, 20), (128, 128, 64, 65, 20), (100, 120, 50, 61, 32), (96, 100, 24, 24, 64)])
def test_fno_grid_vs_oracle(be, H, W, m1, m2, C):
    """Whole model (cfd_fno_forward / cfd_fno_backward) with a border mask: forward, loss and every parameter gradient."""
    res = MK.check_fno_vs_oracle(be, 3, C, 2, H, W, m1, m2)
    assert res.pop("nmse_loss") < 1e-5
    _assert_all(res, 1e-9)


def test_fused_train_step_grid_ignores_deferrals(be):
    res = MK.check_train_step_deferred(be, B=4, C=20, L=2, H=96, W=100, m1=12, m2=12)
    assert res.pop("bitwise") == 0.0
    _assert_all(res, 1e-9)


def test_transforms_grid_misaligned(be):
    """The transforms at (97, 113, 48, 57) on buffers 4 bytes past a 16-byte boundary."""
    assert G.check_transforms_misaligned(be, 8, 97, 113, 48, 57) >= 1


@pytest.mark.parametrize("H,W,m1,m2", SHAPES)
def test_transform_lds_of_the_shapes(be, H, W, m1, m2):
    for inverse in (0, 1):
        assert 0 < G.lds_bytes(be, H, W, m1, m2, inverse) <= G.LDS_CAP
    assert G.lds_bytes(be, 64, 64, 12, 12, 0) == 0


def test_grid_range_and_bf16_refusals(be):
    res = G.check_range(be)
    assert all(res.values()), res
    res = MK.check_refusals(be, H=24, W=84, m1=3, m2=4)
    assert res["bf16_forward"] and res["bf16_train"], res


def _model(C, L, m1, m2, p=5, seed=41, gain=4.0):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    from oracle import synth

    params = synth.make_fno_params(seed, C, L, m1, m2, p, spectral_gain=gain)
    model = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, m1, m2, C).to(torch.device("cuda", 0))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model, params


def _f64(params, batch):
    p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in params.items()}
    return p64, {k: v.astype(np.float64) for k, v in batch.items()}


@pytest.mark.parametrize("C", [20, 64])
def test_fno_train_engine_grid_matches_autograd(C):
    """FnoTrainEngine's fused step at 96 x 100 against Fno2d's autograd gradients; two engines from the same state take bitwise-equal
    steps."""
    import torch

    from cfdbench_amd.engine import FnoTrainEngine
    from oracle import synth

    b = {k: torch.from_numpy(v).cuda() for k, v in synth.make_batch(43, 4, 96, 100, 5, border_mask=True).items()}
    ref, _p = _model(C, 2, 12, 12)
    out = ref(**b)
    out["loss"]["nmse"].backward()
    want = {n: (torch.view_as_real(q.grad) if q.is_complex() else q.grad).detach().cpu().numpy().reshape(-1) for n, q in ref.named_parameters()}
    flats = []
    for _ in range(2):
        model, _p = _model(C, 2, 12, 12)
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


@pytest.mark.parametrize("H,W,m1,m2", [(128, 128, 12, 12), (100, 120, 50, 61)])
def test_fno2d_grid_inference_and_rollout(H, W, m1, m2):
    """Fno2d under no_grad against the oracle; FnoRollout's captured graph bitwise equal to generate_many; two calls bitwise equal."""
    import torch

    from cfdbench_amd.rollout import FnoRollout
    from oracle import fno_oracle as O
    from oracle import synth

    L, p, steps = 2, 5, 3
    model, params = _model(20, L, m1, m2)
    batch = synth.make_batch(42, 3, H, W, p, border_mask=True)
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    with torch.no_grad():
        preds = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        again = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        frames = model.generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
        gframes = FnoRollout(model).generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
    torch.cuda.synchronize()
    p64, b64 = _f64(params, batch)
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], None, L)
    assert O.rel_nmse(preds.cpu().numpy(), ref["preds"]) < K.TOL
    assert torch.equal(preds, again)
    assert len(frames) == len(gframes) == steps
    rframes = O.generate_many(p64, b64["inputs"], b64["case_params"], b64["mask"], steps, num_layers=L)
    for a, g, r in zip(frames, gframes, rframes):
        assert torch.equal(a, g)
        assert O.rel_nmse(a.cpu().numpy(), r) < K.TOL


def test_one_model_serves_several_grids():
    """One model at modes (12, 12) run at 64 x 64 (narrow route), 128 x 128 (many-modes route) and 64 x 64 again: each against the oracle,
    the first and the third bitwise equal."""
    import torch

    from oracle import fno_oracle as O
    from oracle import synth

    L, p = 2, 5
    model, params = _model(20, L, 12, 12)
    outs = []
    for seed, n in ((44, 64), (45, 128), (44, 64)):
        batch = synth.make_batch(seed, 2, n, n, p, border_mask=True)
        tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        with torch.no_grad():
            preds = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        torch.cuda.synchronize()
        p64, b64 = _f64(params, batch)
        ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], None, L)
        assert preds.shape == (2, 2, n, n)
        assert O.rel_nmse(preds.cpu().numpy(), ref["preds"]) < K.TOL, n
        outs.append(preds.clone())
    assert torch.equal(outs[0], outs[2])


def test_rollout_bf16_refused_on_wide_grid():
    import torch

    from cfdbench_amd._capi import CfdError
    from cfdbench_amd.rollout import FnoRollout
    from oracle import synth

    model, _p = _model(20, 2, 12, 12)
    tb = {k: torch.from_numpy(v).cuda() for k, v in synth.make_batch(46, 2, 96, 100, 5, border_mask=True).items()}
    with pytest.raises(CfdError):
        with torch.no_grad():
            FnoRollout(model, dtype="bf16").generate_many(tb["inputs"], tb["case_params"], tb["mask"], 2)
    torch.cuda.synchronize()


def test_train_auto_grid_fused_and_autograd(tmp_path):
    """train_auto on a 96 x 100 synthetic dataset, autograd (--fused 0) and fused (--fused 1): one epoch, artefacts written, then test();
    the two paths' per-step losses agree."""
    import torch

    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import test, train

    losses = {}
    for fused in (0, 1):
        args = Args(model="fno", data_name="cavity_bc", loss_name="nmse", fno_hidden_dim=20, fno_depth=2, lr=1e-3,
                    output_dir=str(tmp_path / f"f{fused}"), num_epochs=1, batch_size=4, eval_batch_size=4, eval_interval=1,
                    log_interval=5, plot_interval=0, fused=fused)
        out = get_output_dir(args, is_auto=True)
        tr = SyntheticAutoDataset(n_cases=4, n_frames=4, height=96, width=100, seed=0)
        dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=96, width=100, seed=1)
        torch.manual_seed(0)
        model = init_model(args).cuda()
        losses[fused] = train(model, tr, dev, out, num_epochs=1, lr=args.lr, lr_step_size=args.lr_step_size, lr_gamma=args.lr_gamma,
                              batch_size=4, eval_batch_size=4, log_interval=5, eval_interval=1, fused=bool(fused), plot_interval=0)
        assert (out / "train_losses.json").exists()
        test(model, dev, out / "test", infer_steps=2, plot_interval=10, batch_size=1)
        assert (out / "test" / "preds.pt").exists() and (out / "test" / "scores.json").exists()
    a, b = np.asarray(losses[0], dtype=np.float64), np.asarray(losses[1], dtype=np.float64)
    assert a.shape == b.shape and np.all(np.isfinite(a))
    assert np.max(np.abs(a - b) / np.abs(a)) < 1e-4


def test_multistep_grid(tmp_path):
    """test_multistep's batched inference at 96 x 100 against its per-case formulation."""
    import torch

    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.test_multistep import get_metrics, infer, infer_case, prepare_cases

    args = Args(model="fno", data_name="cavity_bc", loss_name="nmse", fno_hidden_dim=20, fno_depth=2, output_dir=str(tmp_path))
    torch.manual_seed(1)
    model = init_model(args).cuda()
    data = SyntheticAutoDataset(n_cases=3, n_frames=4, height=96, width=100, seed=5, border_mask=True)
    steps = 4
    feats, cps = prepare_cases(data, steps)
    metrics = infer(model, feats, cps, steps)
    assert len(metrics) == steps
    preds = [infer_case(model, f, c, steps) for f, c in zip(feats, cps)]
    for s in range(steps):
        ms = [get_metrics(preds[c][s][0][0] * feats[c][s][-1], feats[c][s][0] * feats[c][s][-1]) for c in range(3)]
        for k in metrics[s]:
            want = float(np.mean([m[k] for m in ms]))
            assert np.isfinite(metrics[s][k]) and abs(metrics[s][k] - want) <= 1e-5 * abs(want) + 1e-12, (s, k)


def _golden(name):
    return np.load(Path(__file__).resolve().parent / "golden" / f"{name}.npz")


def test_fno2d_grid_vs_reference_golden():
    """96 x 100 model at the default modes (12, 12) of the reference (tools/make_golden_grid.py): predictions, the four losses and sampled
    gradient entries."""
    import torch

    from oracle import fno_oracle as O
    from oracle import synth

    g = _golden("fno_g96x100_m12")
    pseed, bseed, B, C, L, H, W, p, border, m1, m2 = [int(v) for v in g["meta"]]
    model, _p = _model(C, L, m1, m2, p, pseed, float(g["gain"]))
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=bool(border))
    out = model(**{k: torch.from_numpy(v).cuda() for k, v in batch.items()})
    out["loss"]["nmse"].backward()
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


def test_spectral_grid_vs_reference_golden(be):
    """SpectralConv2d at 100 x 120, modes (50, 61), of the reference (tools/make_golden_grid.py): output and all three gradients."""
    _assert_all(MK.check_spectral_golden(be, _golden("spectral_g100x120_m50x61")), 1e-9)
