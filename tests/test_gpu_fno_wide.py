"""MI355X: the FNO's wide-channel route, hidden widths 33 .. 128 (cfdbench_amd/csrc/wide.hip), against the fp64 oracle, through
the C ABI and through Fno2d / FnoRollout (same checks as tests/test_emul_fno_wide.py, at larger sizes and up to width 128)."""
import numpy as np
import pytest

from tests import kernel_checks as K
from tests import wide_checks as WK

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("Cin,Cout", [(33, 33), (48, 40), (64, 64), (20, 72), (128, 128)])
def test_mix_and_spectral_wgrad_wide(be, Cin, Cout):
    _assert_all(K.check_mix_wgrad(be, 37, Cin, Cout))


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
@pytest.mark.parametrize("C", [64, 128])
def test_spectral_fwd_bwd_wide(be, H, W, C):
    _assert_all(K.check_spectral(be, 3, C, C, H, W))


@pytest.mark.parametrize("C", [33, 64, 128])
@pytest.mark.parametrize("act", [0, 1])
def test_chanmix_wide(be, C, act):
    _assert_all(K.check_chanmix(be, 5, C, C, 66 * 65, act))


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
def test_block_wide(be, H, W):
    _assert_all(K.check_block(be, 3, 64, 64, H, W))


@pytest.mark.parametrize("C", [48, 64, 128])
def test_stem_wide(be, C):
    _assert_all(K.check_stem(be, 3, 66, 65, 5, C, True))


@pytest.mark.parametrize("C", [48, 64, 128])
@pytest.mark.parametrize("act", [0, 1])
def test_head_fwd_wide(be, C, act):
    _assert_all(WK.check_head_fwd(be, 3, C, 64 * 64, act))


@pytest.mark.parametrize("C", [48, 64, 128])
def test_head_and_head_train_wide(be, C):
    res = K.check_head(be, 20, C, 64 * 64, True, "nmse", True)
    _assert_all({k: v for k, v in res.items() if k not in ("sums", "scores")})
    assert res["sums"] < 1e-5 and res["scores"] < 1e-5
    res = K.check_head_train(be, 20, C, 64 * 64, True, "nmse")
    assert res.pop("sums") < 1e-5
    _assert_all(res)


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
@pytest.mark.parametrize("C", [48, 64, 128])
def test_fno_wide_vs_oracle(be, H, W, C):
    """Whole model: forward, loss and every parameter gradient (cfd_fno_forward / cfd_fno_backward) with a border mask."""
    res = K.check_fno_vs_oracle(be, 3, C, 2, H, W, border=True)
    assert res.pop("nmse_loss") < 1e-5
    _assert_all(res, 1e-9)


def test_fused_train_step_wide_ignores_deferrals(be):
    res = K.check_fno_train_step_deferred(be, B=4, C=64, L=2, H=64, W=64, which="mse", flags=7)
    assert res.pop("sums") == 0.0 and res.pop("preds") == 0.0
    assert res.pop("params") == 0.0 and res.pop("grad_vs_immediate") == 0.0
    _assert_all(res, 1e-11)


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
@pytest.mark.parametrize("C", [48, 64, 128])
def test_fno_forward_wide_vs_oracle(be, H, W, C):
    _assert_all(WK.check_fno_forward_vs_oracle(be, 4, C, 2, H, W, border=True))


def test_bf16_storage_refused_wide(be):
    res = WK.check_wide_refusals(be)
    assert all(res.values()), res


def _wide_model(C=64, L=2, p=5, seed=41):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    from oracle import synth

    params = synth.make_fno_params(seed, C, L, 12, 12, p, spectral_gain=4.0)
    model = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C).to(torch.device("cuda", 0))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model, params


@pytest.mark.parametrize("H,W", [(64, 64), (66, 65)])
def test_fno2d_wide_inference_and_rollout(be, H, W):
    """Fno2d at width 64 under no_grad against the oracle; FnoRollout's captured graph bitwise equal to generate_many; two
    identical forward calls bitwise equal."""
    import torch

    from cfdbench_amd.rollout import FnoRollout
    from oracle import fno_oracle as O
    from oracle import synth

    L, p, steps = 2, 5, 3
    model, params = _wide_model(64, L, p)
    batch = synth.make_batch(42, 3, H, W, p, border_mask=True)
    dev = torch.device("cuda", 0)
    tb = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    with torch.no_grad():
        preds = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        again = model(inputs=tb["inputs"], case_params=tb["case_params"], mask=tb["mask"])["preds"]
        frames = model.generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
        gframes = FnoRollout(model).generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
    torch.cuda.synchronize()
    p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in params.items()}
    b64 = {k: v.astype(np.float64) for k, v in batch.items()}
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], None, L)
    assert O.rel_nmse(preds.cpu().numpy(), ref["preds"]) < K.TOL
    assert torch.equal(preds, again)
    assert len(frames) == len(gframes) == steps
    rframes = O.generate_many(p64, b64["inputs"], b64["case_params"], b64["mask"], steps, num_layers=L)
    for a, b, r in zip(frames, gframes, rframes):
        assert torch.equal(a, b)
        assert O.rel_nmse(a.cpu().numpy(), r) < K.TOL


def test_fno_train_engine_wide_is_deterministic():
    """FnoTrainEngine at width 64: two engines from the same state, the same two steps -> bitwise-equal parameters."""
    import torch

    from cfdbench_amd.engine import FnoTrainEngine
    from oracle import synth

    outs = []
    for _ in range(2):
        model, _p = _wide_model(64, 2, 5)
        eng = FnoTrainEngine(model, lr=1e-3, loss_name="nmse")
        b = {k: torch.from_numpy(v).cuda() for k, v in synth.make_batch(43, 4, 64, 64, 5, border_mask=True).items()}
        for _ in range(2):
            eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
        torch.cuda.synchronize()
        outs.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def test_train_auto_wide_fused_and_autograd(tmp_path):
    """train_auto at --fno_hidden_dim 64, autograd (--fused 0) and fused (--fused 1): one epoch on synthetic data, artefacts
    written, then test_multistep; the two paths' per-step losses agree."""
    import torch

    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import test, train

    losses = {}
    for fused in (0, 1):
        args = Args(model="fno", data_name="cavity_bc", loss_name="nmse", fno_hidden_dim=64, fno_depth=2, lr=1e-3,
                    output_dir=str(tmp_path / f"f{fused}"), num_epochs=1, batch_size=4, eval_batch_size=4, eval_interval=1,
                    log_interval=5, plot_interval=0, fused=fused)
        out = get_output_dir(args, is_auto=True)
        tr = SyntheticAutoDataset(n_cases=4, n_frames=4, height=64, width=64, seed=0)
        dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=64, width=64, seed=1)
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


def _golden(name):
    from pathlib import Path
    return np.load(Path(__file__).resolve().parent / "golden" / f"{name}.npz")


def test_fno2d_wide_vs_reference_golden():
    """Width-64 model of the reference (tools/make_golden_wide.py): predictions, the four losses and sampled gradient entries."""
    import torch

    from oracle import fno_oracle as O
    from oracle import synth

    g = _golden("fno_w64_64x64")
    pseed, bseed, B, C, L, H, W, p, border = [int(v) for v in g["meta"]]
    model, params = _wide_model(C, L, p, pseed)
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=float(g["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
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


def test_generate_many_wide_vs_reference_golden():
    import torch

    from oracle import fno_oracle as O
    from oracle import synth

    g = _golden("rollout_w64_66x65")
    pseed, bseed, B, C, L, H, W, p, steps, border = [int(v) for v in g["meta"]]
    model, _p = _wide_model(C, L, p, pseed)
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=float(g["gain"]))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    batch = synth.make_smooth_batch(bseed, B, H, W, p)
    if border:
        batch["mask"][:, :, 0, :] = 0
        batch["mask"][:, :, -1, :] = 0
        batch["mask"][:, :, :, 0] = 0
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    with torch.no_grad():
        frames = model.eval().generate_many(b["inputs"], b["case_params"], b["mask"], steps)
    assert len(frames) == steps
    assert O.rel_nmse(frames[0].cpu().numpy(), g["first"]) < K.TOL
    assert O.rel_nmse(frames[-1].cpu().numpy(), g["last"]) < 1e-7
