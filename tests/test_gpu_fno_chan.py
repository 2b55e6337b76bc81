"""MI355X: the FNO at channel counts other than 2 / 2 -- the projection head's channel route (out_chan 3 .. 8) on the narrow, wide and
many-modes routes, the lifting layer at in_chan 1 and 3 .. 8, and the model-level paths on top (Fno2d under autograd, FnoRollout,
FnoTrainEngine, train_auto / test).  The emulator twin (and the CPU-only checks of this feature) is tests/test_emul_fno_chan.py."""
from pathlib import Path

import numpy as np
import pytest

from tests import chan_checks as CK
from tests import kernel_checks as K
from tests import wide_checks as WK
from tests.backends import TorchBackend

pytestmark = pytest.mark.gpu

GRIDS = [(64, 64), (66, 65)]  # 66 x 65: planes that are not 16-byte aligned


@pytest.fixture(scope="module")
def be():
    return TorchBackend()


@pytest.fixture(autouse=True)
def _guard_bands_intact(be):
    """Every buffer of tests/backends.py sits between guard bands: a write outside one fails the test that made it."""
    yield
    be.verify()


def _assert_all(res, tol=K.TOL):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


def _assert_head(res):
    assert res.pop("sums") < 1e-5 and res.pop("scores", 0.0) < 1e-5, res
    _assert_all(res)


def _assert_head_fwd(res):
    assert res.pop("count") == 0.0
    _assert_all(res)  # (the sums: nm() of one element, the squared relative error -- 1e-5 relative)


@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("C", [20, 32, 48, 128])
@pytest.mark.parametrize("Co", [3, 4, 5, 8])
def test_head_fwd_chan(be, Co, C, act):
    for HW in (64 * 64, 66 * 65):
        _assert_head_fwd(WK.check_head_fwd(be, 3, C, HW, act, Co=Co))


@pytest.mark.parametrize("Co,C", [(5, 20), (8, 32)])
def test_head_fwd_chan_multi_tile_loop(be, Co, C):
    """One workgroup walks every tile."""
    with K.tuned(be, head_blocks=1):
        _assert_head_fwd(WK.check_head_fwd(be, 3, C, 66 * 65, 1, Co=Co))


@pytest.mark.parametrize("which", ["mse", "nmse", "mae"])
@pytest.mark.parametrize("C", [20, 32, 48])
@pytest.mark.parametrize("Co", [3, 5, 8])
def test_head_bwd_and_train_chan(be, Co, C, which):
    for HW in (64 * 64, 66 * 65):
        _assert_head(CK.check_head(be, 3, C, HW, (Co + C // 4) % 2, Co, which))
        _assert_head(CK.check_head_train(be, 3, C, HW, (Co + C // 4 + 1) % 2, Co, which))


@pytest.mark.parametrize("Co,C", [(3, 20), (8, 32), (5, 48)])
def test_head_bwd_chan_external_gradient(be, Co, C):
    _assert_head(CK.check_head(be, 3, C, 66 * 65, 1, Co, label_loss=False))


def test_head_bwd_chan_multi_tile_loop(be):
    with K.tuned(be, head_blocks=2):
        _assert_head(CK.check_head(be, 3, 20, 66 * 65, 1, 5, "nmse", with_ext=True))


@pytest.mark.parametrize("C", [20, 48])
@pytest.mark.parametrize("P_", [0, 5])
@pytest.mark.parametrize("cin", [1, 3, 4, 5, 8])
def test_stem_chan(be, cin, P_, C):
    for H, W in GRIDS:
        _assert_all(CK.check_stem(be, 3, H, W, P_, C, cin))


def _assert_model(res):
    assert res.pop("losses") < 1e-5, res
    _assert_all(res, 1e-9)
    assert res["preds"] < K.TOL and res["preds_infer"] < K.TOL, res


@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("cin,cout,C", [(3, 3, 20), (4, 4, 20), (8, 8, 20), (1, 3, 20), (5, 1, 20), (3, 3, 32), (3, 3, 48)])
def test_fno_chan_vs_oracle(be, cin, cout, C, H, W):
    """Whole model through cfd_fno_forward / cfd_fno_backward, L = 2, border mask: forward, losses and every parameter gradient."""
    _assert_model(CK.check_fno_vs_oracle(be, 3, C, 2, H, W, cin, cout))


def test_fno_chan_many_modes_vs_oracle(be):
    _assert_model(CK.check_fno_vs_oracle(be, 3, 20, 2, 64, 64, 3, 3, m1=16, m2=16))


@pytest.mark.parametrize("H,W", GRIDS)
def test_fused_train_step_chan(be, H, W):
    """flags = 7 against flags = 0: nothing is deferred above two output channels -- bitwise-equal steps, oracle gradients."""
    res = CK.check_fno_train_step(be, B=3, C=20, L=2, H=H, W=W, cin=3, cout=3, which="nmse", flags=7)
    assert res.pop("sums") == 0.0 and res.pop("preds") == 0.0
    assert res.pop("params") == 0.0 and res.pop("grad_vs_immediate") == 0.0
    _assert_all(res, 1e-9)


def test_fused_train_step_on_odd_fc0_ranges(be):
    """tests/test_emul_fno_chan.py's row: k_adam_f's walk over 16-byte units that are half the lifting-layer job's."""
    res = CK.check_fno_train_step(be, 1, 5, 1, 64, 64, 2, 2, p=4, flags=7)
    print(res)
    assert res.pop("sums") < 1e-6 and res.pop("preds") == 0.0
    _assert_all(res, 1e-11)


def test_refusals_chan(be):
    res = CK.check_refusals(be, H=64, W=64)
    assert all(res.values()), res


def test_dirty_reuse_head_chan(be):
    res = K.check_dirty_reuse(be, CK.case_head, dict(B=128, HW=4096), dict(B=3, HW=4096))
    assert not any(res.values()), res


# ---- model level -----------------------------------------------------------------------------------------------------------

def _model(cin=3, cout=3, C=20, L=2, p=5, seed=51, gain=4.0):
    import torch

    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn

    params = CK.make_params(seed, C, L, 12, 12, p, cin, cout, gain)
    model = Fno2d(cin, cout, p, loss_name_to_fn("nmse"), L, 12, 12, C).to(torch.device("cuda", 0))
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return model, params


def _p64(params):
    return {k: v.astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in params.items()}


@pytest.mark.parametrize("H,W", GRIDS)
def test_fno2d_chan_autograd_vs_oracle(H, W):
    """Fno2d(3, 3) under autograd: predictions and every gradient against the oracle; two identical forward calls bitwise equal."""
    import torch

    from oracle import fno_oracle as O

    L = 2
    model, params = _model()
    batch = CK.make_batch(52, 3, H, W, 5, 3, 3, border=True)
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    out = model(**tb)
    out["loss"]["nmse"].backward()
    with torch.no_grad():
        again = model(**tb)["preds"]
    b64 = {k: v.astype(np.float64) for k, v in batch.items()}
    ref = O.fno_forward(_p64(params), b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
    rg = O.fno_backward(_p64(params), ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], "nmse"), L)
    assert O.rel_nmse(out["preds"].detach().cpu().numpy(), ref["preds"]) < K.TOL
    assert torch.equal(out["preds"].detach(), again)
    assert abs(out["loss"]["nmse"].item() - ref["loss"]["nmse"]) < 1e-5 * ref["loss"]["nmse"]
    for k, prm in model.named_parameters():
        assert O.rel_nmse(prm.grad.cpu().numpy(), rg[k]) < 1e-9, k


def test_rollout_chan_graph_vs_eager_vs_oracle():
    """FnoRollout (one HIP graph), 3 steps at 66 x 65 with a border mask: bitwise equal to generate_many, both at the oracle."""
    import torch

    from cfdbench_amd.rollout import FnoRollout
    from oracle import fno_oracle as O

    L, steps = 2, 3
    model, params = _model()
    batch = CK.make_batch(53, 3, 66, 65, 5, 3, 3, border=True)
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    with torch.no_grad():
        frames = model.generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
        gframes = FnoRollout(model).generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
    torch.cuda.synchronize()
    b64 = {k: v.astype(np.float64) for k, v in batch.items()}
    rframes = O.generate_many(_p64(params), b64["inputs"], b64["case_params"], b64["mask"], steps, num_layers=L)
    assert len(frames) == len(gframes) == steps
    for a, b, r in zip(frames, gframes, rframes):
        assert torch.equal(a, b)
        assert O.rel_nmse(a.cpu().numpy(), r) < K.TOL


def test_fno_train_engine_chan_is_deterministic():
    """Two FnoTrainEngines from the same state, the same two steps -> bitwise-equal parameters; gradients() is the loss's own."""
    import torch

    from cfdbench_amd.engine import FnoTrainEngine
    from oracle import fno_oracle as O

    outs, grads = [], []
    batch = CK.make_batch(54, 4, 64, 64, 5, 3, 3, border=True)
    for _ in range(2):
        model, params = _model()
        eng = FnoTrainEngine(model, lr=1e-3, loss_name="nmse")
        b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
        grads.append(eng.gradients().detach().clone())
        eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
        torch.cuda.synchronize()
        outs.append({k: v.detach().clone() for k, v in model.state_dict().items()})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    assert torch.equal(grads[0], grads[1])
    # the first step's gradient in the loss's own units: its norm over all tensors against the oracle's
    _m, params = _model()
    b64 = {k: v.astype(np.float64) for k, v in batch.items()}
    ref = O.fno_forward(_p64(params), b64["inputs"], b64["case_params"], b64["mask"], b64["label"], 2)
    rg = O.fno_backward(_p64(params), ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], "nmse"), 2)
    got = float(torch.linalg.vector_norm(grads[0].double()).item())  # (the padding between the flat buffer's tensors is zero)
    want = float(np.sqrt(sum(np.sum(np.abs(v) ** 2) for k, v in rg.items() if k in params)))
    assert abs(got - want) < 1e-5 * want, (got, want)


def test_train_auto_chan_fused_and_autograd(tmp_path):
    """train_auto with --in_chan 3 --out_chan 3 on SyntheticAutoDataset(n_fields=3), autograd (--fused 0) and fused (--fused 1): one
    epoch, artefacts written, then test; the two paths' per-step losses agree."""
    import torch

    from cfdbench_amd.harness.args import Args
    from cfdbench_amd.harness.autoregressive import init_model
    from cfdbench_amd.harness.common import get_output_dir
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.harness.train_auto import test, train

    losses = {}
    for fused in (0, 1):
        args = Args(model="fno", data_name="cavity_bc", loss_name="nmse", fno_hidden_dim=20, fno_depth=2, lr=1e-3, in_chan=3, out_chan=3,
                    output_dir=str(tmp_path / f"f{fused}"), num_epochs=1, batch_size=4, eval_batch_size=4, eval_interval=1,
                    log_interval=5, plot_interval=0, fused=fused)
        out = get_output_dir(args, is_auto=True)
        tr = SyntheticAutoDataset(n_cases=4, n_frames=4, height=64, width=64, seed=0, n_fields=3)
        dev = SyntheticAutoDataset(n_cases=2, n_frames=4, height=64, width=64, seed=1, n_fields=3)
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


def test_fno2d_chan_vs_reference_golden():
    """The reference's own Fno2d(3, 3) (tools/make_golden_chan.py): predictions, the four losses and sampled gradient entries."""
    import torch

    from oracle import fno_oracle as O

    g = np.load(Path(__file__).resolve().parent / "golden" / "fno_c3_64x64.npz")
    pseed, bseed, B, C, L, H, W, p, border, cin, cout = [int(v) for v in g["meta"]]
    model, _params = _model(cin, cout, C, L, p, pseed, float(g["gain"]))
    batch = CK.make_batch(bseed, B, H, W, p, cin, cout, bool(border))
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
