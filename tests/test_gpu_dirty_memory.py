"""MI355X: the Python boundary on a poisoned caching allocator.  The product allocates outputs and workspaces with torch.empty; here
every model family, the training engine and the captured rollout run once in a clean state and once after every free byte of the
allocator has been filled with NaN (tests/dirty_memory.py, which proves that the poison landed), from the same state_dict and inputs:
predictions, losses, every gradient and the trained parameters must be bitwise equal and finite.  The goldens pin the clean run's
values (tests/test_gpu_model.py and friends), so nothing here has a tolerance."""
import numpy as np
import pytest

from oracle import synth
from tests.dirty_memory import poison_caching_allocator

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _loss():
    from cfdbench_amd.models.loss import loss_name_to_fn
    return loss_name_to_fn("nmse")


def _host(t):
    return t.detach().cpu().numpy().copy()


def _clean_then_poisoned(torch, run):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    clean = run()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    poison_caching_allocator(torch, peak)
    dirty = run()
    torch.cuda.synchronize()
    assert clean.keys() == dirty.keys() and len(clean) > 0
    bad = {}
    for k, a in clean.items():
        b = dirty[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        n = int(np.count_nonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)))
        if a.dtype.kind in "fc":
            n += int(np.count_nonzero(~np.isfinite(a))) + int(np.count_nonzero(~np.isfinite(b)))
        if n:
            bad[k] = n
    assert not bad, f"bytes that differ between the clean and the poisoned run (+ non-finite values): {bad}"


def _forward_backward(torch, make_model, make_kwargs, train=True):
    """Model forward with the loss, nMSE backward: predictions, the four scores, every parameter gradient, the input gradient, buffers."""
    def run():
        m = make_model()
        m.train() if train else m.eval()
        kw = make_kwargs()
        out = m(**kw)
        out["loss"]["nmse"].backward()
        torch.cuda.synchronize()
        res = {"preds": _host(out["preds"])}
        res.update({f"loss::{k}": _host(v) for k, v in out["loss"].items()})
        res.update({f"grad::{k}": _host(p.grad) for k, p in m.named_parameters() if p.grad is not None})
        res.update({f"buffer::{k}": _host(v) for k, v in m.named_buffers()})
        if "inputs" in kw and kw["inputs"].grad is not None:
            res["g_inputs"] = _host(kw["inputs"].grad)
        return res
    return run


def _sd(torch, g):
    return {k[len("sd::"):]: torch.from_numpy(np.ascontiguousarray(g[k])) for k in g.files if k.startswith("sd::")}


def _fno(torch, params, C, L, p, m1=12, m2=12):
    from cfdbench_amd.models.fno.fno2d import Fno2d
    m = Fno2d(2, 2, p, _loss(), L, m1, m2, C).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    return m


def _batch_kwargs(torch, batch, grad_inputs=True, **extra):
    def make():
        kw = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        if grad_inputs:
            kw["inputs"].requires_grad_(True)
        kw.update({k: v() for k, v in extra.items()})
        return kw
    return make


# name -> (golden whose sizes are used, modes)
FNO_CASES = {
    "default": ("fno_cfg1_b8", None),
    "width32_66x65": ("rollout200_c32_66x65", None),
    "width64": ("fno_w64_64x64", None),
    "modes24x24": ("fno_m32x33_64x64", (24, 24)),
}


@pytest.mark.parametrize("case", sorted(FNO_CASES))
def test_fno2d(torch, golden_dir, case):
    name, modes = FNO_CASES[case]
    pseed, bseed, B, C, L, H, W, p = [int(v) for v in np.load(golden_dir / f"{name}.npz")["meta"][:8]]
    m1, m2 = modes or (12, 12)
    params = synth.make_fno_params(pseed, C, L, m1, m2, p, spectral_gain=4.0)
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=True)
    _clean_then_poisoned(torch, _forward_backward(torch, lambda: _fno(torch, params, C, L, p, m1, m2), _batch_kwargs(torch, batch, grad_inputs=False)))


def test_unet(torch, golden_dir):
    from cfdbench_amd.models.unet import UNet
    g = np.load(golden_dir / "unet_dim4_32x32.npz")
    seed, bseed, B, H, W, dim, p, steps = [int(v) for v in g["meta"]]
    batch = synth.make_smooth_batch(bseed, B, H, W, p)
    batch["mask"][:, :, 0, :] = 0
    batch["mask"][:, :, :, 0] = 0

    def model():
        m = UNet(2, 2, _loss(), p, insert_case_params_at="input", bilinear=False, dim=dim).cuda()
        m.load_state_dict(_sd(torch, g))
        return m
    _clean_then_poisoned(torch, _forward_backward(torch, model, _batch_kwargs(torch, batch)))


def test_resnet_eval(torch, golden_dir):
    from cfdbench_amd.models.resnet import ResNet
    g = np.load(golden_dir / "resnet_h4_20x24.npz")
    seed, bseed, B, H, W, hidden, nblocks, p, steps = [int(v) for v in g["meta"]]
    batch = synth.make_smooth_batch(bseed, B, H, W, p)
    batch["mask"][:, :, -1, :] = 0

    def model():
        m = ResNet(2, 2, p, _loss(), hidden_chan=hidden, num_blocks=nblocks, kernel_size=7, padding=3).cuda()
        m.load_state_dict(_sd(torch, g))
        return m
    _clean_then_poisoned(torch, _forward_backward(torch, model, _batch_kwargs(torch, batch), train=False))


def test_auto_deeponet(torch, golden_dir):
    from cfdbench_amd.models.auto_deeponet import AutoDeepONet
    from oracle import deeponet_oracle as D
    g = np.load(golden_dir / "auto_deeponet_small_16x16.npz")
    pseed, bseed, B, H, W, width, bdepth, tdepth, p, steps = [int(v) for v in g["meta"]]
    params = D.make_params(pseed, H * W + p, width, bdepth, tdepth)
    batch = synth.make_smooth_batch(bseed, B, H, W, p)

    def model():
        m = AutoDeepONet(H * W + p, 2, _loss(), branch_depth=bdepth, trunk_depth=tdepth, width=width, act_name=str(g["act"])).cuda()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
        return m
    _clean_then_poisoned(torch, _forward_backward(torch, model, _batch_kwargs(torch, batch)))


@pytest.mark.parametrize("name", ["auto_edeeponet_relu_16x18", "auto_ffn_relu_16x18"])
def test_auto_edeeponet_and_auto_ffn(torch, golden_dir, name):
    from cfdbench_amd.models.auto_edeeponet import AutoEDeepONet
    from cfdbench_amd.models.auto_ffn import AutoFfn
    g = np.load(golden_dir / f"{name}.npz")
    seed, bseed, B, H, W, width, depth, p, steps, nq = [int(v) for v in g["meta"]]
    act = str(g["act"])
    batch = synth.make_smooth_batch(bseed, B, H, W, p)

    def model():
        if str(g["kind"]) == "auto_edeeponet":
            m = AutoEDeepONet(H * W, p, 2, _loss(), branch_depth=depth, trunk_depth=depth, width=width, act_name=act).cuda()
        else:
            m = AutoFfn(H * W, p, 2, _loss(), depth=depth, width=width, act_name=act).cuda()
        m.load_state_dict(_sd(torch, g))
        return m
    _clean_then_poisoned(torch, _forward_backward(torch, model, _batch_kwargs(torch, batch, query_idxs=lambda: torch.from_numpy(g["q"]).cuda())))


def test_auto_deeponet_cnn(torch, golden_dir):
    from cfdbench_amd.models.auto_deeponet_cnn import AutoDeepONetCnn
    g = np.load(golden_dir / "auto_deeponet_cnn_64x64.npz")
    seed, bseed, B, trunk_depth, p, steps, nq = [int(v) for v in g["meta"]]
    batch = synth.make_smooth_batch(bseed, B, 64, 64, p)
    batch["mask"][:, :, 0, :] = 0

    def model():
        m = AutoDeepONetCnn(2, 2, _loss(), height=64, width=64, num_case_params=p, trunk_depth=trunk_depth).cuda()
        m.load_state_dict(_sd(torch, g))
        return m
    _clean_then_poisoned(torch, _forward_backward(torch, model, _batch_kwargs(torch, batch, query_idxs=lambda: torch.from_numpy(g["q"]).cuda())))


@pytest.mark.parametrize("name", ["deeponet_normact_relu", "ffnmodel_normact_gelu"])
def test_deeponet_and_ffn_model(torch, golden_dir, name):
    from cfdbench_amd.models.deeponet import DeepONet
    from cfdbench_amd.models.ffn import FfnModel
    g = np.load(golden_dir / f"{name}.npz")
    seed, B, K_, H, W, width, p, act_norm = [int(v) for v in g["meta"]]
    act = str(g["act"])

    def model():
        if str(g["kind"]) == "deeponet":
            m = DeepONet(p, 3, _loss(), branch_depth=3, trunk_depth=3, width=width, act_name=act, act_norm=bool(act_norm)).cuda()
        else:
            m = FfnModel(_loss(), [p + 3, width, width, 1], act_name=act, act_norm=bool(act_norm)).cuda()
        m.load_state_dict(_sd(torch, g))
        return m

    def kwargs():
        cp, t, label, q = (torch.from_numpy(g[k]).cuda() for k in ("cp", "t", "label", "q"))
        return dict(case_params=cp, t=t, label=label, query_idxs=q)
    _clean_then_poisoned(torch, _forward_backward(torch, model, kwargs))


def test_train_engine_two_steps(torch, golden_dir):
    """FnoTrainEngine.train_step twice: the scores of both steps and the flat parameters after them."""
    from cfdbench_amd.engine import FnoTrainEngine
    g = np.load(golden_dir / "adam_small_64x64.npz")
    pseed, bseed, B, C, L, H, W, p, nsteps = [int(v) for v in g["meta"]]
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=float(g["gain"]))

    def run():
        eng = FnoTrainEngine(_fno(torch, params, C, L, p), lr=float(g["lr"]))
        res = {}
        for s in range(2):
            b = {k: torch.from_numpy(v).cuda() for k, v in synth.make_batch(bseed + s, B, H, W, p).items()}
            eng.train_step(b["inputs"], b["label"], b["case_params"], b["mask"])
            res.update({f"step{s}::{k}": np.array([v], np.float64) for k, v in eng.scores().items()})
        torch.cuda.synchronize()
        res["flat"] = _host(eng.flat.data)
        return res
    _clean_then_poisoned(torch, run)


def test_rollout_three_steps(torch, golden_dir):
    """FnoRollout.generate_many (the captured graph over its own ping-pong buffers and workspace), 3 steps."""
    from cfdbench_amd.rollout import FnoRollout
    g = np.load(golden_dir / "rollout_small_64x64.npz")
    pseed, bseed, B, C, L, H, W, p, steps, border = [int(v) for v in g["meta"]]
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=float(g["gain"]))
    batch = synth.make_smooth_batch(bseed, B, H, W, p)

    def run():
        m = _fno(torch, params, C, L, p).eval()
        b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        with torch.no_grad():
            frames = FnoRollout(m).generate_many(b["inputs"], b["case_params"], b["mask"], 3)
        torch.cuda.synchronize()
        return {f"frame{t}": _host(f) for t, f in enumerate(frames)}
    _clean_then_poisoned(torch, run)
