"""MI355X: the torch boundary (cfdbench_amd/functional.py and the models on top) on tensors that are not fresh contiguous allocations.
functional._f32c() passes a contiguous view through without a copy, so its data_ptr() reaches the C ABI at whatever alignment the
storage offset leaves (include/cfdbench_amd.h, "Alignment"); anything non-contiguous is copied first.  Per model family, forward and
backward with
  (a) every tensor input a contiguous view one element into a larger buffer,
  (d) every parameter rebound to a view at an odd float offset (complex: 8 bytes off the 16-byte grid) of one flat buffer,
  (e) every input a batch slice big[1 : 1 + B],
      -- these must meet the tolerance against the reference's golden outputs that the family's own test uses (tests/test_gpu_model.py,
      test_gpu_fno_wide.py, test_gpu_fno_chan.py) --
  (b) non-contiguous inputs (channels_last / a channel slice of a wider tensor / transposed storage),
  (c) the upstream gradient of preds.sum() (expanded, stride 0) and a sliced one,
      -- these are copied by _f32c and must equal the run on fresh contiguous clones bit for bit.
No case may raise: where the C ABI refuses a placement the wrapper takes its other route (ConvTransposeCatFn.supported, DropoutGeluFn).
The autograd.Function classes of functional.py that the graphs of these runs contain are collected; the last test fails on any that no
run reached."""
from pathlib import Path

import numpy as np
import pytest

from oracle import fno_oracle as O
from oracle import synth
from tests import chan_checks as CK

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
SEEN = set()  # names of the custom autograd nodes the runs below went through


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---- placements ---------------------------------------------------------------------------------------------------------
def offset_view(torch, t):
    """`t` as a contiguous view one element into a larger buffer (4 bytes off for float32)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() + t.element_size()
    return v


def batch_slice(torch, t):
    big = torch.cat([t[-1:], t, t[:1]], dim=0)
    v = big[1:1 + t.shape[0]]
    assert v.is_contiguous() and v.storage_offset() == t[0].numel()
    return v


def non_contiguous(torch, t):
    """channels_last for images, a channel slice of a wider tensor for one-channel images, transposed storage for matrices."""
    if t.dim() == 4 and t.shape[1] > 1 and t.shape[2] * t.shape[3] > 1:
        v = t.contiguous(memory_format=torch.channels_last)
    elif t.dim() == 4 and t.shape[1] > 1:  # (a 1 x 1 kernel: channels_last is the same layout -- a slice of a wider last dimension)
        v = torch.cat([t, t], dim=3)[:, :, :, :1]
    elif t.dim() == 4:
        v = torch.cat([t, t], dim=1)[:, 1:]
        v = torch.cat([v, v], dim=3)[:, :, :, :t.shape[3]]
    elif t.dim() == 2 and min(t.shape) > 1:
        v = t.t().contiguous().t()
    else:
        return t
    assert not v.is_contiguous() and torch.equal(v, t)
    return v


def rebind_parameters(torch, m):
    """Every parameter becomes a view into ONE flat float32 buffer: real tensors one float, complex tensors two floats past a 16-byte
    boundary (a flat training buffer whose layout does not pad to 16 bytes)."""
    ps = list(m.parameters())
    floats = lambda p: p.numel() * (2 if p.is_complex() else 1)  # noqa: E731
    flat = torch.empty(sum(floats(p) + 8 for p in ps) + 8, dtype=torch.float32, device="cuda")
    assert flat.data_ptr() % 16 == 0
    off = 0
    for p in ps:
        off = (off + 3) // 4 * 4 + (2 if p.is_complex() else 1)
        seg = flat[off:off + floats(p)]
        v = torch.view_as_complex(seg.view(*p.shape, 2)) if p.is_complex() else seg.view(p.shape)
        v.copy_(p.data)
        p.data = v
        assert p.data_ptr() % 16 == (8 if p.is_complex() else 4)
        off += floats(p)
    return flat


def walk(root):
    """Names of the custom Function nodes of the graph under `root` (e.g. 'FnoForwardFnBackward' -> 'FnoForwardFn')."""
    seen, todo = set(), [root.grad_fn]
    while todo:
        n = todo.pop()
        if n is None or n in seen:
            continue
        seen.add(n)
        name = type(n).__name__
        if name.endswith("FnBackward"):
            SEEN.add(name[:-len("Backward")])
        todo.extend(f for f, _ in n.next_functions)


# ---- the families: build() -> (model, forward kwargs, name of the input that takes a gradient, golden, tolerances) -----------------
def _fno(name, cin=2, cout=2):
    def build(torch):
        from cfdbench_amd.models.fno.fno2d import Fno2d
        from cfdbench_amd.models.loss import loss_name_to_fn
        g = np.load(GOLDEN / f"{name}.npz")
        pseed, bseed, B, C, L, H, W, p, border = [int(v) for v in g["meta"][:9]]
        if (cin, cout) == (2, 2):
            params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=float(g["gain"]))
            batch = synth.make_batch(bseed, B, H, W, p, border_mask=bool(border))
        else:
            params = CK.make_params(pseed, C, L, 12, 12, p, cin, cout, float(g["gain"]))
            batch = CK.make_batch(bseed, B, H, W, p, cin, cout, bool(border))
        m = Fno2d(cin, cout, p, loss_name_to_fn("nmse"), L, 12, 12, C).cuda()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
        kw = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
        return m, kw, None, g, dict(preds=1e-9 if name.startswith("fno_small") else 1e-10, grad=1e-8, gsum=1e-6, loss=5e-6)
    return build


def _sd_model(name, make, batch_of, xgrad="inputs", tols=None, extra=None, train=False):
    def build(torch):
        g = np.load(GOLDEN / f"{name}.npz")
        m = make(g).cuda()
        sd = {k[len("sd::"):]: torch.from_numpy(np.ascontiguousarray(g[k])) for k in g.files if k.startswith("sd::")}
        m.load_state_dict(sd)
        m.train(train)
        kw = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in batch_of(g).items()}
        return m, kw, xgrad, g, dict(tols or dict(preds=1e-9, grad=1e-7, loss=1e-5))
    return build


def _unet(name):
    def make(g):
        from cfdbench_amd.models.loss import loss_name_to_fn
        from cfdbench_amd.models.unet import UNet
        dim, p = int(g["meta"][5]), int(g["meta"][6])
        return UNet(2, 2, loss_name_to_fn("nmse"), p, insert_case_params_at="hidden" if "hidden" in name else "input",
                    bilinear="bilinear" in name, dim=dim)

    def batch_of(g):
        seed, bseed, B, H, W, dim, p, steps = [int(v) for v in g["meta"]]
        b = synth.make_smooth_batch(bseed, B, H, W, p)
        b["mask"][:, :, 0, :] = 0
        b["mask"][:, :, :, 0] = 0
        return b
    return _sd_model(name, make, batch_of, train=True, tols=dict(preds=1e-9, grad=1e-7, loss=1e-5, preds_key="preds_train", tiny=1e-7))


def _resnet():
    def make(g):
        from cfdbench_amd.models.loss import loss_name_to_fn
        from cfdbench_amd.models.resnet import ResNet
        seed, bseed, B, H, W, hidden, nblocks, p, steps = [int(v) for v in g["meta"]]
        return ResNet(2, 2, p, loss_name_to_fn("nmse"), hidden_chan=hidden, num_blocks=nblocks, kernel_size=7, padding=3)

    def batch_of(g):
        seed, bseed, B, H, W, hidden, nblocks, p, steps = [int(v) for v in g["meta"]]
        b = synth.make_smooth_batch(bseed, B, H, W, p)
        b["mask"][:, :, -1, :] = 0
        return b
    return _sd_model("resnet_h4_20x24", make, batch_of)


def _auto_deeponet(name):
    def build(torch):
        from cfdbench_amd.models.auto_deeponet import AutoDeepONet
        from cfdbench_amd.models.loss import loss_name_to_fn
        from oracle import deeponet_oracle as D
        g = np.load(GOLDEN / f"{name}.npz")
        pseed, bseed, B, H, W, width, bdepth, tdepth, p, steps = [int(v) for v in g["meta"]]
        m = AutoDeepONet(H * W + p, 2, loss_name_to_fn("nmse"), branch_depth=bdepth, trunk_depth=tdepth, width=width, act_name=str(g["act"])).cuda()
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in D.make_params(pseed, H * W + p, width, bdepth, tdepth).items()})
        kw = {k: torch.from_numpy(v).cuda() for k, v in synth.make_smooth_batch(bseed, B, H, W, p).items()}
        return m, kw, "inputs", g, dict(preds=1e-9, grad=1e-8, loss=1e-5)
    return build


def _auto_q(name):
    def make(g):
        from cfdbench_amd.models.auto_edeeponet import AutoEDeepONet
        from cfdbench_amd.models.auto_ffn import AutoFfn
        from cfdbench_amd.models.loss import loss_name_to_fn
        seed, bseed, B, H, W, width, depth, p, steps, nq = [int(v) for v in g["meta"]]
        if str(g["kind"]) == "auto_edeeponet":
            return AutoEDeepONet(H * W, p, 2, loss_name_to_fn("nmse"), branch_depth=depth, trunk_depth=depth, width=width, act_name=str(g["act"]))
        return AutoFfn(H * W, p, 2, loss_name_to_fn("nmse"), depth=depth, width=width, act_name=str(g["act"]))

    def batch_of(g):
        seed, bseed, B, H, W, width, depth, p, steps, nq = [int(v) for v in g["meta"]]
        return dict(synth.make_smooth_batch(bseed, B, H, W, p), query_idxs=g["q"])
    return _sd_model(name, make, batch_of)


def _deeponet_cnn():
    def make(g):
        from cfdbench_amd.models.auto_deeponet_cnn import AutoDeepONetCnn
        from cfdbench_amd.models.loss import loss_name_to_fn
        seed, bseed, B, trunk_depth, p, steps, nq = [int(v) for v in g["meta"]]
        return AutoDeepONetCnn(2, 2, loss_name_to_fn("nmse"), height=64, width=64, num_case_params=p, trunk_depth=trunk_depth)

    def batch_of(g):
        seed, bseed, B, trunk_depth, p, steps, nq = [int(v) for v in g["meta"]]
        b = synth.make_smooth_batch(bseed, B, 64, 64, p)
        b["mask"][:, :, 0, :] = 0
        return dict(b, query_idxs=g["q"])
    return _sd_model("auto_deeponet_cnn_64x64", make, batch_of, tols=dict(preds=1e-9, grad=1e-7, loss=1e-4))


def _deeponet(name):
    def make(g):
        from cfdbench_amd.models.deeponet import DeepONet
        from cfdbench_amd.models.ffn import FfnModel
        from cfdbench_amd.models.loss import loss_name_to_fn
        seed, B, K_, H, W, width, p, act_norm = [int(v) for v in g["meta"]]
        if str(g["kind"]) == "deeponet":
            return DeepONet(p, 3, loss_name_to_fn("nmse"), branch_depth=3, trunk_depth=3, width=width, act_name=str(g["act"]), act_norm=bool(act_norm))
        return FfnModel(loss_name_to_fn("nmse"), [p + 3, width, width, 1], act_name=str(g["act"]), act_norm=bool(act_norm))

    def batch_of(g):
        return dict(case_params=g["cp"], t=g["t"], label=g["label"], query_idxs=g["q"])
    return _sd_model(name, make, batch_of, xgrad=None)


FAMILIES = {
    "fno": _fno("fno_small_64x64"), "fno_66x65": _fno("fno_small_66x65"), "fno_wide": _fno("fno_w64_64x64"), "fno_chan": _fno("fno_c3_64x64", 3, 3),
    "unet": _unet("unet_dim4_32x32"), "unet_bilinear": _unet("unet_bilinear_dim4_32x48"), "unet_hidden": _unet("unet_hidden_dim2_32x32"), "resnet": _resnet(),
    "auto_deeponet": _auto_deeponet("auto_deeponet_small_16x16"), "auto_ffn": _auto_q("auto_ffn_relu_16x18"),
    "auto_edeeponet": _auto_q("auto_edeeponet_relu_16x18"), "auto_deeponet_cnn": _deeponet_cnn(), "deeponet": _deeponet("deeponet_normact_relu"),
    "ffn_model": _deeponet("ffnmodel_normact_gelu"),
}


def run(torch, family, place=None, rebind=False, upstream=None):
    """One forward + backward of a family on transformed inputs; returns (predictions, loss, {name: gradient}, golden, tolerances)."""
    m, kw, xgrad, g, tols = FAMILIES[family](torch)
    flat = rebind_parameters(torch, m) if rebind else None
    if place is not None:
        kw = {k: place(torch, v) for k, v in kw.items()}
    if xgrad:
        leaf = kw[xgrad].detach().clone().requires_grad_(True)
        kw[xgrad] = leaf if place is None else place(torch, leaf)  # (a differentiable view / copy of the leaf: the gradient flows back)
    out = m(**kw)
    preds = out["preds"]
    if upstream is None:
        walk(out["loss"]["nmse"])
        out["loss"]["nmse"].backward()
    else:
        walk(preds)
        upstream(torch, preds)
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    if xgrad:
        grads["g_inputs"] = leaf.grad.detach().clone()
    del flat
    return preds.detach().clone(), out["loss"]["nmse"].item(), grads, g, tols


def assert_golden(preds, loss, grads, g, tols):
    assert O.rel_nmse(preds.cpu().numpy().reshape(g[tols.get("preds_key", "preds")].shape), g[tols.get("preds_key", "preds")]) < tols["preds"]
    assert abs(loss - float(g["loss_nmse"])) <= tols["loss"] * abs(float(g["loss_nmse"]))
    n = 0
    for k, got in grads.items():
        key = "g_inputs" if k == "g_inputs" else f"grad::{k}"
        if key in g.files:
            ref = g[key]
            if "tiny" in tols and np.abs(ref).max() < tols["tiny"]:  # conv bias in front of a train-mode BatchNorm: the exact gradient is zero
                assert float(got.abs().max()) < 1e-6, k
            else:
                assert O.rel_nmse(got.cpu().numpy(), ref) < tols["grad"], k
            n += 1
        elif f"gsum::{k}::vals" in g.files:  # sampled entries of the reference's fp32 gradient (tests/test_gpu_fno_wide.py)
            assert O.rel_nmse(got.cpu().numpy().reshape(-1)[g[f"gsum::{k}::idx"]], g[f"gsum::{k}::vals"]) < tols["gsum"], k
            n += 1
    assert n >= len(grads) - 1, (n, sorted(grads))


def assert_bitwise(a, b):
    assert torch_equal(a[0], b[0]), "predictions differ"
    assert a[1] == b[1], (a[1], b[1])
    assert a[2].keys() == b[2].keys()
    for k in a[2]:
        assert torch_equal(a[2][k], b[2][k]), k


def torch_equal(x, y):
    import torch
    return torch.equal(x, y)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_fresh_contiguous_inputs_meet_the_golden(torch, family):
    """The harness of this file on plain inputs: what (a), (d) and (e) are then held to."""
    assert_golden(*run(torch, family))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_a_inputs_one_element_into_a_larger_buffer(torch, family):
    assert_golden(*run(torch, family, place=offset_view))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_d_parameters_at_odd_offsets_of_a_flat_buffer(torch, family):
    assert_golden(*run(torch, family, rebind=True))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_e_inputs_as_a_batch_slice(torch, family):
    assert_golden(*run(torch, family, place=batch_slice))


def test_e_batch_slice_of_66x65_images_with_three_channels(torch):
    """big[1 : 1 + B] of 66 x 65 images with an odd channel count: one sample is 3 * 66 * 65 * 4 = 51480 bytes (the mask: 17160), so inputs,
    label and mask sit 8 bytes off the 16-byte grid and case_params 4.  Fno2d(3, 3) under autograd, generate_many and FnoRollout against
    the fp64 oracle at the bounds of tests/test_gpu_fno_chan.py (test_fno2d_chan_autograd_vs_oracle, test_rollout_chan_graph_vs_eager_vs_oracle)."""
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    from cfdbench_amd.rollout import FnoRollout
    from tests.kernel_checks import TOL
    B, C, L, H, W, p, steps = 3, 20, 2, 66, 65, 5, 3
    params = CK.make_params(51, C, L, 12, 12, p, 3, 3, 4.0)
    batch = CK.make_batch(52, B, H, W, p, 3, 3, border=True)
    m = Fno2d(3, 3, p, loss_name_to_fn("nmse"), L, 12, 12, C).cuda()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    tb = {k: batch_slice(torch, torch.from_numpy(v).cuda()) for k, v in batch.items()}
    for k in ("inputs", "label", "mask"):
        assert tb[k].data_ptr() % 16 == 8, (k, tb[k].data_ptr() % 16)
    assert tb["case_params"].data_ptr() % 16 == 4
    out = m(**tb)
    walk(out["loss"]["nmse"])
    out["loss"]["nmse"].backward()
    with torch.no_grad():
        frames = m.generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
        gframes = FnoRollout(m).generate_many(tb["inputs"], tb["case_params"], tb["mask"], steps)
    p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in params.items()}
    b64 = {k: v.astype(np.float64) for k, v in batch.items()}
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
    rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], "nmse"), L)
    assert O.rel_nmse(out["preds"].detach().cpu().numpy(), ref["preds"]) < TOL
    assert abs(out["loss"]["nmse"].item() - ref["loss"]["nmse"]) < 1e-5 * ref["loss"]["nmse"]
    for k, prm in m.named_parameters():
        assert O.rel_nmse(prm.grad.cpu().numpy(), rg[k]) < 1e-9, k
    rframes = O.generate_many(p64, b64["inputs"], b64["case_params"], b64["mask"], steps, num_layers=L)
    assert len(frames) == len(gframes) == steps
    for a, c, r in zip(frames, gframes, rframes):
        assert torch.equal(a, c)
        assert O.rel_nmse(a.cpu().numpy(), r) < TOL


@pytest.mark.parametrize("family", list(FAMILIES))
def test_b_non_contiguous_inputs_equal_their_contiguous_clones(torch, family):
    assert_bitwise(run(torch, family, place=non_contiguous), run(torch, family))


def _expanded(torch, preds):
    preds.sum().backward()


def _ones(torch, preds):
    preds.backward(torch.ones_like(preds).contiguous())


def _weights(torch, preds):
    gen = torch.Generator(device="cuda").manual_seed(7)
    return torch.randn(preds.shape[:-1] + (preds.shape[-1] + 1,), device="cuda", generator=gen)


def _sliced(torch, preds):
    g = _weights(torch, preds)[..., 1:]
    assert not g.is_contiguous() or preds.dim() == 1
    preds.backward(g)


def _sliced_clone(torch, preds):
    preds.backward(_weights(torch, preds)[..., 1:].clone())


@pytest.mark.parametrize("family", list(FAMILIES))
def test_c_expanded_and_sliced_upstream_gradients_equal_contiguous_ones(torch, family):
    assert_bitwise(run(torch, family, upstream=_expanded), run(torch, family, upstream=_ones))
    assert_bitwise(run(torch, family, upstream=_sliced), run(torch, family, upstream=_sliced_clone))


# ---- MseLoss and the rollout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", [None, offset_view, batch_slice, non_contiguous], ids=["plain", "a", "e", "b"])
def test_mseloss_on_views(torch, place):
    from cfdbench_amd.models.loss import MseLoss
    g = np.load(GOLDEN / "mseloss.npz")
    rng = np.random.default_rng(int(g["meta"][0]))
    p = rng.standard_normal((3, 2, 17, 19)).astype(np.float32)
    l = rng.standard_normal((3, 2, 17, 19)).astype(np.float32)
    leaf = torch.from_numpy(p).cuda().requires_grad_(True)
    pt, lt = leaf, torch.from_numpy(l).cuda()
    if place is not None:
        pt, lt = place(torch, leaf), place(torch, lt)
    r = MseLoss(normalize=True)(preds=pt, labels=lt)
    for k in ("mse", "rmse", "mae", "nmse"):
        assert abs(r[k].item() - float(g[k])) < 2e-6 * abs(float(g[k]))
    walk(r["nmse"])
    r["nmse"].backward()
    assert O.rel_nmse(leaf.grad.cpu().numpy(), O.loss_grad_wrt_preds(p.astype(np.float64), l.astype(np.float64), "nmse")) < 1e-10


@pytest.mark.parametrize("place", [None, offset_view, batch_slice, non_contiguous, "rebind"], ids=["plain", "a", "e", "b", "d"])
@pytest.mark.parametrize("name", ["rollout_small_64x64", "rollout_small_66x65"])
def test_rollout_on_views(torch, name, place):
    """generate_many and FnoRollout (which captures the parameter pointers into a HIP graph); "d": the parameters rebound to views at odd
    offsets of a flat buffer before the graph is captured."""
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    from cfdbench_amd.rollout import FnoRollout
    g = np.load(GOLDEN / f"{name}.npz")
    pseed, bseed, B, C, L, H, W, p, steps, border = [int(v) for v in g["meta"]]
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=float(g["gain"]))
    batch = synth.make_smooth_batch(bseed, B, H, W, p)
    if border:
        batch["mask"][:, :, 0, :] = 0
        batch["mask"][:, :, -1, :] = 0
        batch["mask"][:, :, :, 0] = 0
    m = Fno2d(2, 2, p, loss_name_to_fn("nmse"), L, 12, 12, C).cuda().eval()
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    b = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    flat = None
    if place == "rebind":
        flat = rebind_parameters(torch, m)
        assert all(p.data_ptr() % 16 for p in m.parameters()) and flat.data_ptr() % 16 == 0
    elif place is not None:
        b = {k: place(torch, v) for k, v in b.items()}
    with torch.no_grad():
        for frames in (m.generate_many(b["inputs"], b["case_params"], b["mask"], steps),
                       FnoRollout(m).generate_many(b["inputs"], b["case_params"], b["mask"], steps)):
            assert len(frames) == steps
            assert O.rel_nmse(frames[0].cpu().numpy(), g["first"]) < 1e-9
            assert O.rel_nmse(frames[-1].cpu().numpy(), g["last"]) < 1e-7


# ---- the transposed convolution's two routes: the C ABI refuses, the wrappers do not raise ------------------------------------
def test_convtranspose_wrappers_take_views(torch):
    """ConvTransposeCatFn.supported() sends a contiguous x off the 16-byte grid to ConvTranspose2x2Fn + torch.cat (cfd_convt2_bwd_ex
    takes `in` at 16 bytes only); an upstream gradient off the grid is copied by both backward passes (cfd_convt2_bwd: 8 bytes)."""
    from cfdbench_amd import functional as F_
    gen = torch.Generator(device="cuda").manual_seed(3)
    B, Ci, Co, H, W = 2, 8, 4, 8, 8
    x, w, b = (torch.randn(s, device="cuda", generator=gen) for s in ((B, Ci, H, W), (Ci, Co, 2, 2), (Co,)))
    skip = torch.randn((B, 3, 2 * H, 2 * W), device="cuda", generator=gen)
    gcat = torch.randn((B, 3 + Co, 2 * H, 2 * W), device="cuda", generator=gen)
    assert F_.ConvTransposeCatFn.supported(x, w, skip)
    assert not F_.ConvTransposeCatFn.supported(offset_view(torch, x), w, skip)
    assert not F_.ConvTransposeCatFn.supported(x, offset_view(torch, w), skip)
    assert F_.ConvTransposeCatFn.supported(non_contiguous(torch, x), w, skip)  # (copied: the copy is aligned)

    def grads(fn, xin, g):
        xl, wl, bl = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
        out = fn(xin(xl), wl, bl)
        walk(out)
        out.backward(g)
        return out.detach(), xl.grad, wl.grad, bl.grad
    cat = lambda xx, ww, bb: F_.ConvTransposeCatFn.apply(xx, ww, bb, skip)  # noqa: E731
    two = lambda xx, ww, bb: torch.cat([skip, F_.ConvTranspose2x2Fn.apply(xx, ww, bb)], dim=1)  # noqa: E731
    ident = lambda t: t  # noqa: E731
    ref = grads(two, ident, gcat)
    for fn, xin, g in ((cat, ident, gcat), (cat, ident, offset_view(torch, gcat)), (two, lambda t: offset_view(torch, t), gcat),
                       (two, ident, offset_view(torch, gcat)), (cat, lambda t: non_contiguous(torch, t), gcat)):
        got = grads(fn, xin, g)
        assert torch.equal(got[0], ref[0])
        for a, c in zip(got[1:], ref[1:]):  # (the strided and the dense route sum in different orders: fp32 round-off)
            assert O.rel_nmse(a.cpu().numpy(), c.cpu().numpy()) < 1e-10


def test_dropout_gelu_takes_views(torch):
    """DropoutGeluFn on an x / an upstream gradient off the 16-byte grid: the two-pass route, value for value the fused one."""
    from cfdbench_amd.functional import DropoutGeluFn
    gen = torch.Generator(device="cuda").manual_seed(4)
    x, g = torch.randn(4 * 1031, device="cuda", generator=gen), torch.randn(4 * 1031, device="cuda", generator=gen)
    res = []
    for xin, gin in ((x, g), (offset_view(torch, x), g), (x, offset_view(torch, g)), (offset_view(torch, x), offset_view(torch, g))):
        leaf = xin.detach().requires_grad_(True)
        y = DropoutGeluFn.apply(leaf, 0.2, 1234)
        walk(y)
        y.backward(gin)
        res.append((y.detach().clone(), leaf.grad.clone()))
    for y, gx in res[1:]:
        assert torch.equal(y, res[0][0]) and torch.equal(gx, res[0][1])


# ---- the Functions no model above goes through, against the same operation of torch in float64 ------------------------------------
def _direct(torch, fn, ref, shapes, tol, seed, complex_at=()):
    """fn(*inputs) and its gradients on plain tensors, on views one element into a buffer (upstream gradient too) and on non-contiguous
    inputs, each against ref(*inputs in float64) under autograd; the non-contiguous run equals the plain one bit for bit."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    base = [torch.randn(sh, device="cuda", generator=gen, dtype=torch.complex64 if i in complex_at else torch.float32)
            for i, sh in enumerate(shapes)]
    l64 = [t.to(torch.complex128 if t.is_complex() else torch.float64).requires_grad_(True) for t in base]
    want = ref(*l64)
    gup = torch.randn(want.shape, device="cuda", generator=gen)
    want.backward(gup.double())
    runs = {}
    for name, place in (("plain", None), ("a", offset_view), ("b", non_contiguous)):
        leaves = [t.clone().requires_grad_(True) for t in base]
        out = fn(*[t if place is None else place(torch, t) for t in leaves])
        walk(out)
        out.backward(gup if place is None else place(torch, gup))
        runs[name] = [out.detach()] + [t.grad for t in leaves]
        for got, ref_t in zip(runs[name], [want] + [t.grad for t in l64]):
            assert O.rel_nmse(got.cpu().numpy(), ref_t.detach().cpu().numpy()) < tol, name
    for a, c in zip(runs["b"], runs["plain"]):
        assert torch.equal(a, c)


def test_gelu_batchnorm_zero_padded_conv_and_dropout_on_views(torch):
    """GeluFn, BatchNormFn (training, with ReLU), Conv2dZeroPadFn and DropoutFn; 1e-10 is the kernel checks' bound for these entry points
    (tests/kernel_checks.py: TOL)."""
    from cfdbench_amd import functional as F_
    Fn = torch.nn.functional
    _direct(torch, F_.GeluFn.apply, Fn.gelu, [(3, 5, 8, 8)], 1e-10, 11)
    C = 5

    def bn(x, gamma, beta):
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        return F_.BatchNormFn.apply(x, gamma, beta, rm, rv, True, True, 1e-5, 0.1)
    _direct(torch, bn, lambda x, ga, be: Fn.relu(Fn.batch_norm(x, None, None, ga, be, True, 0.1, 1e-5)), [(4, C, 8, 8), (C,), (C,)], 1e-10, 12)
    x, w = torch.empty((3, 8, 6, 6), device="cuda"), torch.empty((7, 8, 3, 3), device="cuda")
    assert F_.Conv2dZeroPadFn.supported(x, w)
    _direct(torch, F_.Conv2dZeroPadFn.apply, lambda xx, ww, bb: Fn.conv2d(xx, ww, bb, padding=1),
            [(3, 8, 6, 6), (7, 8, 3, 3), (7,)], 1e-10, 13)
    # dropout: the mask is a hash of (seed, element index), so every placement keeps the same elements
    gen = torch.Generator(device="cuda").manual_seed(14)
    z, g = torch.randn((2, 3, 8, 8), device="cuda", generator=gen), torch.randn((2, 3, 8, 8), device="cuda", generator=gen)
    res = []
    for place in (None, offset_view, non_contiguous):
        leaf = z.clone().requires_grad_(True)
        y = F_.DropoutFn.apply(leaf if place is None else place(torch, leaf), 0.2, 1234)
        walk(y)
        y.backward(g if place is None else place(torch, g))
        res.append((y.detach(), leaf.grad))
    assert torch.equal(res[0][0] != 0, res[0][1] != 0) and torch.allclose(res[0][0][res[0][0] != 0], (z / 0.8)[res[0][0] != 0])
    for y, gx in res[1:]:
        assert torch.equal(y, res[0][0]) and torch.equal(gx, res[0][1])


def _spectral64(torch, x, w1, w2):
    """SpectralConv2d_fast in the input's precision: rfft2, the two corner blocks of modes times their weights, irfft2."""
    m1, m2 = w1.shape[2:]
    xf = torch.fft.rfft2(x)
    of = torch.zeros(x.shape[0], w1.shape[1], x.shape[2], x.shape[3] // 2 + 1, dtype=xf.dtype, device=x.device)
    of[:, :, :m1, :m2] = torch.einsum("bixy,ioxy->boxy", xf[:, :, :m1, :m2], w1)
    of[:, :, -m1:, :m2] = torch.einsum("bixy,ioxy->boxy", xf[:, :, -m1:, :m2], w2)
    return torch.fft.irfft2(of, s=x.shape[2:])


def test_spectral_conv_and_fno_block_functions_on_views(torch):
    """SpectralConv2dFn and FnoBlockFn (the stand-alone modules SpectralConv2d_fast and FnoBlock; Fno2d itself runs FnoForwardFn): x, the
    complex weights (8 bytes off the grid), the 1 x 1 convolution and the upstream gradient as views, against torch in float64.  32 x 32
    keeps H W % 4 == 0, so the pointer alone decides the route; 1e-10 is the kernel checks' bound (tests/kernel_checks.py: TOL)."""
    from cfdbench_amd import functional as F_
    Fn = torch.nn.functional
    B, Ci, Co, H, W, m = 2, 3, 5, 32, 32, 12
    _direct(torch, F_.spectral_conv2d, lambda x, w1, w2: _spectral64(torch, x, w1, w2),
            [(B, Ci, H, W), (Ci, Co, m, m), (Ci, Co, m, m)], 1e-10, 21, complex_at=(1, 2))
    for gelu in (True, False):
        def ref(x, w1, w2, w0, b0):
            y = _spectral64(torch, x, w1, w2) + Fn.conv2d(x, w0, b0)
            return Fn.gelu(y) if gelu else y
        _direct(torch, lambda *a: F_.fno_block(*a, gelu=gelu), ref,
                [(B, Ci, H, W), (Ci, Co, m, m), (Ci, Co, m, m), (Co, Ci, 1, 1), (Co,)], 1e-10, 22, complex_at=(1, 2))


def test_two_node_loss_functions_on_views(torch):
    """LossSumsFn + LossScoresFn (scores_from_sums), the two-node form of the loss: predictions, labels and the four score gradients as
    views, against loss.py's formulas in float64.  The sums are fp32 accumulations of 3 * 2 * 16 * 18 terms: 1e-10 in relative squared
    error is (1e-5)^2, the bound the loss tests of this suite put on a score."""
    from cfdbench_amd import functional as F_

    def fn(p, l):
        return torch.stack(list(F_.scores_from_sums(F_.LossSumsFn.apply(p, l), True).values()))

    def ref(p, l):
        mse = ((p - l) ** 2).mean()
        return torch.stack([mse, mse.sqrt(), (p - l).abs().mean(), mse / (l * l).mean()])
    _direct(torch, fn, ref, [(3, 2, 16, 18), (3, 2, 16, 18)], 1e-10, 23)


def test_zz_which_functions_the_runs_reached():
    """Every autograd.Function of functional.py sits in the graph of at least one run above."""
    import inspect

    import torch

    from cfdbench_amd import functional as F_
    if not SEEN:
        pytest.fail("runs after the tests above (same module): nothing was collected")
    classes = {n for n, c in inspect.getmembers(F_, inspect.isclass) if issubclass(c, torch.autograd.Function) and c.__module__ == F_.__name__}
    missing = sorted(classes - SEEN)
    assert not missing, f"autograd.Functions no view test reached: {missing} (reached: {sorted(SEEN)})"
