"""CPU: what training through a rollout window needs around the engine -- the flag table (--unroll_steps with --fused 1, --device_loader 1,
--fused_accumulation_steps, --unroll_detach), the resident loader's windows against unroll.collate_windows, the resume record, and
unrolled_loss(detach=True).  The device side is tests/test_gpu_fno_window.py."""
import pytest
import torch

from cfdbench_amd.harness.data import DeviceBatchLoader, SyntheticAutoDataset
from cfdbench_amd.unroll import collate_windows, unroll_windows, unrolled_loss

ACCEPTED = {
    "fused": dict(fused=1, unroll_steps=3),
    "fused_device_loader": dict(fused=1, unroll_steps=4, device_loader=1),
    "eager_device_loader": dict(unroll_steps=3, device_loader=1),
    "fused_accumulation": dict(fused=1, unroll_steps=3, fused_accumulation_steps=2, max_grad_norm=1.0),
    "fused_detach": dict(fused=1, unroll_steps=3, unroll_detach=1),
    "eager_detach": dict(unroll_steps=2, unroll_detach=1),
    "bf16_detach": dict(fused=1, unroll_steps=3, dtype="bf16", unroll_detach=1),
    "one_step": dict(fused=1),
}
REFUSED = {
    "graph": (dict(unroll_steps=3, graph=1), "--graph 1"),
    "bf16_full_gradient": (dict(fused=1, unroll_steps=3, dtype="bf16"), "--unroll_detach 1"),
    "other_model": (dict(model="unet", unroll_steps=3), "fno model"),
    "eager_accumulation": (dict(unroll_steps=3, gradient_accumulation_steps=2), "gradient_accumulation_steps"),
    "detach_without_unroll": (dict(unroll_detach=1), "--unroll_steps > 1"),
    "detach_out_of_range": (dict(unroll_steps=3, unroll_detach=2), "--unroll_detach"),
}


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_is_args_valid_accepts(name):
    from cfdbench_amd.harness.args import Args, is_args_valid
    is_args_valid(Args(**dict(dict(model="fno", data_name="cavity_bc"), **ACCEPTED[name])))


@pytest.mark.parametrize("name", list(REFUSED))
def test_is_args_valid_refuses_with_a_reason(name):
    from cfdbench_amd.harness.args import Args, is_args_valid
    kw, why = REFUSED[name]
    with pytest.raises(AssertionError, match=why):
        is_args_valid(Args(**dict(dict(model="fno", data_name="cavity_bc"), **kw)))


def test_unroll_detach_flag_parses_and_is_saved():
    from cfdbench_amd.harness.args import Args
    assert Args().parse_args(["--model", "fno", "--data", "cavity_bc"]).unroll_detach == 0
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--unroll_steps", "3", "--unroll_detach", "1"])
    assert args.unroll_detach == 1 and args.as_dict()["unroll_detach"] == 1


def test_resume_refuses_another_unroll_detach():
    from cfdbench_amd.harness.dist_util import check_resume_state
    check_resume_state(dict(fused=True, world=1, unroll_steps=3, unroll_detach=1), fused=True, world=1, unroll_steps=3, unroll_detach=1)
    check_resume_state(dict(fused=True, world=1, unroll_steps=3), fused=True, world=1, unroll_steps=3, unroll_detach=0)  # no key: 0
    for state, now in ((dict(fused=True, world=1, unroll_steps=3), 1), (dict(fused=True, world=1, unroll_steps=3, unroll_detach=1), 0)):
        with pytest.raises(RuntimeError, match="unroll_detach"):
            check_resume_state(state, fused=True, world=1, unroll_steps=3, unroll_detach=now)


def _equal_batches(a, b):
    assert set(a) == set(b) == {"inputs", "label", "mask", "case_params", "labels_seq"}
    for k in ("inputs", "label", "mask", "case_params"):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert len(a["labels_seq"]) == len(b["labels_seq"])
    for x, y in zip(a["labels_seq"], b["labels_seq"]):
        assert x.is_contiguous() and torch.equal(x, y)
    assert torch.equal(a["labels_seq"][0], a["label"])


@pytest.mark.parametrize("indices", [None, [7, 2, 9, 0, 4]], ids=["all_windows", "indices"])
def test_device_batch_loader_windows_equal_collate_windows(indices):
    """Items are window numbers; every tensor of every batch is the one unroll.collate_windows builds -- a short last batch included."""
    from cfdbench_amd.harness.train_auto import collate_fn
    ds = SyntheticAutoDataset(n_cases=3, n_frames=7, height=8, width=8, seed=3, border_mask=True)
    K = 3
    starts, label_idx = unroll_windows(ds, K)
    assert len(starts) == 3 * 4
    loader = DeviceBatchLoader(ds, 4, shuffle=False, device="cpu", indices=indices, window_labels=label_idx)
    order = list(range(len(starts))) if indices is None else indices
    assert len(loader) == (len(order) + 3) // 4
    batches = list(loader)
    assert len(batches) == len(loader)
    for k, got in enumerate(batches):
        _equal_batches(got, collate_windows(ds, label_idx, order[4 * k:4 * k + 4], collate_fn, device=None))
    # shuffled: the same permutation draw as any loader of that many items, applied to window numbers
    torch.manual_seed(5)
    perm = torch.randperm(len(order)).tolist()
    torch.manual_seed(5)
    shuffled = DeviceBatchLoader(ds, 4, shuffle=True, device="cpu", indices=indices, window_labels=label_idx)
    for k, got in enumerate(shuffled):
        _equal_batches(got, collate_windows(ds, label_idx, [order[i] for i in perm[4 * k:4 * k + 4]], collate_fn, device=None))


def test_device_batch_loader_windows_refuse_bound_buffers():
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)
    _starts, label_idx = unroll_windows(ds, 2)
    loader = DeviceBatchLoader(ds, 2, device="cpu", window_labels=label_idx)
    bufs = {k: v.clone() for k, v in next(iter(DeviceBatchLoader(ds, 2, device="cpu", shuffle=False))).items()}
    with pytest.raises(ValueError, match="window"):
        loader.bind(bufs)
    with pytest.raises(ValueError, match="window_labels"):
        DeviceBatchLoader(ds, 2, device="cpu", window_labels=torch.zeros(4, dtype=torch.long))


class _Stub(torch.nn.Module):
    """A nonlinear one-step model with Fno2d's call signature and result dict."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.conv = torch.nn.Conv2d(2, 2, 3, padding=1).double()
        self.film = torch.nn.Linear(5, 2).double()

    def forward(self, inputs, case_params, mask=None, label=None):
        preds = torch.tanh(self.conv(inputs)) * (1.0 + self.film(case_params))[:, :, None, None] * mask
        lab = label * mask
        return dict(preds=preds, loss=dict(nmse=((preds - lab) ** 2).mean() / (lab ** 2).mean()))


def test_unrolled_loss_detach_is_the_sum_of_the_one_step_gradients():
    torch.manual_seed(1)
    K, model = 3, _Stub()
    x0, cp = torch.randn(2, 2, 6, 6, dtype=torch.float64), torch.randn(2, 5, dtype=torch.float64)
    mask = (torch.rand(2, 1, 6, 6) > 0.2).double()
    labels = [torch.randn(2, 2, 6, 6, dtype=torch.float64) for _ in range(K)]
    names = [n for n, _ in model.named_parameters()]

    def grads_of(loss):
        return dict(zip(names, torch.autograd.grad(loss, list(model.parameters()))))

    loss_d, preds_d = unrolled_loss(model, x0, labels, cp, mask, detach=True)
    got = grads_of(loss_d)
    want, x = {n: 0.0 for n in names}, x0
    for k in range(K):  # the one-step gradients along the model's own rollout, each with the window's 1 / K
        out = model(inputs=x, case_params=cp, mask=mask, label=labels[k])
        for n, g in grads_of(out["loss"]["nmse"] / K).items():
            want[n] = want[n] + g
        assert torch.equal(out["preds"].detach(), preds_d[k].detach())
        x = out["preds"].detach()
    for n in names:
        assert torch.allclose(got[n], want[n], rtol=1e-12, atol=1e-15), n
    loss_f, preds_f = unrolled_loss(model, x0, labels, cp, mask)
    full = grads_of(loss_f)
    assert torch.equal(loss_f.detach(), loss_d.detach()) and all(torch.equal(a.detach(), b.detach()) for a, b in zip(preds_f, preds_d))
    assert any((full[n] - got[n]).abs().max() > 1e-6 * full[n].abs().max() for n in names), "detach=False gives the truncated gradient"
    assert preds_d[0].requires_grad, "the returned predictions keep their graph; only the fed-back copy is cut"
