"""CPU: the window bookkeeping of training through a rollout (cfdbench_amd/unroll.py) and the option combinations train_auto refuses
with --unroll_steps > 1.  The device side is tests/test_gpu_fno_ingrad.py."""
import types

import pytest
import torch

from cfdbench_amd.harness.data import SyntheticAutoDataset
from cfdbench_amd.unroll import collate_windows, unroll_windows, unrolled_loss


@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_windows_never_cross_a_case(K):
    ds = SyntheticAutoDataset(n_cases=3, n_frames=6, height=8, width=8, seed=0)  # 5 items per case
    starts, idx = unroll_windows(ds, K)
    assert len(starts) == 3 * (5 - (K - 1)) and idx.shape == (len(starts), K)
    assert idx[:, 0].tolist() == starts
    for row in idx.tolist():
        assert len({ds.case_ids[i] for i in row}) == 1
        assert row == list(range(row[0], row[0] + K))
        for k in range(K - 1):  # the label of step k is the input frame of step k + 1
            assert torch.equal(ds.labels[row[k]], ds.inputs[row[k + 1]])
    # every window that fits is there
    fits = [i for i in range(len(ds)) if i + K - 1 < len(ds) and ds.case_ids[i + K - 1] == ds.case_ids[i]]
    assert starts == fits


def test_windows_follow_the_time_step_size():
    """Items two frames apart (delta_time = 2 data steps): step k's label is item i + 2 k; cases of 5, 4 and 1 items."""
    ds = types.SimpleNamespace(time_step_size=2, case_ids=[0] * 5 + [1] * 4 + [2])
    starts, idx = unroll_windows(ds, 3)
    assert starts == [0]
    assert idx.tolist() == [[0, 2, 4]]
    starts, idx = unroll_windows(ds, 2)
    assert starts == [0, 1, 2, 5, 6] and idx[:, 1].tolist() == [2, 3, 4, 7, 8]
    assert unroll_windows(ds, 4)[0] == [] and tuple(unroll_windows(ds, 4)[1].shape) == (0, 4)
    with pytest.raises(ValueError):
        unroll_windows(ds, 0)


def test_collate_windows_carries_the_label_frames():
    from cfdbench_amd.harness.train_auto import collate_fn
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=1)
    starts, idx = unroll_windows(ds, 3)
    batch = collate_windows(ds, idx, [0, 3], collate_fn, device=None)
    assert len(batch["labels_seq"]) == 3 and batch["labels_seq"][0] is batch["label"]
    for j, w in enumerate([0, 3]):
        assert torch.equal(batch["inputs"][j], ds.inputs[starts[w]][:-1])
        for k in range(3):
            assert torch.equal(batch["labels_seq"][k][j], ds.labels[starts[w] + k][:-1])


def test_unrolled_loss_needs_matching_channel_counts():
    with pytest.raises(ValueError, match="in_chan == out_chan"):
        unrolled_loss(None, torch.zeros(1, 2, 4, 4), [torch.zeros(1, 3, 4, 4)], torch.zeros(1, 5))
    with pytest.raises(ValueError):
        unrolled_loss(None, torch.zeros(1, 2, 4, 4), [], torch.zeros(1, 5))


@pytest.mark.parametrize("kw", [dict(fused=True), dict(graph=True), dict(device_loader=True), dict(gradient_accumulation_steps=2)])
def test_unroll_steps_refuses_what_it_does_not_run(tmp_path, kw):
    from cfdbench_amd.harness.train_auto import train
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)
    model = Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4)
    with pytest.raises(NotImplementedError, match="unroll_steps"):
        train(model, ds, ds, tmp_path / "run", num_epochs=1, unroll_steps=3, plot_interval=0, **kw)
    assert not (tmp_path / "run").exists()


def test_unroll_steps_refuses_other_models_and_short_cases(tmp_path):
    from cfdbench_amd.harness.train_auto import train
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    ds = SyntheticAutoDataset(n_cases=2, n_frames=3, height=8, width=8, seed=0)
    with pytest.raises(NotImplementedError, match="fno"):
        train(torch.nn.Linear(2, 2), ds, ds, tmp_path / "run", num_epochs=1, unroll_steps=2, plot_interval=0)
    with pytest.raises(ValueError, match="consecutive"):
        train(Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4), ds, ds, tmp_path / "run", num_epochs=1, unroll_steps=4, plot_interval=0)


def test_unroll_steps_flag():
    from cfdbench_amd.harness.args import Args, is_args_valid
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc"])
    assert args.unroll_steps == 1
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--unroll_steps", "3"])
    is_args_valid(args)
    assert args.unroll_steps == 3 and args.as_dict()["unroll_steps"] == 3
    with pytest.raises(AssertionError):
        is_args_valid(Args(model="fno", data_name="cavity_bc", unroll_steps=0))


def test_resume_refuses_another_unroll_steps():
    """An unrolled run writes into the directory of the one-step run with the same arguments: train_state.pt records unroll_steps, and a
    state written without it is a one-step run's."""
    from cfdbench_amd.harness.dist_util import check_resume_state
    check_resume_state(dict(fused=False, world=1), fused=False, world=1)
    check_resume_state(dict(fused=False, world=1, unroll_steps=3), fused=False, world=1, unroll_steps=3)
    for state, now in ((dict(fused=False, world=1), 3), (dict(fused=False, world=1, unroll_steps=3), 1),
                       (dict(fused=False, world=1, unroll_steps=2), 3)):
        with pytest.raises(RuntimeError, match="unroll_steps"):
            check_resume_state(state, fused=False, world=1, unroll_steps=now)
