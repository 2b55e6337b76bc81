"""CPU: the gradient-clipping rule of tests/clip_checks.py against torch.nn.utils.clip_grad_norm_, the --max_grad_norm flag and what the
trainers refuse with it, and ABI 604's two struct fields.  The kernels: tests/test_emul_fno_clip.py, tests/test_gpu_fno_clip.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import clip_checks as CC

REPO = Path(__file__).resolve().parent.parent


def _tensors(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(7, 5, generator=g, dtype=torch.float64), torch.randn(3, generator=g, dtype=torch.float64),
            torch.complex(torch.randn(2, 3, 4, generator=g, dtype=torch.float64), torch.randn(2, 3, 4, generator=g, dtype=torch.float64))]


@pytest.mark.parametrize("complex_too", [False, True])
@pytest.mark.parametrize("factor", [0.25, 4.0])  # threshold below and above the norm
def test_rule_matches_torch(complex_too, factor):
    grads = _tensors(3)[:3 if complex_too else 2]
    params = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads]
    for p_, g in zip(params, grads):
        p_.grad = g.clone()
    norm0 = float(torch.sqrt(sum((g.abs() ** 2).sum() for g in grads)))
    max_norm = factor * norm0
    norm_t = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    norm, coef, clipped = CC.clip_rule([g.numpy() for g in grads], max_norm)
    assert abs(norm - norm_t) <= 1e-6 * norm_t and abs(norm - norm0) <= 1e-12 * norm0
    assert (coef == 1.0) == (factor > 1.0)
    for p_, c in zip(params, clipped):
        assert np.max(np.abs(p_.grad.numpy() - c)) <= 1e-6 * np.max(np.abs(c))


def test_rule_scale_is_inside_the_norm():
    g = [np.arange(1.0, 9.0)]
    n1, c1, e1 = CC.clip_rule(g, 1.0, scale=0.5)
    n2, c2, e2 = CC.clip_rule([0.5 * g[0]], 1.0)
    assert n1 == n2 and c1 == c2 and np.allclose(e1[0], e2[0], rtol=1e-15)
    assert CC.clip_rule(g, float("inf"))[1] == 1.0


def test_flag_and_validation():
    from cfdbench_amd.harness.args import Args, is_args_valid
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc"])
    assert args.max_grad_norm == 0.0 and isinstance(args.max_grad_norm, float)
    is_args_valid(args)
    args = Args().parse_args(["--model", "fno", "--data", "cavity_bc", "--fused", "1", "--max_grad_norm", "1.0"])
    is_args_valid(args)
    assert args.max_grad_norm == 1.0 and args.as_dict()["max_grad_norm"] == 1.0
    is_args_valid(Args(model="unet", data_name="cavity_bc", max_grad_norm=0.5))
    with pytest.raises(AssertionError):
        is_args_valid(Args(model="fno", data_name="cavity_bc", max_grad_norm=-1.0))
    with pytest.raises(AssertionError):
        is_args_valid(Args(model="fno", data_name="cavity_bc", graph=1, max_grad_norm=1.0))
    is_args_valid(Args(model="fno", data_name="cavity_bc", graph=1))


@pytest.mark.parametrize("auto", [True, False])
def test_graph_with_clipping_is_refused_before_the_directory_is_made(tmp_path, auto):
    from cfdbench_amd.harness.data import SyntheticAutoDataset
    from cfdbench_amd.models.fno.fno2d import Fno2d
    from cfdbench_amd.models.loss import loss_name_to_fn
    if auto:
        from cfdbench_amd.harness.train_auto import train
    else:
        from cfdbench_amd.harness.train import train
    ds = SyntheticAutoDataset(n_cases=2, n_frames=5, height=8, width=8, seed=0)
    model = Fno2d(2, 2, 5, loss_name_to_fn("nmse"), 1, 2, 2, 4)
    with pytest.raises(NotImplementedError, match="max_grad_norm"):
        train(model, ds, ds, tmp_path / "run", num_epochs=1, graph=True, max_grad_norm=1.0, plot_interval=0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        train(model, ds, ds, tmp_path / "run", num_epochs=1, max_grad_norm=-1.0, plot_interval=0)
    assert not (tmp_path / "run").exists()


def test_abi_version_and_struct_fields(tmp_path):
    """ABI 604 in the binding and the header; cfd_fno_params ends with clip, max_grad_norm at the offsets the C compiler gives them."""
    from cfdbench_amd._capi import ABI_VERSION, CFD_CLIP_FLOATS, FnoParams
    from tests.emul.build_emul import CLANG
    header = (REPO / "include" / "cfdbench_amd.h").read_text()
    assert ABI_VERSION == 604 == int(re.search(r"#define CFD_ABI_VERSION (\d+)", header).group(1))
    assert CFD_CLIP_FLOATS == int(re.search(r"#define CFD_CLIP_FLOATS (\d+)", header).group(1))
    assert [f[0] for f in FnoParams._fields_][-2:] == ["clip", "max_grad_norm"]
    src = tmp_path / "offsets.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "cfdbench_amd.h"\nint main() { printf("%zu %zu %zu %zu\\n", '
                   'offsetof(cfd_fno_params, d_case_params), offsetof(cfd_fno_params, clip), offsetof(cfd_fno_params, max_grad_norm), '
                   'sizeof(cfd_fno_params)); }\n')
    exe = tmp_path / "offsets"
    subprocess.run([CLANG, "-x", "c++", f"-I{REPO / 'include'}", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [FnoParams.d_case_params.offset, FnoParams.clip.offset, FnoParams.max_grad_norm.offset, ctypes.sizeof(FnoParams)]
    assert FnoParams.clip.offset == FnoParams.d_case_params.offset + 8 and FnoParams.max_grad_norm.offset == FnoParams.clip.offset + 8
