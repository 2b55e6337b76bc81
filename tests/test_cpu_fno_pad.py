"""CPU: host side of the FNO's domain padding -- the shape struct's new field, the harness flag and the run directory (no kernel runs)."""
import pytest

from cfdbench_amd._capi import FnoShape
from cfdbench_amd.harness.args import Args, is_args_valid
from cfdbench_amd.harness.autoregressive import init_model
from cfdbench_amd.harness.common import get_output_dir


def test_fno_shape_pad_field_defaults_to_zero():
    """An 11-field FnoShape, as every caller before ABI 602 builds it, means pad = 0."""
    assert FnoShape(1, 8, 8, 2, 2, 5, 20, 2, 4, 4, 128).pad == 0
    assert FnoShape(1, 8, 8, 2, 2, 5, 20, 2, 4, 4, 128, 3).pad == 3
    assert [n for n, _ in FnoShape._fields_][-1] == "pad"


def test_fno_padding_flag_and_output_dir():
    base = ["--model", "fno", "--data", "cavity_bc", "--fno_hidden_dim", "20"]
    plain, padded = Args().parse_args(base), Args().parse_args(base + ["--fno_padding", "8"])
    assert plain.fno_padding is None and padded.fno_padding == 8
    is_args_valid(plain)
    is_args_valid(padded)
    d0, d1 = get_output_dir(plain, is_auto=True), get_output_dir(padded, is_auto=True)
    assert "pad" not in d0.name and d1.name == d0.name + "_pad8" and d1.parent == d0.parent
    assert init_model(plain).padding is None and init_model(padded).padding == 8
    for bad in (dict(fno_padding=0), dict(fno_padding=4, dtype="bf16"), dict(model="unet", fno_padding=4)):
        with pytest.raises(AssertionError):
            is_args_valid(Args(**{**dict(model="fno", data_name="cavity_bc"), **bad}))
