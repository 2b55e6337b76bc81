"""Loader of the HIP extension (cfdbench_amd/_C/libcfdbench_amd.so).

There is NO fallback: if the library is missing or lacks a symbol the import of any compute entry point
raises, so a GPU run can never silently route around the hand-written kernels.
"""
from __future__ import annotations

import ctypes
import os
import threading
from pathlib import Path
from typing import Dict, NamedTuple, Tuple

from ._capi import CApi, CfdError, FnoShape

# CFDBENCH_AMD_LIB: explicit path of another build of the same library (kernel experiments: tools/build_variant.sh); there is
# still no fallback -- a path that does not exist fails exactly like a missing default build
_LIB_PATH = Path(os.environ.get("CFDBENCH_AMD_LIB") or Path(__file__).resolve().parent / "_C" / "libcfdbench_amd.so")
_lock = threading.Lock()
_api: CApi | None = None
_plans: Dict[Tuple[int, int, int, int, int], int] = {}


def lib_path() -> Path:
    return _LIB_PATH


def api() -> CApi:
    """The bound C ABI.  torch is imported first so that libamdhip64 resolves to the copy torch already
    loaded (one HIP runtime per process: streams and allocations are shared with PyTorch)."""
    global _api
    if _api is None:
        with _lock:
            if _api is None:
                import torch  # noqa: F401  (must precede the dlopen below)
                if not _LIB_PATH.exists():
                    raise CfdError(
                        f"HIP extension not built: {_LIB_PATH} is missing. Run `python -m cfdbench_amd.build` "
                        "(or __graft_entry__.build()). cfdbench_amd has no CPU/PyTorch fallback by design.")
                _api = CApi(ctypes.CDLL(str(_LIB_PATH), mode=ctypes.RTLD_GLOBAL), require_all=True)
                _check_single_hip_runtime()
    return _api


def _check_single_hip_runtime():
    try:
        with open("/proc/self/maps") as f:
            libs = {line.split()[-1] for line in f if "libamdhip64" in line}
    except OSError:
        return
    real = {os.path.realpath(p) for p in libs}
    if len(real) > 1:
        raise CfdError(f"two HIP runtimes are loaded in this process ({sorted(real)}); the extension must share "
                       "PyTorch's libamdhip64 -- import torch before cfdbench_amd and do not preload /opt/rocm's copy")


def plan(H: int, W: int, m1: int, m2: int, device_index: int) -> int:
    """Process-wide cache of operator tables keyed by (grid, modes, device).  Creating a plan allocates device
    memory, so it must not happen inside stream capture: call this once before capturing."""
    key = (H, W, m1, m2, device_index)
    p = _plans.get(key)
    if p is None:
        with _lock:
            p = _plans.get(key)
            if p is None:
                import torch
                with torch.cuda.device(device_index):
                    p = api().plan_create(H, W, m1, m2)
                _plans[key] = p
    return p


class FnoCall(NamedTuple):
    plan: int
    shape: FnoShape
    defers: bool  # the route honours CFD_TRAIN_DEFER_*


def fno_call(cfg: dict, B: int, in_chan: int, H: int, W: int, n_case_params: int, device, input_grads: bool = False) -> FnoCall:
    """What a whole-model C call needs besides its tensors, from ``Fno2d.abi_config()`` and one batch's extents: the plan and the
    ``FnoShape``.  The one place that knows the domain-padding rule: ``Fno2d(padding=)`` runs its FnoBlocks on (H + pad, W + pad), so
    that is the grid the plan is for, while the shape carries the data grid and ``pad``.

    ``defers`` mirrors ``route()`` of csrc/fno.cpp (the table above it): the wide route (hidden > 32), the many-modes route (modes1 > 15
    or modes2 > 16, or a plan wider than 80 columns: cfd_plan_create), the head's channel route (out_chan > 2) and a padded shape have
    none of the kernels that carry a deferred job and ignore the flags, so their gradients are final after the pass; the same holds for
    a pass whose ``grads`` struct asks for the gradients of the inputs or case parameters (``input_grads``; ABI 603).  Only
    ``FnoTrainEngine.gradients()`` reads ``defers``, and no caller sets ``input_grads`` yet: the engine never asks for input gradients
    and ``FnoForwardFn`` passes no flags.  The argument keeps this mirror of ``route()`` complete for the caller that will."""
    pad = int(cfg.get("padding", 0))
    m1, m2 = cfg["modes1"], cfg["modes2"]
    shape = FnoShape(B, H, W, in_chan, cfg["out_chan"], n_case_params, cfg["hidden"], cfg["num_layers"], m1, m2, cfg["head"], pad)
    defers = cfg["hidden"] <= 32 and m1 <= 15 and m2 <= 16 and W + pad <= 80 and cfg["out_chan"] <= 2 and pad == 0 and not input_grads
    return FnoCall(plan(H + pad, W + pad, m1, m2, device.index), shape, defers)
