"""Fused training engine for Auto-FNO: the reference's step
    model(**batch) -> loss["nmse"].backward() -> Adam.step() -> zero_grad()      (src/train_auto.py:231-257)
as three C-ABI calls on one flat parameter / gradient / moment buffer, plus (world_size > 1) one RCCL all-reduce of
the flat gradient between backward and Adam.  One process per GPU; nothing here syncs with the host.

The engine re-points the model's parameters at slices of the flat buffer, so ``model.state_dict()`` (reference
key names, complex64 spectral weights) always reflects the trained weights and checkpoints stay interchangeable.

Fine-tuning: parameters with ``requires_grad = False`` (or outside ``trainable=``) stay out of the flat buffers and keep their own storage;
the backward pass stops behind the phase of the shallowest trainable tensor (``last_backward_phase``).  ``optimizer="adamw"`` runs
decoupled weight decay inside the same optimiser launch (CFD_STEP_DECOUPLED_WD).

Unattended runs: ``skip_nonfinite=True`` skips an optimiser step whose gradient norm is not finite inside that same launch
(CFD_STEP_SKIP_NONFINITE): weights and moments keep their bits, the counts stay on the device.

Averaged weights: ``ema_decay=d`` keeps an exponential moving average of the trainable weights, updated inside that same launch
(cfd_fno_adam_step_ema): no launch more, a skipped step leaves it alone.  ``averaged()`` swaps it into the model for evaluation.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
from torch import Tensor

from . import _lib
from ._capi import (CFD_CLIP_CONSECUTIVE, CFD_CLIP_FLOATS, CFD_CLIP_SKIPPED, CFD_STEP_ACCUM_INIT, CFD_STEP_ACCUMULATE, CFD_STEP_DECOUPLED_WD,
                    CFD_STEP_SKIP_NONFINITE, CFD_HS_REC_FLOATS, CFD_OBJ_REC_FLOATS, OBJECTIVE_IDS)
from .functional import _param_struct
from .sobolev import HS_NAME, hs_arguments

_LOSS_IDS = {"mse": 0, "nmse": 1, "mae": 2}
_ACT_DTYPES = {"fp32": 0, "f32": 0, "float32": 0, "bf16": 1, "bfloat16": 1}


def _check_tensors(*tensors: Optional[Tensor]) -> None:
    if any(t is not None and (not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous()) for t in tensors):
        raise RuntimeError("FnoTrainEngine expects contiguous float32 CUDA tensors")


def flatten_layout(params: Sequence[Tensor], align: int = 4, trainable: Optional[Sequence[bool]] = None) -> Tuple[List[int], int]:
    """Offsets (in floats) of each tensor inside one flat fp32 buffer; complex tensors take 2 floats per element.  ``trainable`` (one flag
    per tensor; None = all): the COMPACT layout of a trainable subset -- same order, same alignment rule, a frozen tensor takes no room:
    its offset is that of the next trainable tensor (or the total), so ``backward_phase_slices`` holds on the compact buffer as it is."""
    offs, off = [], 0
    for i, p in enumerate(params):
        n = p.numel() * (2 if p.is_complex() else 1) if trainable is None or trainable[i] else 0
        offs.append(off)
        off += (n + align - 1) // align * align
    return offs, off


def param_phase(i: int, num_layers: int) -> int:
    """The backward phase that writes tensor i of ``abi_parameters`` (fc0 x2, four per FnoBlock, fc1 x2, fc2 x2): the head's four are
    phase 0, FnoBlock l's are phase L - l, fc0's are phase L + 1."""
    if not 0 <= i < 6 + 4 * num_layers:
        raise IndexError(f"tensor {i} of a model with {num_layers} FnoBlocks")
    if i < 2:
        return num_layers + 1
    if i >= 2 + 4 * num_layers:
        return 0
    return num_layers - (i - 2) // 4


def last_backward_phase(trainable: Sequence[bool], num_layers: int) -> int:
    """The last backward phase a pass must run for its trainable tensors (one flag per tensor, ``abi_parameters`` order): the phase of the
    SHALLOWEST trainable tensor -- head only: 0 (with the one-pass head no backward-phase call is made at all), FnoBlock l: L - l, fc0:
    L + 1.  A pass that must hand back the gradient of its inputs (``grads->d_inputs``) runs all L + 2 phases whatever this says."""
    if len(trainable) != 6 + 4 * num_layers:
        raise ValueError(f"{len(trainable)} flags for a model of {6 + 4 * num_layers} tensors")
    phases = [param_phase(i, num_layers) for i, t in enumerate(trainable) if t]
    if not phases:
        raise ValueError("nothing is trainable")
    return max(phases)


def mask_defer_flags(flags: int, fc0_trainable: bool, last_phase: int) -> int:
    """The CFD_TRAIN_DEFER_* bits a pass over a trainable subset may keep.  CFD_TRAIN_DEFER_STEM (4) goes when fc0 is frozen: the optimiser
    call would finish fc0's rows into the flat buffer, which holds no fc0.  CFD_TRAIN_DEFER_HEAD (2) goes when backward phase 1 does not
    run: that phase carries the head's reduction.  CFD_TRAIN_DEFER_SCALE (1) stays: the optimiser call applies the factor to whatever the
    flat gradient holds.  All trainable: the flags as they are."""
    if not fc0_trainable:
        flags &= ~4
    if last_phase < 1:
        flags &= ~2
    return flags


def match_prefixes(names: Sequence[str], prefixes: Sequence[str]) -> List[bool]:
    """One flag per name: whether a state_dict key prefix covers it (``blocks.1`` covers ``blocks.1.w0.weight``, not ``blocks.10...``; a
    full key covers itself).  A prefix that covers nothing is an error."""
    prefixes = [q.rstrip(".") for q in prefixes]
    covers = lambda q, k: k == q or k.startswith(q + ".")  # noqa: E731
    for q in prefixes:
        if not q or not any(covers(q, k) for k in names):
            raise ValueError(f"prefix {q!r} matches no parameter (keys: {', '.join(names)})")
    return [any(covers(q, k) for q in prefixes) for k in names]


class FlatParams:
    """One contiguous fp32 buffer holding every TRAINABLE parameter (``trainable``: one flag per tensor, None = all); the module's
    trainable Parameters become views of it.  A frozen parameter keeps its own (contiguous) storage -- ``views`` holds a float view of
    it, so ``ptrs()`` serves the ``params`` struct alike -- and its entry of ``grad_views`` lies in ``sink``, a scratch buffer the
    backward phases may write (they write every gradient tensor of their layer) and nothing reads."""

    def __init__(self, params: Sequence[torch.nn.Parameter], trainable: Optional[Sequence[bool]] = None):
        self.params = list(params)
        self.trainable = [True] * len(self.params) if trainable is None else [bool(t) for t in trainable]
        dev = self.params[0].device
        self.offsets, self.numel = flatten_layout(self.params, trainable=self.trainable)
        self.data = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        frozen = [not t for t in self.trainable]
        sink_offs, sink_numel = flatten_layout(self.params, trainable=frozen)
        self.sink = torch.empty(sink_numel, dtype=torch.float32, device=dev) if sink_numel else None
        self.views: List[Tensor] = []
        self.grad_views: List[Tensor] = []
        for p, off, soff, t in zip(self.params, self.offsets, sink_offs, self.trainable):
            n = p.numel() * (2 if p.is_complex() else 1)
            if not t:
                if p.dtype not in (torch.float32, torch.complex64):
                    raise TypeError("FlatParams: a frozen parameter must be float32 or complex64")
                p.data = p.detach().contiguous()
                self.views.append((torch.view_as_real(p.data) if p.is_complex() else p.data).reshape(-1))
                self.grad_views.append(self.sink[soff:soff + n])
                continue
            sl = self.data[off:off + n]
            gsl = self.grad[off:off + n]
            if p.is_complex():
                sl.view(*p.shape, 2).copy_(torch.view_as_real(p.detach().contiguous()))
                p.data = torch.view_as_complex(sl.view(*p.shape, 2))
            else:
                sl.view(p.shape).copy_(p.detach())
                p.data = sl.view(p.shape)
            self.views.append(sl)
            self.grad_views.append(gsl)

    def ptrs(self, grad: bool = False) -> List[int]:
        return [(g if grad else v).data_ptr() for v, g in zip(self.views, self.grad_views)]


# The process group the data-parallel exchanges use when none is given: the default group, or the one
# harness/dist_util.overlapping_comm_group picked (a communicator whose stream really overlaps the compute stream).
_dp_group = None


def set_default_group(group) -> None:
    global _dp_group
    _dp_group = group


def _resolve_group(group):
    if group is not None or _dp_group is None:
        return group
    try:  # (a group of a process group that has been destroyed since is forgotten)
        dist.get_world_size(_dp_group)
        return _dp_group
    except Exception:  # noqa: BLE001
        set_default_group(None)
        return None


class GradSync:
    """Data-parallel gradient exchange: SUM all-reduce of the flat gradient buffer (RCCL over xGMI on GPUs, gloo in
    the CPU tests) in ``n_buckets`` contiguous slices; the 1/world_size factor is folded into the Adam kernel.
    Semantics = DistributedDataParallel's (per-rank loss normalisers, averaged gradients)."""

    def __init__(self, group=None, n_buckets: int = 1):
        live = dist.is_available() and dist.is_initialized()
        group = _resolve_group(group) if live else group
        self.group = group
        self.world = dist.get_world_size(group) if live else 1
        self.n_buckets = max(1, n_buckets)
        # A one-rank group has nothing to exchange and skips the collectives -- unless CFDBENCH_DP_ALWAYS_EXCHANGE=1 asks for them:
        # that is how a one-GPU box runs the RCCL path itself (communicator stream, event ordering, slices of the flat buffer
        # reduced while later backward phases still write it; tests/test_gpu_dp.py).  A SUM over one rank is the identity.
        self.exchange = self.world > 1 or (live and os.environ.get("CFDBENCH_DP_ALWAYS_EXCHANGE", "0") == "1")
        # RCCL ("nccl") reduces device buffers on its own stream, ordered by events: the asynchronous per-slice exchange below.
        # Any other backend (gloo: the CPU tests, and the 2-process tests that share one GPU) gets device slices through an
        # explicit, stream-ordered host staging in wait_all -- correct by construction, no overlap.
        self.device_native = self.exchange and dist.get_backend(group) == "nccl"

    def bucket_slices(self, numel: int) -> List[Tuple[int, int]]:
        per = (numel + self.n_buckets - 1) // self.n_buckets
        per = (per + 3) // 4 * 4
        return [(s, min(numel, s + per)) for s in range(0, numel, per)]

    def reduce_slice_async(self, flat_grad: Tensor, start: int, stop: int):
        """Start the SUM all-reduce of flat_grad[start:stop] (ordered after the work already enqueued on the current
        stream, running on the communicator's own stream); None when there is nothing to exchange."""
        if not self.exchange or stop <= start:
            return None
        if flat_grad.is_cuda and not self.device_native:
            return ("host", flat_grad, start, stop)
        return dist.all_reduce(flat_grad[start:stop], op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def wait_all(self, handles) -> float:
        """Make the current stream wait for the started reductions; returns the 1/world scale for Adam."""
        for h in handles:
            if isinstance(h, tuple):  # host-staged slice: D2H (ordered after every kernel enqueued so far), reduce, H2D
                _, flat, a, b = h
                t = flat[a:b].cpu()
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
                flat[a:b].copy_(t)
            elif h is not None:
                h.wait()
        return 1.0 / self.world

    def all_reduce(self, flat_grad: Tensor) -> float:
        """Returns the scale to apply to the reduced gradient (1/world)."""
        if not self.exchange:
            return 1.0
        return self.wait_all([self.reduce_slice_async(flat_grad, a, b) for a, b in self.bucket_slices(flat_grad.numel())])


def backward_phase_slices(offsets: Sequence[int], numel: int, num_layers: int) -> List[Tuple[int, int]]:
    """[start, stop) of the flat gradient buffer written by backward phase k (``cfd_fno_backward_phase``): phase 0 = head
    (fc1, fc2: the last four tensors), phase 1 .. L = FnoBlock L-k (four tensors each), phase L+1 = fc0 (the first two).
    ``Fno2d.abi_parameters`` order is fc0, blocks 0 .. L-1, fc1, fc2, so every phase owns one contiguous slice and the
    slices tile the buffer."""
    end = lambda i: offsets[i + 1] if i + 1 < len(offsets) else numel
    sl = [(offsets[2 + 4 * num_layers], numel)]
    for k in range(1, num_layers + 1):
        l = num_layers - k
        sl.append((offsets[2 + 4 * l], end(2 + 4 * l + 3)))
    sl.append((0, end(1)))
    return sl


class FlatGradExchange:
    """Data-parallel gradient exchange of the AUTOGRAD training paths (U-Net, ResNet, the DeepONet family; eager or replayed from
    HIP graphs -- graph.GraphedTrainStep): after a backward pass every parameter gradient is packed, pre-scaled by 1 / world, into
    ONE flat fp32 buffer by one launch per 80 tensors (``cfd_scale_copy_multi``; complex gradients as (re, im) pairs), the buffer is
    SUM-all-reduced (RCCL over xGMI on GPUs; gloo in the CPU tests, staged through the host for device tensors like GradSync), and
    the parameters' ``.grad`` are re-pointed at views of the buffer, so the optimizer reads the reduced values where they are: no
    scatter-back.  DistributedDataParallel semantics (per-rank loss normalisers, averaged gradients).  (Rounds 1-4: ``torch.cat`` +
    all-reduce + ``mul_`` + one ``copy_`` launch per tensor, eager only.)"""

    def __init__(self, params: Sequence[torch.nn.Parameter], group=None):
        self.params = [p for p in params if p.requires_grad]
        if not self.params:
            raise ValueError("FlatGradExchange: no trainable parameters")
        self.sync = GradSync(group)
        self.world = self.sync.world
        dev = self.params[0].device
        self.offsets, self.numel = flatten_layout(self.params)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=dev)
        self.views: List[Tensor] = []  # what the optimizer reads: one view per parameter, the parameter's shape and dtype
        self._real_views: List[Tensor] = []
        for p_, off in zip(self.params, self.offsets):
            n = p_.numel() * (2 if p_.is_complex() else 1)
            sl = self.flat[off:off + n]
            self._real_views.append(sl)
            self.views.append(torch.view_as_complex(sl.view(*p_.shape, 2)) if p_.is_complex() else sl.view(p_.shape))
        self._table = None  # (key, ctypes tables) of the last pack

    def _sources(self) -> List[Tensor]:
        src = []
        for p_ in self.params:
            g = p_.grad
            if g is None:
                raise RuntimeError("FlatGradExchange.pack: a trainable parameter has no gradient (every parameter must take part in the "
                                   "loss: the flat buffer is exchanged whole)")
            g = torch.view_as_real(g) if g.is_complex() else g
            src.append(g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous())
        return src

    def pack(self) -> None:
        """``.grad`` of every parameter (wherever autograd left it) -> the flat buffer, times 1 / world."""
        src = self._sources()
        scale = 1.0 / self.world
        if self.flat.is_cuda:
            key = tuple(t.data_ptr() for t in src)
            if self._table is None or self._table[0] != key:
                col = lambda vals, ty: (ty * len(vals))(*vals)  # noqa: E731
                self._table = (key, (len(src), col(list(key), ctypes.c_void_p), col([v.data_ptr() for v in self._real_views], ctypes.c_void_p),
                                     col([t.numel() for t in src], ctypes.c_size_t)))
            n, sp, dp, nn = self._table[1]
            self._keep = src  # (temporaries of non-contiguous gradients live until the next pack)
            _lib.api().call("cfd_scale_copy_multi", n, sp, dp, nn, float(scale), torch.cuda.current_stream().cuda_stream)
        else:  # host tensors (the gloo tests of the exchange logic)
            with torch.no_grad():
                for d, t in zip(self._real_views, src):
                    d.copy_(t.reshape(-1)).mul_(scale)

    def reduce(self) -> None:
        """SUM all-reduce of the flat buffer (ordered after the work enqueued on the current stream)."""
        self.sync.wait_all([self.sync.reduce_slice_async(self.flat, a, b) for a, b in self.sync.bucket_slices(self.numel)])

    def install(self) -> None:
        """``p.grad`` = the parameter's view of the flat buffer (what ``optimizer.step()`` then reads)."""
        for p_, v in zip(self.params, self.views):
            p_.grad = v

    def exchange(self) -> None:
        self.pack()
        self.reduce()
        self.install()


def sync_gradients(params: Sequence[torch.nn.Parameter], group=None) -> None:
    """Data-parallel gradient averaging for the eager autograd training path (any model): FlatGradExchange on the parameters that
    received a gradient -- one pack launch per 80 tensors, ONE all-reduce, ``.grad`` left as views of the reduced flat buffer.
    Same semantics as DistributedDataParallel.  No-op outside a process group / in a one-rank group."""
    if not (dist.is_available() and dist.is_initialized()):
        return
    if dist.get_world_size(_resolve_group(group)) == 1 and os.environ.get("CFDBENCH_DP_ALWAYS_EXCHANGE", "0") != "1":
        return
    ps = [p_ for p_ in params if p_.requires_grad and p_.grad is not None]
    if not ps:
        return
    # One exchange object per (parameter set, group, world, backend), hung off the FIRST parameter so that it dies with the model
    # (a module-global dict kept every model's parameters and a model-sized flat buffer alive: ADVICE r5), and re-validated against
    # the live process group: after destroy_process_group + a new init in the same process a cached object would carry a stale
    # world size, backend and 1 / world scale.
    group = _resolve_group(group)
    world, backend = dist.get_world_size(group), dist.get_backend(group)
    key = tuple(id(p_) for p_ in ps) + (id(group), world, backend)
    slot = getattr(ps[0], "_cfd_grad_exchange", None)
    ex = slot[1] if slot is not None and slot[0] == key else None
    if ex is None or any(a is not b for a, b in zip(ex.params, ps)) or ex.sync.world != world:
        ex = FlatGradExchange(ps, group)
        ps[0]._cfd_grad_exchange = (key, ex)
    ex.exchange()


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [start, stop) of the items owned by ``rank`` (sizes differ by at most one)."""
    base, rem = divmod(n, world)
    start = rank * base + min(rank, rem)
    return start, start + base + (1 if rank < rem else 0)


class FnoTrainEngine:
    """The fused Auto-FNO training step on flat buffers (module docstring).

    What ``flat.grad`` holds after ``train_step``: the buffer the backward kernels wrote, NOT the gradient Adam applied.  With the
    deferred single-GPU step (``defer_flags``) it lacks the nMSE normaliser ``sums[3] / sums[2]`` (Adam's launch applies that factor)
    and its fc0 rows are written by the optimiser call itself; data-parallel, it is the SUM over ranks (Adam applies ``1 / world``);
    and it is never clipped.  Read gradients through ``gradients()`` (loss units, unclipped) and their norm through ``grad_norm()``;
    calling ``torch.nn.utils.clip_grad_norm_`` on the engine's views clips the wrong numbers -- pass ``max_grad_norm`` instead.

    Gradient accumulation: ``accumulate(..., weight=1 / N, first=k == 0)`` for each of a group's N micro-batches, then
    ``apply_accumulated()`` -- one optimiser step on ``sum_k weight_k * gradient_k``; ``train_step`` is the N = 1 case with its own,
    shorter launch sequence and never touches the accumulator."""

    def __init__(self, model, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, loss_name: str = "nmse", group=None, grad_buckets: int = 1,
                 overlap: bool = True, fused_head: bool = True, act_dtype: str = "fp32", max_grad_norm: Optional[float] = None,
                 trainable: Optional[Sequence[str]] = None, optimizer: str = "adam", skip_nonfinite: bool = False,
                 ema_decay: Optional[float] = None, ema_warmup: bool = False, objective: Optional[str] = None,
                 hs_k: Optional[int] = None, hs_a: Optional[Sequence[float]] = None, hs_group: Optional[bool] = None):
        """``trainable``: state_dict key prefixes (``{"fc1", "fc2"}``, ``{"blocks.3", "fc1", "fc2"}``) of the parameters to train; the
        others are frozen (their ``requires_grad`` is set to match).  None: the engine honours ``requires_grad`` as it finds it.  The
        flat buffers (parameters, gradient, moments, accumulator, what a data-parallel run exchanges) hold the trainable tensors only, and
        the backward pass stops behind the phase of the shallowest one (``last_backward_phase``); ``gradients()`` and ``grad_norm()`` are
        those of the trainable subset -- what ``clip_grad_norm_`` over the trainable parameters sees.  Nothing trainable: ValueError.

        ``optimizer``: "adam" (``weight_decay`` is L2, coupled: added to the gradient) or "adamw" (decoupled, torch.optim.AdamW's rule:
        CFD_STEP_DECOUPLED_WD of cfd_fno_adam_step, which is then the optimiser call on every route).

        ``max_grad_norm``: global gradient-norm clipping inside the optimiser call (cfd_fno_params.clip; the semantics of
        ``torch.nn.utils.clip_grad_norm_`` with norm_type 2, taken of the gradient Adam applies -- after the deferred normaliser, the
        lifting layer's rows and, data-parallel, the all-reduce and its 1 / world).  None: no clipping, the calls of an engine without
        the argument; ``float("inf")``: the norm is measured (``grad_norm()``) and nothing is clipped.  One launch more per step.

        ``skip_nonfinite``: an optimiser step whose gradient norm is not finite -- a NaN or inf anywhere in the gradient, an all-zero
        label under nMSE, a rollout window that blew up -- is SKIPPED on the device (CFD_STEP_SKIP_NONFINITE of cfd_fno_adam_step, which
        is then the optimiser call on every route): parameters and both moments keep their bits, no host sync.  The norm is the one
        clipping takes, so without ``max_grad_norm`` the engine measures it as ``float("inf")`` does (the same one launch more) and
        clips nothing.  ``skipped_steps()``, ``consecutive_skipped()`` and ``last_step_skipped()`` are device scalars.  The test sits
        where the gradient is final, so it holds on every route: ``train_step`` / ``optimizer_step`` / ``train_step_graph`` (the
        optimiser call is outside the replay), frozen subsets and AdamW (bits beside it), and ``apply_accumulated`` -- accumulation
        groups and rollout windows: a non-finite micro-batch makes the accumulator non-finite and the whole group is dropped.
        Data-parallel, both the overlapped and the single exchange decide on the REDUCED gradient: the all-reduce hands every rank the
        same bits (a NaN on one rank is a NaN in every rank's sum), each rank forms the same norm from them with the same 1 / world, so
        all ranks skip together and the replicas stay identical without a second collective.
        ``step_count`` advances on a skipped step too: the bias corrections after a skip are those of t, not of the number of applied
        steps (the one difference from a ``torch.amp.GradScaler`` skip; it keeps the guarded step without skips bitwise the unguarded
        one).

        ``ema_decay`` = d, 0 <= d < 1 (None: no average, the calls of an engine without the argument): ``self.ema``, a flat buffer laid out
        like ``flat.data`` -- compact, the trainable tensors only; a frozen tensor's average is the tensor itself -- starts as a copy of
        the initial weights and follows every applied optimiser step inside its launch (cfd_fno_adam_step_ema, which is then the optimiser
        call on every route, as with clipping and AdamW): ``ema = fmaf(d_t, ema, (1 - d_t) * new weight)``, timm's and diffusers'
        ``ema.mul_(d).add_(p, alpha=1 - d)``.  No launch more.  d_t (``ema_decay_at``) is d, or with ``ema_warmup`` min(d, (1 + t) / (10 + t))
        with t = ``step_count`` of the step (1 for the first; it runs on over a skipped step, like the bias corrections), formed on the
        host in double and rounded once, to the fp32 the call takes.  It holds on ``train_step`` / ``optimizer_step`` /
        ``train_step_graph`` (the call is outside the replay), ``apply_accumulated`` (groups and rollout windows: ``accumulate`` calls never
        touch the average), frozen subsets, AdamW and clipping; a step skipped by ``skip_nonfinite`` leaves the average's bits; data-
        parallel, every rank applies the same bits, so the replicas' averages stay identical with no collective.  ``ema_state_dict()``
        and ``averaged()`` read it; ``state_dict()`` carries it.

        ``objective`` = "rel_l2" | "nmse_sample" | "nmse_channel" (None: today's engine, call for call): what the step MINIMISES, beside
        what it reports (include/cfdbench_amd.h, "Training objectives": the per-sample relative L2 norm -- LpLoss().rel of the reference's
        FNO directory --, nMSE per sample, nMSE per channel).  A pass is then cfd_fno_forward (training; it still fills the loss sums, so
        ``scores()`` and the returned sums keep reporting mse / nmse), cfd_objective_fwd, cfd_objective_bwd into a per-shape gradient on
        the predictions, and the backward phases entered with that buffer as ``gpreds_ext`` (label = NULL, flags = 0); the gradient is
        final before the unchanged optimiser call, so clipping, ``skip_nonfinite``, EMA, AdamW, frozen subsets, accumulation groups and
        rollout windows (step k's 1 / K rides in ``upstream``, the chained input gradient of step k + 1 enters as ``gadd``) work as they
        do.  Nothing is deferred and the one-pass head is not used: ``loss_name`` must stay "nmse" and bf16 activation storage is
        refused (ValueError).  Data-parallel runs exchange once behind the pass, each rank's objective over its own batch.
        ``objective_value()`` is the device scalar of the last pass ((K,) for a window).
        ``objective`` = "hs": the relative Sobolev norm (include/cfdbench_amd.h, "Sobolev objective": HsLoss of the reference's FNO
        directory) with ``hs_k`` (1 or 2; default 1), ``hs_a`` (the k weights; default ones) and ``hs_group`` (the balanced form; default
        False).  The pass is the same call for call, with cfd_sobolev_fwd / cfd_sobolev_bwd on the predictions' data grid (H, W) -- also
        under domain padding -- in place of cfd_objective_fwd / _bwd.  The ``hs_*`` arguments with another objective: ValueError.

        ``act_dtype`` = "bf16": bf16-storage training (src/args.py:77-80 of the fork's other trainers): the saved
        activations a_0 .. a_L are rounded to bf16 when stored -- half the bytes of what the backward pass re-reads -- and the
        backward pass reads those rounded values; master weights, gradients, accumulation and Adam stay fp32
        (cfd_fno_forward_train_ex / cfd_fno_backward_phase_ex).  Needs the one-pass head (fused_head)."""
        if loss_name not in _LOSS_IDS:
            raise ValueError(f"loss_name must be one of {sorted(_LOSS_IDS)}")
        if act_dtype not in _ACT_DTYPES:
            raise ValueError(f"act_dtype must be one of {sorted(_ACT_DTYPES)}")
        self.act_dtype = _ACT_DTYPES[act_dtype]
        if self.act_dtype and not fused_head:
            raise ValueError("bf16 activation storage runs the one-pass training head: fused_head must be True")
        if objective is not None:
            if objective not in OBJECTIVE_IDS and objective != HS_NAME:
                raise ValueError(f"objective must be None or one of {sorted(OBJECTIVE_IDS) + [HS_NAME]}")
            if loss_name != "nmse":
                raise ValueError("an objective replaces the loss the step minimises; the reported loss stays nmse: loss_name must be 'nmse'")
            if self.act_dtype:
                raise ValueError("an objective runs the two-pass head: bf16 activation storage (the one-pass head) is not available")
        if objective != HS_NAME and not (hs_k is None and hs_a is None and hs_group is None):
            raise ValueError(f"hs_k, hs_a and hs_group are arguments of objective={HS_NAME!r}")
        self.objective = objective
        self.hs = hs_arguments(1 if hs_k is None else hs_k, hs_a, bool(hs_group)) if objective == HS_NAME else None
        if optimizer not in ("adam", "adamw"):
            raise ValueError("optimizer must be 'adam' or 'adamw'")
        self.optimizer = optimizer
        self._dw_flag = CFD_STEP_DECOUPLED_WD if optimizer == "adamw" else 0  # (beside the pass's flags in every optimiser call)
        self.api = _lib.api()
        self.model = model
        params = model.abi_parameters()
        if not params[0].is_cuda:
            raise RuntimeError("FnoTrainEngine: move the model to the GPU first (no CPU fallback)")
        self.device = params[0].device
        self.cfg = model.abi_config()
        self.L = self.cfg["num_layers"]
        key_of = {id(p_): k for k, p_ in model.named_parameters()}
        self.param_names = [key_of[id(p_)] for p_ in params]
        if trainable is not None:
            for p_, t in zip(params, match_prefixes(self.param_names, sorted(trainable))):
                p_.requires_grad_(t)
        mask = [bool(p_.requires_grad) for p_ in params]
        if not any(mask):
            raise ValueError("FnoTrainEngine: nothing is trainable (every parameter of the model is frozen)")
        self.all_trainable = all(mask)
        self.trainable_names = [k for k, t in zip(self.param_names, mask) if t]
        # the last backward phase of a pass (all trainable: L + 1, every phase)
        self.last_phase = last_backward_phase(mask, self.L)
        self.flat = FlatParams(params, None if self.all_trainable else mask)
        self.exp_avg = torch.zeros_like(self.flat.data)
        self.exp_avg_sq = torch.zeros_like(self.flat.data)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.loss_id = _LOSS_IDS[loss_name]
        self.step_count = 0
        self.sync = GradSync(group, grad_buckets)
        self.overlap = overlap  # DP: reduce each backward phase's gradients while the next phase computes
        # the projection head in ONE pass for both directions (cfd_fno_forward_train: the loss is fixed, so its gradient's
        # coefficient is known from the labels before the head runs); False = cfd_fno_forward + cfd_loss_coef + head backward
        self.fused_head = fused_head
        self.pstruct = _param_struct(self.flat.ptrs(False), self.L)
        self.gstruct = _param_struct(self.flat.ptrs(True), self.L)
        # Round 6: the single-GPU step folds its three tiny launches into launches that exist anyway (include/cfdbench_amd.h,
        # CFD_TRAIN_DEFER_*: the nMSE normaliser into Adam, the head's reduction into backward phase 1, the fc0 combine into Adam's
        # launch).  Data-parallel steps keep them: a rank's gradients must be final and normalised by ITS labels before the all-reduce.
        # With the flags, `flat.grad` after train_step holds the gradients of sum d^2 * upstream / n (nmse); `gradients()` rescales.
        # A trainable subset keeps the flags whose carrier still runs and whose result has a place (mask_defer_flags).  The normaliser's
        # flag is never dropped, so what reads `_route_defers` (optimizer_step, for gradients()) holds for a subset as it is.
        # (an objective's gradient enters the backward pass from outside: nothing is deferred)
        self.defer_flags = mask_defer_flags(0 if (self.sync.exchange or not fused_head or objective is not None) else 7, mask[0],
                                            self.last_phase)
        self._route_defers = False  # whether the batch's route honours the flags: known per batch (_prepare, _lib.fno_call)
        self.sums = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.coef = torch.zeros(2, dtype=torch.float32, device=self.device)
        self.scores_buf = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._shape_key = None
        self._graph = None
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.clip = None
        if self.max_grad_norm is not None and not self.max_grad_norm > 0.0:  # (NaN fails the comparison too)
            raise ValueError("max_grad_norm must be > 0 (None: no clipping, float('inf'): measure the norm only)")
        # the guard rides on the norm clipping takes: without a threshold of the caller's it measures (+inf) and clips nothing
        self.skip_nonfinite = bool(skip_nonfinite)
        self._skip_flag = CFD_STEP_SKIP_NONFINITE if self.skip_nonfinite else 0  # (beside the pass's flags in every optimiser call)
        self._clip_threshold = float("inf") if (self.skip_nonfinite and self.max_grad_norm is None) else self.max_grad_norm
        if self._clip_threshold is not None:
            # (zeroed: with the guard the last two floats are its counters, CFD_CLIP_SKIPPED / CFD_CLIP_CONSECUTIVE)
            self.clip = torch.zeros(CFD_CLIP_FLOATS, dtype=torch.float32, device=self.device)
            self.gstruct.clip, self.gstruct.max_grad_norm = self.clip.data_ptr(), self._clip_threshold
        # gradient accumulation over micro-batches (accumulate / apply_accumulated): the accumulator, laid out like flat.grad, and its
        # struct exist from the first accumulate() on -- an engine that never accumulates holds no more memory
        self.accum: Optional[Tensor] = None
        self.astruct = None
        self._accum_open = False   # between an accumulate() and its apply_accumulated()
        self._grad_in_accum = False  # whether the last optimiser step read the accumulator (gradients())
        # the averaged weights (cfd_fno_adam_step_ema): laid out like flat.data, a copy of the initial weights
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        if self.ema_decay is not None and not 0.0 <= self.ema_decay < 1.0:  # (NaN fails the comparison too)
            raise ValueError("ema_decay must be >= 0 and < 1 (None: no averaged weights)")
        self.ema_warmup = bool(ema_warmup)
        self.ema: Optional[Tensor] = None if self.ema_decay is None else self.flat.data.detach().clone()
        self._ema_scratch: Optional[Tensor] = None  # averaged(): where the trained weights wait
        self._averaged = False

    # ------------------------------------------------------------------------------------------------
    def _prepare(self, inputs: Tensor, case_params: Tensor):
        B, in_chan, H, W = inputs.shape
        key = (B, in_chan, H, W, case_params.shape[1])
        if key == self._shape_key:
            return
        c = self.cfg
        self.plan, self.shape, self._route_defers = _lib.fno_call(c, B, in_chan, H, W, case_params.shape[1], self.device)
        nbytes = self.api.size("cfd_fno_workspace_bytes_ex", self.plan, ctypes.byref(self.shape), 1, self.act_dtype)
        if nbytes == 0:
            raise RuntimeError("cfd_fno_workspace_bytes_ex returned 0 for this shape / activation type")
        self.ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        self.preds = torch.empty((B, c["out_chan"], H, W), dtype=torch.float32, device=self.device)
        if self.objective is not None:  # (per shape, like preds: a captured graph replays on these addresses)
            floats = CFD_HS_REC_FLOATS if self.hs is not None else CFD_OBJ_REC_FLOATS
            self._obj_rec = torch.empty(floats(B, c["out_chan"]), dtype=torch.float32, device=self.device)
            self._obj_gpreds = torch.empty_like(self.preds)
            self._obj_value = torch.zeros((), dtype=torch.float32, device=self.device)
            self._obj_last = self._obj_value
        self._shape_key = key
        self._graph = None

    def _objective_backward(self, plan, sh, pr, gr, data, sums, ws, st, value: Tensor, last_phase: int, gadd: Optional[int] = None,
                            upstream: float = 1.0) -> None:
        """Behind a training forward pass: the objective's value into ``value``, its gradient on the predictions times ``upstream`` (plus ``gadd``,
        the device address of a gradient to add, or None) into the per-shape buffer, and the backward phases 0 .. last_phase entered with it (label = NULL, no loss
        coefficients, flags = 0; the mse id: at flags = 0 the route rule does not read ``which``)."""
        a = self.api
        inputs, cp, mk, label, preds = data
        B, Co, HW = self.shape.B, self.shape.out_chan, self.shape.H * self.shape.W
        rec, gp = self._obj_rec.data_ptr(), self._obj_gpreds.data_ptr()
        if self.hs is not None:  # (the predictions' data grid: a padded model still returns (B, Co, H, W))
            H, W = self.shape.H, self.shape.W
            a.call("cfd_sobolev_fwd", preds, label, mk, rec, value.data_ptr(), B, Co, H, W, *self.hs, st)
            a.call("cfd_sobolev_bwd", preds, label, mk, rec, gadd, None, float(upstream), gp, B, Co, H, W, *self.hs, st)
        else:
            kind = OBJECTIVE_IDS[self.objective]
            a.call("cfd_objective_fwd", preds, label, mk, rec, value.data_ptr(), B, Co, HW, kind, st)
            a.call("cfd_objective_bwd", preds, label, mk, rec, gadd, None, float(upstream), gp, B, Co, HW, kind, st)
        for phase in range(last_phase + 1):
            a.call("cfd_fno_backward_phase_f", plan, sh, pr, gr, inputs, cp, mk, None, preds, gp, None, sums, ws, phase, _LOSS_IDS["mse"], 0,
                   0, st)

    def objective_value(self) -> Tensor:
        """Device tensor (no sync): the objective of the last pass -- 0-dim; after a rollout window (K,), one value per step."""
        if self.objective is None:
            raise RuntimeError("FnoTrainEngine.objective_value: the engine was built without objective")
        if getattr(self, "_obj_last", None) is None:
            raise RuntimeError("FnoTrainEngine.objective_value: no pass has run")
        return self._obj_last

    def forward_backward(self, inputs: Tensor, label: Tensor, case_params: Tensor, mask: Optional[Tensor] = None, flags: int = 0):
        """Enqueue forward + loss + backward into the flat gradient buffer (every gradient is overwritten).  ``flags`` =
        CFD_TRAIN_DEFER_* (train_step passes ``defer_flags``): the gradients are then complete only after ``optimizer_step``'s launch."""
        a = self.api
        model, data, sums, coef, ws, st = self._begin(inputs, label, case_params, mask, flags)
        if self.objective is not None:
            if flags:
                raise RuntimeError("FnoTrainEngine: a pass with an objective defers nothing (flags must be 0)")
            a.call("cfd_fno_forward", *model[:3], *data, sums, ws, 1, st)
            self._objective_backward(*model, data, sums, ws, st, self._obj_value, self.last_phase)
            self._obj_last = self._obj_value
            return
        if self.fused_head:
            a.call("cfd_fno_forward_train_f", *model, *data, sums, coef, ws, self.loss_id, 1.0, self.act_dtype, flags, st)
            # phase 0 (the head) left the fused kernel already; a trainable subset stops behind its shallowest tensor's phase
            for phase in range(1, self.last_phase + 1):
                a.call("cfd_fno_backward_phase_f", *model, *data, None, coef, sums, ws, phase, self.loss_id, self.act_dtype, flags, st)
            return
        if flags:
            raise RuntimeError("FnoTrainEngine: the deferred training step needs the one-pass head (fused_head)")
        self._forward_two_pass_head(model, data, sums, coef, ws, st)
        if self.all_trainable:
            a.call("cfd_fno_backward", *model, *data, None, coef, ws, st)
            return
        for phase in range(self.last_phase + 1):  # (cfd_fno_backward is every phase: a subset walks the phase entry itself)
            a.call("cfd_fno_backward_phase_ex", *model, *data, None, coef, ws, phase, self.act_dtype, st)

    def _begin(self, inputs: Tensor, label: Tensor, case_params: Tensor, mask: Optional[Tensor], flags: int):
        """What every pass starts with: the tensor check, the per-shape state, and the arguments its C calls share --
        (plan, shape, params, grads), (inputs, case_params, mask, label, preds), sums, coef, workspace, stream."""
        _check_tensors(inputs, label, case_params, mask)
        self._prepare(inputs, case_params)
        self._last = (inputs, case_params, mask, flags)  # optimizer_step finishes what the flags deferred
        model = (self.plan, ctypes.byref(self.shape), ctypes.byref(self.pstruct), ctypes.byref(self.gstruct))
        data = (inputs.data_ptr(), case_params.data_ptr(), None if mask is None else mask.data_ptr(), label.data_ptr(), self.preds.data_ptr())
        return (model, data, self.sums.data_ptr(), self.coef.data_ptr(), self.ws.data_ptr(), torch.cuda.current_stream().cuda_stream)

    def _forward_two_pass_head(self, model, data, sums, coef, ws, st):
        """fused_head = False: the plain forward (which keeps the activations), then the loss coefficients from its sums."""
        self.api.call("cfd_fno_forward", *model[:3], *data, sums, ws, 1, st)
        self.api.call("cfd_loss_coef", sums, coef, self.loss_id, 1.0, st)

    # ---- data-parallel step: backward phase by phase, each phase's gradient slice reduced while the next computes ----
    def phase_slices(self) -> List[Tuple[int, int]]:
        """[start, stop) of the flat gradient buffer written by backward phase k (cfd_fno_backward_phase): phase 0 = head
        (fc1, fc2: the last four tensors), phase 1 .. L = FnoBlock L-k (four tensors each), phase L+1 = fc0 (the first
        two).  ``abi_parameters`` order is fc0, blocks 0 .. L-1, fc1, fc2, so every phase owns one contiguous slice.  With a
        trainable subset the buffer is compact: a phase's slice covers its trainable tensors and is empty where it has none."""
        return backward_phase_slices(self.flat.offsets, self.flat.numel, self.L)

    def forward_backward_overlapped(self, inputs: Tensor, label: Tensor, case_params: Tensor,
                                    mask: Optional[Tensor] = None) -> float:
        """forward_backward with the gradient exchange overlapped: after each backward phase is enqueued, the SUM
        all-reduce of that phase's (final) gradient slice is started asynchronously -- RCCL runs it on its own stream
        while the following phases compute (the head's 12 KB first, then one 0.9-MB bucket per FnoBlock, during the next
        block's DFT / mix / fused block kernels).  Returns the 1/world scale for Adam.  Bitwise the same gradients as
        forward_backward + GradSync.all_reduce (same kernels, same reduction per element)."""
        a = self.api
        # (flags = 0: a data-parallel pass defers nothing, optimizer_step runs the plain flat Adam)
        model, data, sums, coef, ws, st = self._begin(inputs, label, case_params, mask, 0)
        if self.fused_head:
            a.call("cfd_fno_forward_train_ex", *model, *data, sums, coef, ws, self.loss_id, 1.0, self.act_dtype, st)
        else:
            self._forward_two_pass_head(model, data, sums, coef, ws, st)
        handles = []
        for phase, (s0, s1) in enumerate(self.phase_slices()):
            if not (self.fused_head and phase == 0):  # the fused forward has produced the head's gradients already
                a.call("cfd_fno_backward_phase_ex", *model, *data, None, coef, ws, phase, self.act_dtype, st)
            handles.append(self.sync.reduce_slice_async(self.flat.grad, s0, s1))
        return self.sync.wait_all(handles)

    def _adam_step(self, params, grads, dst: Tensor, grad: Tensor, stepping: bool, scale: float, flags: int, inputs: Tensor,
                   case_params: Tensor, mask: Optional[Tensor], sums: Optional[Tensor] = None, ws: Optional[Tensor] = None) -> None:
        """The cfd_fno_adam_step call of every route: ``params`` / ``grads`` structs, ``dst`` the flat buffer it writes (parameters or
        accumulator), ``grad`` the one it reads; ``stepping``: with moments, hyper-parameters, step count and the optimiser's own flags (an
        accumulate call takes none: NULL and zeros); then the pass's data tensors, and its loss sums and workspace where they are not the engine's own."""
        state = ((self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.flat.numel, self.lr, *self.betas, self.eps, self.weight_decay,
                  self.step_count) if stepping else (None, None, self.flat.numel, 0.0, 0.0, 0.0, 0.0, 0.0, 0))
        flags |= (self._dw_flag | self._skip_flag) if stepping else 0
        # with averaged weights the entry that carries them, on every route; an accumulate call writes no parameter and takes the plain one
        entry, tail = "cfd_fno_adam_step", ()
        if stepping and self.ema is not None:
            entry, tail = "cfd_fno_adam_step_ema", (self.ema.data_ptr(), self.ema_decay_at(self.step_count))
        self.api.call(entry, self.plan, ctypes.byref(self.shape), ctypes.byref(params), ctypes.byref(grads), inputs.data_ptr(),
                      case_params.data_ptr(), None if mask is None else mask.data_ptr(), (self.sums if sums is None else sums).data_ptr(),
                      (self.ws if ws is None else ws).data_ptr(), dst.data_ptr(), grad.data_ptr(), *state, scale, self.loss_id,
                      self.act_dtype, flags, torch.cuda.current_stream().cuda_stream, *tail)

    def _not_averaged(self, what: str) -> None:
        if self._averaged:
            raise RuntimeError(f"FnoTrainEngine.{what}: inside averaged() the model holds the averaged weights; training on them would "
                               "lose the trained ones -- leave the context first")

    def _no_open_group(self, what: str) -> None:
        self._not_averaged(what)
        if self._accum_open:
            raise RuntimeError(f"FnoTrainEngine.{what}: an accumulation group is open (accumulate() without its apply_accumulated()); "
                               "the step would run on the last micro-batch's gradient alone")

    # ---- gradient accumulation over micro-batches -----------------------------------------------------
    def accumulate(self, inputs: Tensor, label: Tensor, case_params: Tensor, mask: Optional[Tensor] = None, *, weight: float,
                   first: bool) -> Tensor:
        """One micro-batch of an accumulation group: forward + backward as in ``train_step`` (``defer_flags``; data-parallel: the
        non-overlapped pass, nothing is exchanged here), then ``accumulator (+)= weight * gradient`` in the launch that is Adam's in a plain
        step (cfd_fno_adam_step with CFD_STEP_ACCUMULATE: it finishes what the pass deferred, then adds instead of stepping).  ``first``
        starts a group -- the accumulator is overwritten, never read; ``weight`` is usually 1 / (micro-batches of the group).  Returns the
        device tensor of ``train_step`` for THIS micro-batch.  ``apply_accumulated()`` closes the group."""
        self._not_averaged("accumulate")
        if not first and not self._accum_open:
            raise RuntimeError("FnoTrainEngine.accumulate: first=False without an open group (the accumulator holds nothing to add to)")
        self.forward_backward(inputs, label, case_params, mask, self.defer_flags)
        self._ensure_accum()
        flags = self.defer_flags | CFD_STEP_ACCUMULATE | (CFD_STEP_ACCUM_INIT if first else 0)
        self._adam_step(self.astruct, self.gstruct, self.accum, self.flat.grad, False, float(weight), flags, inputs, case_params, mask)
        self._last = (inputs, case_params, mask, 0)  # (the deferred work of this pass is done)
        self._accum_open = True
        return self.sums

    def _ensure_accum(self) -> None:
        if self.accum is None:
            self.accum = torch.zeros_like(self.flat.grad)
            base, g0 = self.accum.data_ptr(), self.flat.grad.data_ptr()
            # (a frozen tensor's entry stays in the sink: the accumulate call touches the flat buffers and, under CFD_TRAIN_DEFER_STEM --
            # kept only with fc0 trainable -- fc0's rows)
            self.astruct = _param_struct([base + (p_ - g0) if t else p_ for p_, t in zip(self.flat.ptrs(True), self.flat.trainable)], self.L)
            if self.clip is not None:  # (read where the struct is the `grads` of the optimiser call on the accumulator)
                self.astruct.clip, self.astruct.max_grad_norm = self.clip.data_ptr(), self._clip_threshold

    # ---- training through a K-step rollout window ------------------------------------------------------
    def _window_state(self, inputs: Tensor, case_params: Tensor, K: int, full: bool) -> dict:
        """The buffers of a K-step window, per (shape key, K) as ``_prepare``'s are per shape: K prediction buffers and the (K, 4) sums;
        for the full gradient also K training workspaces, K coefficient pairs, the two buffers that carry the chained gradient, and one
        ``grads`` struct per step (they differ in ``d_inputs``)."""
        self._prepare(inputs, case_params)
        key = (self._shape_key, K)
        if getattr(self, "_win_key", None) != key:
            self._win = dict(preds=[torch.empty_like(self.preds) for _ in range(K)],
                             sums=torch.zeros((K, 4), dtype=torch.float32, device=self.device))
            if self.objective is not None:
                self._win["obj"] = torch.zeros(K, dtype=torch.float32, device=self.device)
            self._win_key = key
        w = self._win
        if full and "ws" not in w:
            w["ws"] = [torch.empty_like(self.ws) for _ in range(K)]
            w["coef"] = torch.zeros((K, 2), dtype=torch.float32, device=self.device)
            w["dx"] = [torch.empty_like(inputs) for _ in range(2)]
            ptrs = self.flat.ptrs(True)
            # step k (1-based) writes d loss / d x_k into dx[k % 2]; step 1 asks for none: the window's own inputs need no gradient
            w["gs"] = [_param_struct(ptrs, self.L, d_inputs=w["dx"][k % 2].data_ptr() if k >= 2 else None) for k in range(1, K + 1)]
        return w

    def preds_seq(self) -> List[Tensor]:
        """The K prediction buffers of the last window (K = 1: the one of the last pass); valid until the next window."""
        if getattr(self, "_win_last", None) is None:
            raise RuntimeError("FnoTrainEngine.preds_seq: no window has run")
        return list(self._win_last)

    def accumulate_window(self, inputs: Tensor, labels_seq: Sequence[Tensor], case_params: Tensor, mask: Optional[Tensor] = None, *,
                          weight: float, first: bool, detach: bool = False) -> Tensor:
        """One window of an accumulation group: ``accumulator (+)= weight * gradient of (1 / K) sum_k loss_k`` with ``x_1 = inputs`` and
        prediction k fed back as the input of step k + 1 (``unroll.unrolled_loss``).  Returns the (K, 4) device tensor whose row k is
        ``train_step``'s ``[sum sq err, sum abs err, sum sq label, n]`` of step k; ``preds_seq()`` the K predictions.  Group rules as
        ``accumulate``'s; ``apply_accumulated()`` closes the group, so clipping takes the norm of the whole window's (group's) gradient
        and a data-parallel run exchanges the accumulator once per optimiser step.

        ``detach=False``: the full gradient, through every fed-back frame.  K forward passes (flags = 0), each on a workspace of its own,
        then the backward passes K .. 1: step k's gradient of its inputs (``grads->d_inputs``) is step k - 1's external gradient on its
        predictions (``gpreds_ext``), and behind each pass the accumulate call adds ``weight`` times its parameter gradient.  The 1 / K
        rides in the loss coefficients (``upstream``).  fp32 activation storage only.
        ``detach=True`` (the pushforward trick): the fed-back frame is a constant, so the window is K plain micro-batches of weight
        ``weight / K`` -- ``accumulate`` itself, with deferred launches, one-pass head and bf16 storage as there."""
        self._not_averaged("accumulate_window")
        K = len(labels_seq)
        if K < 1:
            raise ValueError("FnoTrainEngine.accumulate_window: no label frames")
        if inputs.shape[1] != self.cfg["out_chan"] or labels_seq[0].shape[1] != inputs.shape[1]:
            raise ValueError(f"FnoTrainEngine.accumulate_window: the predictions are fed back as inputs, so in_chan == out_chan is required "
                             f"(inputs have {inputs.shape[1]} channels, the model predicts {self.cfg['out_chan']})")
        if K >= 2 and not detach and self.act_dtype:
            raise ValueError("FnoTrainEngine.accumulate_window: the full gradient through the fed-back frames needs fp32 activation storage "
                             "(the input gradient of a bf16-storage pass is not built); use detach=True or act_dtype='fp32'")
        if not first and not self._accum_open:
            raise RuntimeError("FnoTrainEngine.accumulate_window: first=False without an open group (the accumulator holds nothing to add to)")
        if K == 1:
            sums = self.accumulate(inputs, labels_seq[0], case_params, mask, weight=weight, first=first)
            self._win_last = [self.preds]
            return sums.view(1, 4)
        w = self._window_state(inputs, case_params, K, full=not detach)
        if detach:
            own = (self.preds, self.sums, getattr(self, "_obj_value", None))
            try:
                x = inputs
                for k in range(K):  # step k + 1 reads preds_k while it writes preds_{k+1}: every step has its own buffer (and sums row)
                    self.preds, self.sums = w["preds"][k], w["sums"][k]
                    if self.objective is not None:
                        self._obj_value = w["obj"][k]
                    self.accumulate(x, labels_seq[k], case_params, mask, weight=weight / K, first=first and k == 0)
                    x = w["preds"][k]
            finally:
                self.preds, self.sums, self._obj_value = own
            if self.objective is not None:
                self._obj_last = w["obj"]
            self._win_last = w["preds"]
            return w["sums"]
        a, st = self.api, torch.cuda.current_stream().cuda_stream
        _check_tensors(inputs, case_params, mask, *labels_seq)
        self._ensure_accum()
        plan, sh, pr = self.plan, ctypes.byref(self.shape), ctypes.byref(self.pstruct)
        cp, mk = case_params.data_ptr(), None if mask is None else mask.data_ptr()
        xs = [inputs] + w["preds"][:-1]
        one_pass = [False] * K

        def args(k):  # (grads struct, the five data pointers, sums, coef, workspace) of step k (0-based)
            return (ctypes.byref(w["gs"][k]), (xs[k].data_ptr(), cp, mk, labels_seq[k].data_ptr(), w["preds"][k].data_ptr()),
                    w["sums"][k].data_ptr(), w["coef"][k].data_ptr(), w["ws"][k].data_ptr())

        for k in range(K):
            gr, data, sums, coef, ws = args(k)
            if self.objective is not None:  # (the loss sums for the report; the objective itself runs in front of each backward pass)
                a.call("cfd_fno_forward", plan, sh, pr, *data, sums, ws, 1, st)
            elif k == K - 1 and self.fused_head:  # no chained gradient on the last step: the head runs once for both directions
                a.call("cfd_fno_forward_train_f", plan, sh, pr, gr, *data, sums, coef, ws, self.loss_id, 1.0 / K, 0, 0, st)
                one_pass[k] = True
            else:
                a.call("cfd_fno_forward", plan, sh, pr, *data, sums, ws, 1, st)
                a.call("cfd_loss_coef", sums, coef, self.loss_id, 1.0 / K, st)
        for k in range(K - 1, -1, -1):
            gr, data, sums, coef, ws = args(k)
            gext = w["dx"][k % 2].data_ptr() if k < K - 1 else None  # = d_inputs of step k + 1 (1-based k + 2: dx[(k + 2) % 2])
            # step k + 1 >= 2 hands d loss / d x back to the step before it: every phase; the window's first step stops where a plain pass does
            last = self.L + 1 if k >= 1 else self.last_phase
            if self.objective is not None:  # (the chained gradient is added where the objective's is written: gpreds_ext is their sum)
                self._objective_backward(plan, sh, pr, gr, data, sums, ws, st, w["obj"][k], last, gadd=gext, upstream=1.0 / K)
            else:
                for phase in range(1 if one_pass[k] else 0, last + 1):
                    a.call("cfd_fno_backward_phase_f", plan, sh, pr, gr, *data, gext, coef, sums, ws, phase, self.loss_id, 0, 0, st)
            flags = CFD_STEP_ACCUMULATE | (CFD_STEP_ACCUM_INIT if (first and k == K - 1) else 0)
            self._adam_step(self.astruct, w["gs"][k], self.accum, self.flat.grad, False, float(weight), flags, xs[k], case_params, mask,
                            w["sums"][k], w["ws"][k])  # (act_dtype is 0 here: bf16 storage was refused above)
        self._last = (inputs, case_params, mask, 0)
        self._accum_open = True
        self._win_last = w["preds"]
        if self.objective is not None:
            self._obj_last = w["obj"]
        return w["sums"]

    def train_window(self, inputs: Tensor, labels_seq: Sequence[Tensor], case_params: Tensor, mask: Optional[Tensor] = None,
                     detach: bool = False) -> Tensor:
        """One optimisation step on a K-step window: ``accumulate_window(weight=1.0, first=True)`` + ``apply_accumulated()``."""
        sums = self.accumulate_window(inputs, labels_seq, case_params, mask, weight=1.0, first=True, detach=detach)
        self.apply_accumulated()
        return sums

    def apply_accumulated(self) -> None:
        """The optimiser step of an accumulation group: data-parallel, ONE all-reduce of the accumulator (DistributedDataParallel's
        ``no_sync`` semantics: one exchange per optimiser step), then Adam -- with ``max_grad_norm`` the norm is taken of the accumulated
        gradient -- as the plain optimiser call with the accumulator as its gradient buffer.  Afterwards ``gradients()`` returns the
        accumulator (final, loss units, unclipped)."""
        if not self._accum_open:
            raise RuntimeError("FnoTrainEngine.apply_accumulated: nothing accumulated (call accumulate(..., first=True) first)")
        scale = self.sync.all_reduce(self.accum)
        self.step_count += 1
        self._adam_step(self.pstruct, self.astruct, self.flat.data, self.accum, True, scale, 0, *self._last[:3])
        self._accum_open = False
        self._grad_pending_scale = False
        self._grad_in_accum = True

    def optimizer_step(self, grad_scale: float = 1.0):
        self._no_open_group("optimizer_step")
        self._grad_in_accum = False
        self.step_count += 1
        inputs, case_params, mask, flags = getattr(self, "_last", (None, None, None, 0))
        # the pass left work to this launch (nMSE normaliser from sums[2:4], the lifting layer's gradient rows), or the step clips: the
        # norm is taken inside cfd_fno_adam_step, which with flags = 0 is cfd_adam_flat otherwise
        adamw = self._dw_flag != 0  # (decoupled decay exists in cfd_fno_adam_step alone: the optimiser call on every route)
        # (skip_nonfinite holds a clip buffer: the guard exists in cfd_fno_adam_step alone, like clipping)
        ema = self.ema is not None  # (the averaged weights exist in cfd_fno_adam_step_ema alone)
        if (self.clip is not None or adamw or ema) and inputs is None:
            raise RuntimeError("FnoTrainEngine.optimizer_step: gradient clipping, skip_nonfinite, AdamW and ema_decay need the pass that "
                               "produced the gradients (forward_backward / train_step) first")
        if flags or self.clip is not None or adamw or ema:
            self._adam_step(self.pstruct, self.gstruct, self.flat.data, self.flat.grad, True, grad_scale, flags, inputs, case_params, mask)
            self._last = (inputs, case_params, mask, 0)  # (a second optimizer_step on the same gradients must not redo the deferred work)
            self._grad_pending_scale = bool(flags & 1) and self.loss_id == _LOSS_IDS["nmse"] and self._route_defers
            return
        self._grad_pending_scale = False
        self.api.call("cfd_adam_flat", self.flat.data.data_ptr(), self.flat.grad.data_ptr(), self.exp_avg.data_ptr(),
                      self.exp_avg_sq.data_ptr(), self.flat.numel, self.lr, self.betas[0], self.betas[1], self.eps,
                      self.weight_decay, self.step_count, grad_scale, torch.cuda.current_stream().cuda_stream)

    def gradients(self) -> Tensor:
        """The flat gradient of the last step in the loss's own units, UNCLIPPED (with ``max_grad_norm`` Adam applied it times
        ``clip_coef()``; the buffer is never clipped).  After a deferred train_step (``defer_flags``) the buffer holds the gradients of
        sum d^2 / n -- this returns them times n / sum (label*mask)^2; otherwise the buffer itself (data-parallel: the sum over ranks).
        After ``apply_accumulated`` it is the accumulator: the weighted sum over the group's micro-batches, final.  With a trainable
        subset the buffer is compact: the trainable tensors in ``abi_parameters`` order (``flat.offsets``)."""
        if self._grad_in_accum:
            return self.accum
        if getattr(self, "_grad_pending_scale", False):
            return self.flat.grad * (self.sums[3] / self.sums[2])
        return self.flat.grad

    def grad_norm(self) -> Tensor:
        """0-dim device tensor (a view, no sync): the global 2-norm of the gradient the last optimiser call applied, before clipping."""
        if self.clip is None:
            raise RuntimeError("FnoTrainEngine.grad_norm: the engine was built without max_grad_norm (float('inf') measures without clipping)")
        return self.clip[0]

    def clip_coef(self) -> Tensor:
        """0-dim device tensor (a view, no sync): min(1, max_grad_norm / (norm + 1e-6)) of the last optimiser call."""
        if self.clip is None:
            raise RuntimeError("FnoTrainEngine.clip_coef: the engine was built without max_grad_norm")
        return self.clip[1]

    def _need_guard(self, what: str) -> None:
        if not self.skip_nonfinite:
            raise RuntimeError(f"FnoTrainEngine.{what}: the engine was built without skip_nonfinite")

    def skipped_steps(self) -> Tensor:
        """0-dim device tensor (a view, no sync): the optimiser steps skipped so far, a count held as a float (exact up to 2^24)."""
        self._need_guard("skipped_steps")
        return self.clip[CFD_CLIP_SKIPPED]

    def consecutive_skipped(self) -> Tensor:
        """0-dim device tensor (a view, no sync): the optimiser steps skipped since the last applied one."""
        self._need_guard("consecutive_skipped")
        return self.clip[CFD_CLIP_CONSECUTIVE]

    def last_step_skipped(self) -> Tensor:
        """0-dim device boolean (no sync): whether the last optimiser call applied nothing (``clip_coef() == 0``)."""
        self._need_guard("last_step_skipped")
        return self.clip[1] == 0

    # ---- averaged weights --------------------------------------------------------------------------------
    def _need_ema(self, what: str) -> None:
        if self.ema is None:
            raise RuntimeError(f"FnoTrainEngine.{what}: the engine was built without ema_decay")

    def ema_decay_at(self, t: int) -> float:
        """The decay of optimiser step t (``step_count`` of that step, 1 for the first) as a double: ``ema_decay``, with ``ema_warmup``
        min(ema_decay, (1 + t) / (10 + t)).  The call rounds it once, to fp32."""
        self._need_ema("ema_decay_at")
        return min(self.ema_decay, (1.0 + t) / (10.0 + t)) if self.ema_warmup else self.ema_decay

    def ema_state_dict(self) -> Dict[str, Tensor]:
        """The model's ``state_dict`` (reference key names, complex64 spectral weights) with the averaged weights: trainable tensors from
        the average, frozen ones (and buffers) from the model.  Copies: later steps do not change them."""
        self._need_ema("ema_state_dict")
        sd = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        for k, p_, off, t in zip(self.param_names, self.flat.params, self.flat.offsets, self.flat.trainable):
            if t:
                sl = self.ema[off:off + p_.numel() * (2 if p_.is_complex() else 1)]
                sd[k] = (torch.view_as_complex(sl.view(*p_.shape, 2)) if p_.is_complex() else sl.view(p_.shape)).clone()
        return sd

    @contextlib.contextmanager
    def averaged(self):
        """Context manager: inside it the model's storage holds the averaged weights (validation, a test run, a rollout), on exit the
        trained ones are back, bit for bit.  Two device copies each way through one scratch buffer; no pointer moves, so captured graphs
        and ``FnoRollout`` objects stay valid.  Frozen tensors are their own average.  Raises while an accumulation group is open; an
        training call inside the context raises too."""
        self._need_ema("averaged")
        self._no_open_group("averaged")  # (also: not inside averaged() already)
        if self._ema_scratch is None:
            self._ema_scratch = torch.empty_like(self.flat.data)
        self._ema_scratch.copy_(self.flat.data)
        self.flat.data.copy_(self.ema)
        self._averaged = True
        try:
            yield self.model
        finally:
            self.flat.data.copy_(self._ema_scratch)
            self._averaged = False

    def train_step(self, inputs: Tensor, label: Tensor, case_params: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        """One optimisation step; returns the device tensor [sum sq err, sum abs err, sum sq label, n] of THIS rank's
        batch (no host sync -- read it with .tolist() only when logging)."""
        self._no_open_group("train_step")
        # (a frozen subset exchanges its compact gradient once, behind the pass: the per-phase exchange is the all-trainable engine's)
        # (so does an objective: its pass has no per-phase entry of its own)
        if self.sync.exchange and self.overlap and self.all_trainable and self.objective is None:
            scale = self.forward_backward_overlapped(inputs, label, case_params, mask)
        else:
            self.forward_backward(inputs, label, case_params, mask, self.defer_flags)
            scale = self.sync.all_reduce(self.flat.grad)
        self.optimizer_step(scale)
        return self.sums

    # ---- optimiser state for full-state checkpoints (the reference saves weights only) ------------
    def state_dict(self) -> Dict[str, object]:
        """Adam moments (flat, in ``abi_parameters`` order), step count and learning rate.  The weights themselves live in
        the model's ``state_dict`` (the flat buffer is what the model's parameters view).  With ``skip_nonfinite`` also
        ``skipped_steps`` as an int (fetched here: saving synchronises anyway); an engine without the guard writes the state it always did.
        With ``ema_decay`` also ``ema`` (the flat average) and ``ema_decay``; an engine without it writes neither."""
        state = dict(exp_avg=self.exp_avg.detach().clone(), exp_avg_sq=self.exp_avg_sq.detach().clone(),
                     step_count=int(self.step_count), lr=float(self.lr), numel=int(self.flat.numel), trainable=list(self.trainable_names))
        if self.skip_nonfinite:
            state["skipped_steps"] = int(self.clip[CFD_CLIP_SKIPPED].item())
        if self.ema is not None:
            if self._averaged:
                raise RuntimeError("FnoTrainEngine.state_dict: inside averaged() the model holds the averaged weights")
            state["ema"], state["ema_decay"] = self.ema.detach().clone(), float(self.ema_decay)
        return state

    def load_state_dict(self, state: Dict[str, object]) -> None:
        # (a state from before the key existed is an all-trainable engine's)
        theirs = list(state.get("trainable", self.param_names))
        if theirs != self.trainable_names:
            raise ValueError(f"optimiser state is for the trainable tensors {theirs}, the engine trains {self.trainable_names}")
        if int(state["numel"]) != int(self.flat.numel):
            raise ValueError(f"optimiser state is for {state['numel']} parameters, the model has {self.flat.numel}")
        self.exp_avg.copy_(state["exp_avg"].to(self.device))
        self.exp_avg_sq.copy_(state["exp_avg_sq"].to(self.device))
        self.step_count = int(state["step_count"])
        self.lr = float(state["lr"])
        if self.skip_nonfinite:  # (a state without the key -- an unguarded run's -- means 0; the run of consecutive skips starts anew)
            self.clip[CFD_CLIP_SKIPPED] = float(state.get("skipped_steps", 0))
            self.clip[CFD_CLIP_CONSECUTIVE] = 0.0
        if self.ema is not None:
            # a state without the key -- a run without the average -- restarts it from the weights the model holds now: load the model's
            # weights first.  The decay stays this engine's (a resumed run may change it).
            self.ema.copy_(state["ema"].to(self.device) if state.get("ema") is not None else self.flat.data)

    def scores(self) -> Dict[str, float]:
        """{mse, rmse, mae, nmse} of the last step (loss.py:27-35).  Synchronises."""
        self.api.call("cfd_loss_scores", self.sums.data_ptr(), self.scores_buf.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        v = self.scores_buf.tolist()
        return dict(mse=v[0], rmse=v[1], mae=v[2], nmse=v[3])

    # ---- optional HIP-graph replay of forward+backward (static buffers) -------------------------------
    def capture(self, inputs: Tensor, label: Tensor, case_params: Tensor, mask: Optional[Tensor] = None):
        """Capture forward+loss+backward for this batch shape into a HIP graph.  Afterwards ``train_step_graph``
        copies a batch into the static buffers and replays; the all-reduce and Adam stay outside the graph."""
        self._static = [t.clone() if t is not None else None for t in (inputs, label, case_params, mask)]
        self._prepare(inputs, case_params)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self.forward_backward(*self._static, flags=self.defer_flags)  # warm-up outside capture
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        from .graph import CAPTURE_MODE
        torch.cuda.synchronize()  # (no collective of an earlier step in flight: see graph.CAPTURE_MODE)
        # Round 6: over RCCL the per-phase all-reduces are captured with the pass (forked onto the communicator's stream and joined back
        # by events), so a replayed data-parallel step makes no host call into the process group; host-staged backends reduce after it.
        self._graph_exchanges = bool(self.sync.exchange and self.sync.device_native and self.overlap and self.all_trainable
                                     and self.objective is None
                                     and os.environ.get("CFDBENCH_DP_ONE_GRAPH", "1") != "0")
        with torch.cuda.graph(g, capture_error_mode=CAPTURE_MODE):
            if self._graph_exchanges:
                self._graph_scale = self.forward_backward_overlapped(*self._static)
            else:
                self.forward_backward(*self._static, flags=self.defer_flags)
        self._graph = g

    def train_step_graph(self, inputs: Tensor, label: Tensor, case_params: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        self._no_open_group("train_step_graph")
        key = (*inputs.shape, case_params.shape[1], mask is not None)
        if self._graph is None or key != getattr(self, "_graph_key", None):  # a new batch shape needs a new capture
            self.capture(inputs, label, case_params, mask)
            self._graph_key = key
        for dst, src in zip(self._static, (inputs, label, case_params, mask)):
            if dst is not None and src is not dst:
                dst.copy_(src, non_blocking=True)
        self._graph.replay()
        self._last = (self._static[0], self._static[2], self._static[3], self.defer_flags)  # (the replayed pass used the static buffers)
        scale = self._graph_scale if self._graph_exchanges else self.sync.all_reduce(self.flat.grad)
        self.optimizer_step(scale)
        return self.sums
