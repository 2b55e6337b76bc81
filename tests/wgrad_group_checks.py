"""Backend-agnostic checks of the 1x1 weight / bias gradient at 17 .. 24 channels (k_chan_wgrad_grp, csrc/pointwise.hip: the second
16-row operand tiles loaded, activated and split once per group of 4 or 2 chunks) against the per-chunk kernel it replaces there
(`chan_wgrad_grp` = 0) and against the fp64 einsum of kernel_checks.check_chanmix; which kernel ran is read from the profiler hook's
labels; bf16 `in` is reached through one training step with bf16 activation storage.  Used by tests/test_emul_chan_wgrad_groups.py
(CPU, SIMT emulator) and tests/test_gpu_chan_wgrad_groups.py (MI355X).

`chan_wgrad_blocks` caps the workgroups of the launch, so that small shapes give one wave several chunks: with `blocks` workgroups a
wave walks chunks w, w + 4 blocks, .. of the B ceil(HW / 32) chunks."""
from __future__ import annotations

import ctypes

import numpy as np

from oracle import fno_oracle as O
from oracle import synth
from tests import ingrad_checks as IC
from tests import kernel_checks as K

f64 = np.float64


def chunks_per_wave(B, HW, blocks):
    """(fewest, most) chunks one wave of the capped launch walks."""
    total, stride = B * ((HW + 31) // 32), 4 * blocks
    return total // stride, -(-total // stride)


def _run(be, dg, dx, B, Ci, Co, HW, act):
    api, P = be.api, be.ptr
    ws = be.scratch(api.size("cfd_chan_wgrad_workspace_bytes", B, Ci, Co, HW))  # poisoned: every record that is read must be written
    gw, gb = be.out((Co, Ci)), be.out((Co,))
    api.call("cfd_chan_wgrad", P(dg), P(dx), P(gw), P(gb), P(ws), B, Ci, Co, HW, int(act), be.stream)
    be.sync()
    return be.host(gw), be.host(gb)


def check_wgrad_groups(be, B, Ci, Co, HW, act, blocks=-1, pieces=-1, const_g=None, seed=12):
    """cfd_chan_wgrad on the default route and with chan_wgrad_grp = 0, same inputs, fresh poisoned workspace and outputs each:
    gw / gb of the default route against fp64 (nMSE), gw / gb of the two routes against each other (bitwise), all values finite.
    const_g: the gradient is that constant everywhere, so gb[o] = const_g * B * HW exactly (a count of the ones column)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, Ci, HW)).astype(np.float32)
    g = rng.standard_normal((B, Co, HW)).astype(np.float32) if const_g is None else np.full((B, Co, HW), const_g, np.float32)
    f = O.gelu(x.astype(f64)) if act else x.astype(f64)
    ref_w = np.einsum("bop,bip->oi", g.astype(f64), f)
    ref_b = g.astype(f64).sum(axis=(0, 2))
    dg, dx = be.dev(g), be.dev(x)
    with K.tuned(be, chan_wgrad_blocks=blocks, act_pieces=pieces):
        new_w, new_b = _run(be, dg, dx, B, Ci, Co, HW, act)
        with K.tuned(be, chan_wgrad_grp=0):
            old_w, old_b = _run(be, dg, dx, B, Ci, Co, HW, act)
    return {"gw": K.nm(new_w, ref_w), "gb": K.nm(new_b, ref_b), "gw_old": K.nm(old_w, ref_w), "gb_old": K.nm(old_b, ref_b),
            "gw_bits": bool(np.array_equal(new_w.view(np.uint32), old_w.view(np.uint32))),
            "gb_bits": bool(np.array_equal(new_b.view(np.uint32), old_b.view(np.uint32))),
            "finite": bool(np.isfinite(new_w).all() and np.isfinite(new_b).all()),
            "gb_values": new_b, "gb_ref": ref_b}


def assert_case(res, tol=K.TOL):
    """The bound of the existing cfd_chan_wgrad checks (K.TOL; 1e-9 on the two-piece route) and bitwise-equal routes."""
    print({k: v for k, v in res.items() if not k.startswith("gb_v") and k != "gb_ref"})
    assert res["finite"], res
    for k in ("gw", "gb", "gw_old", "gb_old"):
        assert res[k] < tol, (k, res[k], tol)
    assert res["gw_bits"] and res["gb_bits"], res


def route_labels(be, B, Ci, Co, HW, grp=-1):
    """The profiler hook's kernel labels (cfd_prof_begin / cfd_prof_end) of one cfd_chan_wgrad call: which kernel the launcher chose."""
    rng = np.random.default_rng(3)
    dg, dx = be.dev(rng.standard_normal((B, Co, HW)).astype(np.float32)), be.dev(rng.standard_normal((B, Ci, HW)).astype(np.float32))
    buf = ctypes.create_string_buffer(1 << 12)
    with K.tuned(be, chan_wgrad_grp=grp):
        be.api.call("cfd_prof_begin")
        try:
            _run(be, dg, dx, B, Ci, Co, HW, 1)
        finally:
            be.api.call("cfd_prof_end", buf, len(buf))
    return {line.split()[0] for line in buf.value.decode().splitlines()}


# (Ci, Co, chan_wgrad_grp) -> the label of the main kernel
ROUTES = [(17, 17, -1, "k_chan_wgrad_grp"), (20, 20, -1, "k_chan_wgrad_grp"), (24, 24, -1, "k_chan_wgrad_grp"), (20, 17, -1, "k_chan_wgrad_grp"),
          (24, 17, -1, "k_chan_wgrad_grp"), (16, 16, -1, "k_chan_wgrad"), (25, 25, -1, "k_chan_wgrad"), (16, 20, -1, "k_chan_wgrad"),
          (20, 25, -1, "k_chan_wgrad"), (32, 32, -1, "k_chan_wgrad"), (8, 8, -1, "k_chan_wgrad"), (20, 20, 0, "k_chan_wgrad")]


def assert_route(be, Ci, Co, grp, label):
    assert route_labels(be, 2, Ci, Co, 96, grp) == {label, "k_wgrad_reduce"}


# ---- bf16 activation storage (the __bf16 instantiations; no C-ABI entry of their own: one training step) -------------------------------
# (B, H, W, blocks): 12 x 12 planes are 16-byte aligned in bf16 (the vector loads), 5 chunks per entry, the last one holds 16 pixels;
# 11 x 13 = 143 pixels are read element-wise.  25 chunks on one workgroup: its waves walk 7, 6, 6, 6 chunks (a full group + 3 / + 2);
# 20 chunks on one workgroup: 5 each (a full group + 1).  L = 2: block 0's gradient is the instantiation without activation,
# block 1's the one with it.
BF16_STEPS = [(5, 12, 12, 1), (4, 11, 13, 1)]
BF16_TOL = 1e-6  # tests/test_gpu_bf16_train.py: every gradient of a bf16-storage step against the fp64 oracle with the same storage rule


def check_bf16_step(be, B, H, W, blocks, C=20, L=2, m=4, p=5):
    """One training step with bf16 activation storage through the C ABI (cfd_fno_forward_train_f + every backward phase) at C = 20, the
    workgroups of the weight-gradient launches capped: every parameter gradient of the default route against the fp64 oracle with the
    same storage rule (rel nMSE) and, bitwise, against the step with chan_wgrad_grp = 0."""
    assert chunks_per_wave(B, H * W, blocks)[1] > 4
    params = synth.make_fno_params(401, C, L, m, m, p, spectral_gain=4.0)
    batch = synth.make_batch(411, B, H, W, p, border_mask=True)
    p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else f64) for k, v in params.items()}
    b64 = {k: v.astype(f64) for k, v in batch.items()}
    ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L, act_store=O.bf16_round)
    rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], "nmse"), L)
    buf = ctypes.create_string_buffer(1 << 14)
    with K.tuned(be, chan_wgrad_blocks=blocks):
        be.api.call("cfd_prof_begin")
        try:
            new = IC.run_ingrad(be, params, batch, L, C, H, W, p, m, m, want=(), route="phases", act_dtype=1)
        finally:
            be.api.call("cfd_prof_end", buf, len(buf))
        labels = {line.split()[0]: int(line.split()[1]) for line in buf.value.decode().splitlines()}
        assert labels.get("k_chan_wgrad_grp") == L and "k_chan_wgrad" not in labels, labels  # the blocks' weight gradients, new route
        with K.tuned(be, chan_wgrad_grp=0):
            old = IC.run_ingrad(be, params, batch, L, C, H, W, p, m, m, want=(), route="phases", act_dtype=1)
    same = all(np.array_equal(np.ascontiguousarray(v).view(np.uint32), np.ascontiguousarray(old["grads"][k]).view(np.uint32))
               for k, v in new["grads"].items())
    res = {"preds": K.nm(new["preds"], ref["preds"]), "bits": bool(same and np.array_equal(new["preds"], old["preds"])), "finite": all(np.isfinite(v).all() for v in new["grads"].values())}
    res.update({"g:" + k: K.nm(v, rg[k]) for k, v in new["grads"].items()})
    res.update({"old:" + k: K.nm(v, rg[k]) for k, v in old["grads"].items()})
    return res


def assert_bf16_step(res):
    print(res)
    assert res["bits"] and res["finite"], res
    for k, v in res.items():
        if k not in ("bits", "finite"):
            assert v < BF16_TOL, (k, v)


# ---- the cases (shared by both backends) --------------------------------------------------------------------------------------
# group tails at C = 20, HW = 4096 (128 chunks per entry): a wave walks exactly 4, 5, 6, 7 chunks -- a full group of 4, then a full
# group + 1, 2, 3 -- and, with 5 workgroups, 6 or 7 chunks depending on the wave
TAILS = [(1, 8, 4, 4), (5, 32, 5, 5), (3, 16, 6, 6), (7, 32, 7, 7), (1, 5, 6, 7)]  # (B, blocks, fewest, most chunks per wave)
# live lanes of the second tiles: C - 16 = 1, 3, 4 (G = 4) and 5, 8 (G = 2); C = 16 (its second input tile is the ones column alone),
# 25, 32 and 8 stay on the per-chunk kernel.  B = 2, HW = 1024, 2 workgroups: 8 chunks per wave = 2 groups of 4 / 4 groups of 2.
SQUARE = [17, 19, 20, 21, 24, 16, 25, 32, 8]
MIXED = [(20, 17), (17, 20), (24, 17), (18, 23), (21, 20)]  # (Ci, Co): G from the larger side
