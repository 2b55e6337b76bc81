"""Checks of the fused FNO engine's K-step rollout window (FnoTrainEngine.accumulate_window): the engine's exact call sequence over the C
ABI on tests/backends.py's hostile memory.  Used by tests/test_emul_fno_window.py (CPU, SIMT emulator) and tests/test_gpu_fno_window.py
(MI355X).  No new entry point: the forward calls, the head backward with `gpreds_ext`, grads->d_inputs (ABI 603) and cfd_fno_adam_step with
CFD_STEP_ACCUMULATE (ABI 604).

The sequence (full gradient, K >= 2, every pass with flags = 0; k is 1-based):
    forward k = 1 .. K     x_1 = inputs, x_{k+1} = preds_k; workspace, preds, sums and coef of its own per step.  k < K:
                           cfd_fno_forward(training = 1) + cfd_loss_coef(upstream = 1 / K); k = K: the same, or the one-pass head
                           cfd_fno_forward_train_f(upstream = 1 / K)
    backward k = K .. 1    grads->d_inputs = dx[k % 2] (k >= 2; NULL for k = 1), gpreds_ext = dx[(k + 1) % 2] (k < K; NULL for k = K),
                           phases 0 .. L + 1 (phase 0 skipped where the one-pass head ran), then cfd_fno_adam_step with
                           CFD_STEP_ACCUMULATE (| CFD_STEP_ACCUM_INIT iff first and k == K), grad_scale = weight, ws_k, x_k
Truncated gradient (detach): K plain micro-batches, step k with grad_scale = weight / K and CFD_STEP_ACCUM_INIT iff first and k == 1.

Shapes, fixtures and fp64 references are tests/ingrad_checks.py's: small_case, unroll_labels, ref_unroll, ref_run, golden_case."""
from __future__ import annotations

import ctypes

import numpy as np

from cfdbench_amd._capi import CFD_STEP_ACCUM_INIT, CFD_STEP_ACCUMULATE
from tests import fno_checks as F
from tests import ingrad_checks as IC

nm = IC.nm
ACC, INIT = CFD_STEP_ACCUMULATE, CFD_STEP_ACCUM_INIT
NMSE = F.WHICH["nmse"]
ABI_TOL = 1e-9    # C ABI against fp64 (tests/test_gpu_fno_ingrad.py, tests/test_emul_fno_ingrad.py)
MODEL_TOL = 1e-8  # against the reference's fp32 fixtures (what test_unrolled_loss_vs_reference_golden holds the eager window to)

# (B, C, L, H, W, m1, m2, p, cin, pad), K: ingrad's shapes -- the scalar forms on an odd grid, domain padding, the wide route (hidden > 32),
# the head's channel route (out_chan = 3), a model without FnoBlocks, and the benchmark's width at a batch that cuts several records
CASES = {
    "9x7_scalar_form": ((3, 6, 2, 9, 7, 4, 4, 5, 2, 0), 3),
    "12x12_pad4": ((2, 6, 2, 12, 12, 4, 4, 5, 2, 4), 2),
    "c33": ((1, 33, 1, 8, 8, 2, 3, 5, 2, 0), 2),
    "p8_cin3": ((2, 7, 1, 8, 8, 2, 3, 8, 3, 0), 2),
    "no_layers": ((2, 6, 0, 8, 8, 2, 3, 5, 2, 0), 2),
    "64x64_w20_b5": ((5, 20, 2, 64, 64, 12, 12, 5, 2, 0), 2),
}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def case(name, bseed=42):
    """(params, batch, K label frames, shape record, K) of a case; `bseed` picks another batch (and labels) on the same weights."""
    (B, C, L, H, W, m1, m2, p, cin, pad), K_ = CASES[name]
    params, batch = IC.small_case(B, C, L, H, W, m1, m2, p, cin, pad, bseed=bseed)
    labels = IC.cached(("window_labels", name, bseed), lambda: IC.unroll_labels(5 + bseed, batch, K_))
    return params, batch, labels, dict(L=L, C=C, H=H, W=W, p=p, m1=m1, m2=m2, pad=pad, cin=cin), K_


def ref_full(name, bseed=42):
    """fp64: the gradient of (1 / K) sum_k nmse_k through every fed-back frame."""
    params, batch, labels, s, _ = case(name, bseed)
    return IC.cached(("window_ref", name, bseed), lambda: IC.ref_unroll(params, batch, labels, s["L"], s["pad"]))


def ref_detached(name, bseed=42):
    """fp64: (1 / K) sum_k of the one-step gradients taken at x_k, the fp64 predictions fed back as constants."""
    params, batch, labels, s, K_ = case(name, bseed)

    def make():
        x, preds, grads = batch["inputs"], [], None
        for k in range(K_):
            r = IC.ref_run(params, dict(batch, inputs=x, label=labels[k]), s["L"], s["pad"])
            x = r["preds"]
            preds.append(x)
            grads = {q: v / K_ for q, v in r["grads"].items()} if grads is None else {q: grads[q] + r["grads"][q] / K_ for q in grads}
        return dict(preds=preds, grads=grads)
    return IC.cached(("window_ref_detached", name, bseed), make)


class Rig:
    """The buffers of an engine that runs K-step windows of one shape: plan, flat parameters, the hostile flat gradient buffer, the
    NaN-poisoned accumulator, K workspaces / prediction buffers / sums / coef pairs, the two chained-gradient buffers, and one `grads`
    struct per step."""

    def __init__(self, be, params, batch, s, K_):
        self.be, self.api, self.K, self.s = be, be.api, K_, s
        self.L = L = s["L"]
        self.layout, self.numel, self.flat0 = F.flat_layout(params, L)
        self.params = params
        self.plan = self.api.plan_create(s["H"] + s["pad"], s["W"] + s["pad"], s["m1"], s["m2"])
        self.shape = F.fno_shape(batch, L, s["C"], s["H"], s["W"], s["p"], s["m1"], s["m2"], s["pad"])
        self.sh = ctypes.byref(self.shape)
        self.flat = be.dev(self.flat0)
        self.grad = F.flat_grad_buffer(be, self.layout, self.numel)
        self.acc = be.out((self.numel,))
        nbytes = self.api.size("cfd_fno_workspace_bytes", self.plan, self.sh, 1)
        self.ws = [be.scratch(nbytes) for _ in range(K_)]
        self.preds = [be.out(batch["label"].shape) for _ in range(K_)]
        self.sums = [be.out((4,)) for _ in range(K_)]
        self.coef = [be.out((2,)) for _ in range(K_)]
        self.dx = [be.out(batch["inputs"].shape) for _ in range(2)]
        self.ps, self.as_ = F._flat_struct(be, self.flat, self.layout, L), F._flat_struct(be, self.acc, self.layout, L)
        self.gs = []
        for k in range(1, K_ + 1):
            g = F._flat_struct(be, self.grad, self.layout, L)
            g.d_inputs = be.ptr(self.dx[k % 2]) if k >= 2 else None
            self.gs.append(g)
        self.gs_plain = F._flat_struct(be, self.grad, self.layout, L)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.api.plan_destroy(self.plan)

    def load(self, batch, labels):
        be = self.be
        return (be.dev(batch["inputs"]), be.dev(batch["case_params"]), be.dev(batch["mask"])), [be.dev(a) for a in labels]

    def _accumulate(self, gs, x, dc, dm, k, scale, init, flags=0):
        P = self.be.ptr
        self.api.call("cfd_fno_adam_step", self.plan, self.sh, ctypes.byref(self.as_), ctypes.byref(gs), P(x), P(dc), P(dm), P(self.sums[k]),
                      P(self.ws[k]), P(self.acc), P(self.grad), None, None, self.numel, 0.0, 0.0, 0.0, 0.0, 0.0, 0, float(scale), NMSE, 0,
                      flags | ACC | (INIT if init else 0), self.be.stream)

    def window(self, dev_batch, dev_labels, weight, first, one_pass, detach=False, flags=0):
        """FnoTrainEngine.accumulate_window's calls (K >= 2); `one_pass`: the engine's fused_head.  `flags`: the CFD_TRAIN_DEFER_* bits of
        the truncated window's passes (the engine's defer_flags; the full window always runs with 0)."""
        a, P, K_, L, st = self.api, self.be.ptr, self.K, self.L, self.be.stream
        (di, dc, dm), pr = dev_batch, ctypes.byref(self.ps)
        xs = [di] + self.preds[:-1]
        common = lambda k: (P(xs[k]), P(dc), P(dm), P(dev_labels[k]), P(self.preds[k]))  # noqa: E731
        if detach:
            gr = ctypes.byref(self.gs_plain)
            for k in range(K_):
                if one_pass:
                    a.call("cfd_fno_forward_train_f", self.plan, self.sh, pr, gr, *common(k), P(self.sums[k]), P(self.coef[k]), P(self.ws[k]), NMSE,
                           1.0, 0, flags, st)
                    for phase in range(1, L + 2):
                        a.call("cfd_fno_backward_phase_f", self.plan, self.sh, pr, gr, *common(k), None, P(self.coef[k]), P(self.sums[k]),
                               P(self.ws[k]), phase, NMSE, 0, flags, st)
                else:
                    a.call("cfd_fno_forward", self.plan, self.sh, pr, *common(k), P(self.sums[k]), P(self.ws[k]), 1, st)
                    a.call("cfd_loss_coef", P(self.sums[k]), P(self.coef[k]), NMSE, 1.0, st)
                    a.call("cfd_fno_backward", self.plan, self.sh, pr, gr, *common(k), None, P(self.coef[k]), P(self.ws[k]), st)
                self._accumulate(self.gs_plain, xs[k], dc, dm, k, weight / K_, first and k == 0, flags if one_pass else 0)
            self.be.sync()
            return
        for k in range(K_):
            if k == K_ - 1 and one_pass:
                a.call("cfd_fno_forward_train_f", self.plan, self.sh, pr, ctypes.byref(self.gs[k]), *common(k), P(self.sums[k]), P(self.coef[k]),
                       P(self.ws[k]), NMSE, 1.0 / K_, 0, 0, st)
            else:
                a.call("cfd_fno_forward", self.plan, self.sh, pr, *common(k), P(self.sums[k]), P(self.ws[k]), 1, st)
                a.call("cfd_loss_coef", P(self.sums[k]), P(self.coef[k]), NMSE, 1.0 / K_, st)
        for k in range(K_ - 1, -1, -1):
            gr = ctypes.byref(self.gs[k])
            gext = P(self.dx[k % 2]) if k < K_ - 1 else None  # (0-based k: the d_inputs of step k + 1 is dx[(k + 2) % 2])
            for phase in range(1 if (k == K_ - 1 and one_pass) else 0, L + 2):
                a.call("cfd_fno_backward_phase_f", self.plan, self.sh, pr, gr, *common(k), gext, P(self.coef[k]), P(self.sums[k]), P(self.ws[k]),
                       phase, NMSE, 0, 0, st)
            self._accumulate(self.gs[k], xs[k], dc, dm, k, weight, first and k == K_ - 1)
        self.be.sync()

    def result(self):
        h = lambda b: self.be.host(b).copy()  # noqa: E731
        return dict(acc=h(self.acc), preds=[h(b) for b in self.preds], sums=[h(b) for b in self.sums])

    def tensors(self, flat):
        """{name: array of the parameter's shape and type} of a flat buffer."""
        out = {}
        for q, v in self.params.items():
            sl = F.flat_slice(flat, self.layout, q)
            out[q] = sl.reshape(*v.shape, 2).view(np.complex64).reshape(v.shape) if np.iscomplexobj(v) else sl.reshape(v.shape)
        return out


def compare(rig, got, ref, weight=1.0):
    """{what: nMSE} of a window's result against an fp64 reference: every prediction and, per tensor, the accumulator."""
    res = {f"preds_{k + 1}": nm(got["preds"][k], ref["preds"][k]) for k in range(rig.K)}
    for q in rig.layout:
        res["acc:" + q] = nm(F.flat_slice(got["acc"], rig.layout, q), weight * F.flat_view(ref["grads"][q]))
    return res


def run_case(be, name, one_pass, detach=False, flags=0):
    params, batch, labels, s, K_ = case(name)
    with Rig(be, params, batch, s, K_) as r:
        db, dl = r.load(batch, labels)
        r.window(db, dl, 1.0, True, one_pass, detach, flags)
        return r, r.result()


# ---- the checks -----------------------------------------------------------------------------------------------------------------------
def check_golden(be, one_pass):
    """K = 3 on the reference's own unrolled run (fno_unroll3): the three predictions, the accumulator's sampled entries and the loss."""
    g = IC.load_golden("fno_unroll3")
    params, batch, s = IC.golden_case(g)
    K_, lseed = int(g["meta"][13]), int(g["meta"][14])
    labels = IC.unroll_labels(lseed, batch, K_)
    with Rig(be, params, batch, s, K_) as r:
        db, dl = r.load(batch, labels)
        r.window(db, dl, 1.0, True, one_pass)
        got = r.result()
        res = {"preds": IC.golden_field(g, "preds", np.stack(got["preds"]))}
        res.update(IC.golden_gsums(g, r.tensors(got["acc"])))
        loss = float(np.mean([float(v[0]) / float(v[2]) for v in got["sums"]]))
    assert len([q for q in res if q.startswith("gsum:")]) == len(params), sorted(res)
    return res, abs(loss - float(g["loss"])) / abs(float(g["loss"]))


def check_small(be, name, one_pass):
    r, got = run_case(be, name, one_pass)
    assert np.isfinite(got["acc"]).all(), name
    return compare(r, got, ref_full(name))


def check_two_windows(be, name, one_pass):
    """Two windows, weight 1 / 2 each, the second on another batch and on the first one's dirty workspaces and chained-gradient buffers:
    the accumulator against the mean of the two fp64 gradients, the predictions in the buffers against the second window's."""
    params, batch, labels, s, K_ = case(name)
    _p, batch2, labels2, _s, _k = case(name, bseed=52)
    ref1, ref2 = ref_full(name), ref_full(name, 52)
    with Rig(be, params, batch, s, K_) as r:
        r.window(*r.load(batch, labels), 0.5, True, one_pass)
        r.window(*r.load(batch2, labels2), 0.5, False, one_pass)
        got = r.result()
        mean = dict(preds=ref2["preds"], grads={q: 0.5 * (ref1["grads"][q] + ref2["grads"][q]) for q in ref1["grads"]})
        res = compare(r, got, mean)
        # (so that a second window which overwrote instead of adding, or never ran, is told apart)
        res_first = compare(r, got, dict(preds=ref2["preds"], grads=ref1["grads"]), 0.5)
    assert max(v for q, v in res_first.items() if q.startswith("acc:")) > 1e3 * ABI_TOL, res_first
    return res


def check_poisoned_accumulator_and_repeat(be, name, one_pass):
    """A `first` window never reads the accumulator (it starts as NaN poison and comes out finite), and the same window again -- on the
    dirty workspaces, prediction, sums and chained-gradient buffers -- gives the same bits."""
    params, batch, labels, s, K_ = case(name)
    with Rig(be, params, batch, s, K_) as r:
        assert np.isnan(be.host(r.acc)).all()
        db, dl = r.load(batch, labels)
        r.window(db, dl, 1.0, True, one_pass)
        a = r.result()
        assert np.isfinite(a["acc"]).all() and np.any(a["acc"] != 0.0), name
        r.window(db, dl, 1.0, True, one_pass)
        b = r.result()
    assert same_bits(a["acc"], b["acc"]), f"{name}: two runs of the same window differ"
    assert all(same_bits(x, y) for x, y in zip(a["preds"] + a["sums"], b["preds"] + b["sums"]))


def check_detach(be, name, one_pass, flags=0):
    """The truncated window: (1 / K) sum_k of the one-step fp64 gradients at x_k; and it is not the full gradient."""
    r, got = run_case(be, name, one_pass, detach=True, flags=flags)
    res = compare(r, got, ref_detached(name))
    full = ref_full(name)
    far = max(nm(F.flat_slice(got["acc"], r.layout, q), F.flat_view(full["grads"][q])) for q in r.layout)
    return res, far
