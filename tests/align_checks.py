"""The kernel checks on misaligned buffers: one table (ROWS) of every check function of tests/kernel_checks.py, wide_checks.py,
modes_checks.py and chan_checks.py at the smallest arguments at which the 16-byte route is otherwise taken (H W % 4 == 0, K % 4 == 0,
64 x 64 where the 64-wide kernels are meant), so that the pointer alone decides the route.  Used by tests/test_emul_alignment.py
(CPU: the emulator library built with -fsanitize=alignment, in child processes) and tests/test_gpu_alignment.py (the shipped library).

Placements of a row (tests/backends.py: be.misaligned):
  all4    every dev() / out() / zeros() buffer 4 bytes past a 16-byte boundary (complex and other 8-byte element types: 8)
  all8    every buffer 8 bytes past one (the VEC = 2 forms)
  each4   one run per buffer the check allocates, that buffer alone shifted by 4 (a gate that forgets one of its pointers)
  all0    the default placement (the sanitized run of the same checks must be report-free too)
Every placement must meet the tolerance against the fp64 oracle that the existing test of that check uses at that shape (`accept`).
The contract is the "Alignment" paragraph of include/cfdbench_amd.h; the rows of entry points that refuse a placement name the buffers
(`refuse`: allocation index -> argument name in cfd_last_error(), the status is CFD_ERR_UNSUPPORTED) and the nearest placement the
contract allows (`place4`).  A refusal must come before anything is launched: every output of the refused call still holds the poison
word and the guard bands are intact.

2-byte activation storage (cfd_fno_forward_ex with act_dtype = bf16) lives in the workspace, which is 16-byte aligned by contract: no
tensor argument of the C ABI has 2-byte elements, so the bf16 row shifts the fp32 / complex arguments only."""
from __future__ import annotations

import dataclasses
import json
import sys
import time

import numpy as np

from cfdbench_amd._capi import CfdError
from tests import backends as BK
from tests import chan_checks as CK
from tests import fno_checks as F
from tests import kernel_checks as K
from tests import modes_checks as MK
from tests import wide_checks as WK

UNSUPPORTED = -2  # CFD_ERR_UNSUPPORTED: the one status of a placement an entry point does not take


# -- what the existing test of each check asserts ------------------------------------------------------------------------------
def _all(res, tol):
    bad = {k: v for k, v in res.items() if not (v < tol)}
    assert not bad, f"parity failures (tol {tol}): {bad}; all: {res}"


def tol(t=K.TOL, **keys):
    """All values below `t`; `keys`: a bound of their own for single keys (value < bound), 0.0 = must be exactly zero."""
    def accept(res):
        res = dict(res)
        for k, bound in keys.items():
            v = res.pop(k)
            assert (v == 0.0) if bound == 0.0 else (v < bound), (k, v, bound, res)
        _all(res, t)
    return accept


def head_fwd(res):  # tests/test_emul_fno_chan.py: test_head_fwd_chan
    res = dict(res)
    assert res.pop("count") == 0.0
    sums = [res.pop(f"sum{k}") for k in range(3)]
    assert max(sums) < 1e-10, sums
    _all(res, K.TOL)


def chan_head(res):  # _assert_head
    res = dict(res)
    assert res.pop("sums") < 1e-5 and res.pop("scores", 0.0) < 1e-5, res
    _all(res, K.TOL)


def chan_model(res):  # _assert_model
    res = dict(res)
    assert res.pop("losses") < 1e-5, res
    _all(res, 1e-9)
    assert res["preds"] < K.TOL and res["preds_infer"] < K.TOL, res


def bf16_storage(res):  # test_bf16_activation_storage_forward
    res = dict(res)
    info = {k: v for k, v in res.items() if k.startswith("info:")}
    assert res.pop("bf16_loss") < 1e-5
    _all({k: v for k, v in res.items() if not k.startswith("info:")}, 1e-7)
    assert 1e-7 < info["info:bf16_vs_f32"] < 1e-3


def zero(res):
    assert res == 0, res


def all_zero(res):
    assert all(v == 0 for v in res.values()), res


def below(bound):
    def accept(res):
        assert res < bound, res
    return accept


def dropout_gelu(res):
    bad, err = res
    assert bad == 0 and err < 1e-12, res


def loss_adam(res):
    assert res["sums"] < 1e-5 and res["adam_delta"] < 1e-9, res


def all_true(res):
    assert all(res.values()), res


# -- entry points no check of the four modules calls: the smallest parity check of each, against the same fp64 oracle -------------
def check_loss_sums_bwd(be, n=1028, seed=51):
    """cfd_loss_sums_bwd: gp = gs[0] 2 (p - l) + gs[1] sign(p - l), gl = -gp + gs[2] 2 l."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    p, l, gs = (rng.standard_normal(k).astype(np.float32) for k in (n, n, 4))
    dp, dl, dgs = be.dev(p), be.dev(l), be.dev(gs)
    gp, gl = be.out((n,)), be.out((n,))
    api.call("cfd_loss_sums_bwd", P(dp), P(dl), P(dgs), P(gp), P(gl), n, be.stream)
    be.sync()
    p64, l64, g64 = p.astype(np.float64), l.astype(np.float64), gs.astype(np.float64)
    rgp = g64[0] * 2 * (p64 - l64) + g64[1] * np.sign(p64 - l64)
    return {"gp": K.nm(be.host(gp), rgp), "gl": K.nm(be.host(gl), -rgp + g64[2] * 2 * l64)}


def check_deeponet_inner_ex(be, B=3, P_=24, Kq=64, HW=256, ldu=260, seed=52):
    """cfd_deeponet_inner_fwd_ex: the residual field read at a row stride, with query indices."""
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    br, tr = rng.standard_normal((B, P_)).astype(np.float32), rng.standard_normal((Kq, P_)).astype(np.float32)
    bias, u = rng.standard_normal(1).astype(np.float32), rng.standard_normal((B, ldu)).astype(np.float32)
    q = rng.permutation(HW)[:Kq].astype(np.int32)
    dbr, dtr, dbi, du, dq = be.dev(br), be.dev(tr), be.dev(bias), be.dev(u), be.dev(q)
    preds = be.out((B, Kq))
    api.call("cfd_deeponet_inner_fwd_ex", P(dbr), P(dtr), P(dbi), P(du), ldu, P(dq), P(preds), B, P_, Kq, HW, be.stream)
    be.sync()
    ref = br.astype(np.float64) @ tr.astype(np.float64).T + float(bias[0]) + u.astype(np.float64)[:, q]
    return {"preds": K.nm(be.host(preds), ref)}


def check_fno_train_phases(be, ex, B=1, C=8, L=1, H=64, W=64, p=5, which="nmse", pseed=7, bseed=8):
    """cfd_fno_forward_train + cfd_fno_backward_phase(1 .. L + 1) (`ex`: the _ex forms with fp32 storage): predictions and every parameter
    gradient against the fp64 oracle, as check_fno_vs_oracle holds cfd_fno_forward / cfd_fno_backward."""
    import ctypes

    from cfdbench_amd._capi import FnoShape
    from oracle import fno_oracle as O
    from oracle import synth
    api, P = be.api, be.ptr
    params = synth.make_fno_params(pseed, C, L, 12, 12, p, spectral_gain=4.0)
    batch = synth.make_batch(bseed, B, H, W, p, border_mask=True)
    plan = api.plan_create(H, W, 12, 12)
    try:
        shape = FnoShape(B, H, W, 2, 2, p, C, L, 12, 12, 128)
        pd = {k: be.dev(v) for k, v in params.items()}
        gd = {k: be.out(v.shape, np.complex64 if np.iscomplexobj(v) else np.float32) for k, v in params.items()}
        ps, gs = F.make_param_struct(be, pd, L), F.make_param_struct(be, gd, L)
        ws = be.scratch(api.size("cfd_fno_workspace_bytes", plan, ctypes.byref(shape), 1))
        di, dc, dm, dl = (be.dev(batch[k]) for k in ("inputs", "case_params", "mask", "label"))
        preds, sums, coef = be.out((B, 2, H, W)), be.out((4,)), be.out((2,))
        wid = {"mse": 0, "nmse": 1, "mae": 2}[which]
        sfx, tail = ("_ex", (0,)) if ex else ("", ())
        api.call("cfd_fno_forward_train" + sfx, plan, ctypes.byref(shape), ctypes.byref(ps), ctypes.byref(gs), P(di), P(dc), P(dm), P(dl),
                 P(preds), P(sums), P(coef), P(ws), wid, 1.0, *tail, be.stream)
        for phase in range(1, L + 2):
            api.call("cfd_fno_backward_phase" + sfx, plan, ctypes.byref(shape), ctypes.byref(ps), ctypes.byref(gs), P(di), P(dc), P(dm), P(dl),
                     P(preds), None, P(coef), P(ws), phase, *tail, be.stream)
        be.sync()
        p64 = {k: v.astype(np.complex128 if np.iscomplexobj(v) else np.float64) for k, v in params.items()}
        b64 = {k: v.astype(np.float64) for k, v in batch.items()}
        ref = O.fno_forward(p64, b64["inputs"], b64["case_params"], b64["mask"], b64["label"], L)
        rg = O.fno_backward(p64, ref["cache"], O.loss_grad_wrt_preds(ref["cache"]["preds"], ref["cache"]["label"], which), L)
        res = {"preds": K.nm(be.host(preds), ref["preds"])}
        for k in params:
            res["g:" + k] = K.nm(be.host(gd[k]), rg[k])
        return res
    finally:
        api.plan_destroy(plan)


def check_conv_frag_refusals(be, B=2, Ci=3, Co=12, H=16, W=16, ks=3, seed=53):
    """Prepared weight fragments are scratch() buffers, which the placement policy never shifts: here cfd_conv2d_wprep_batch,
    cfd_conv2d_fwd_ex and cfd_conv2d_bwd_ex get a fragment pointer 4 and 8 bytes past a 16-byte boundary (inside a buffer with room for
    it).  Each must return CFD_ERR_UNSUPPORTED naming the argument and leave the fragment / every output all poison."""
    import ctypes
    api, P = be.api, be.ptr
    rng = np.random.default_rng(seed)
    x = be.dev(rng.standard_normal((B, Ci, H, W)).astype(np.float32))
    w = be.dev(rng.standard_normal((Co, Ci, ks, ks)).astype(np.float32))
    b = be.dev(rng.standard_normal((Co,)).astype(np.float32))
    g = be.dev(rng.standard_normal((B, Co, H, W)).astype(np.float32))
    nf = [api.size("cfd_conv2d_wfrag_bytes", Ci, Co, ks, tr) for tr in (0, 1)]
    assert min(nf) > 0, nf
    frags = [be.scratch(n + 16) for n in nf]
    fws = be.scratch(api.size("cfd_conv2d_fwd_workspace_bytes", B, Ci, Co, H, W, ks))
    bws = be.scratch(api.size("cfd_conv2d_bwd_workspace_bytes", B, Ci, Co, H, W, ks))
    out, gin, gw, gb = be.out((B, Co, H, W)), be.out((B, Ci, H, W)), be.out((Co, Ci, ks, ks)), be.out((Co,))

    def refused(arg, untouched, name, *args):
        try:
            api.call(name, *args)
        except CfdError as e:
            be.sync()
            return (f"(status {UNSUPPORTED})" in str(e) and f"{name.replace('_ex', '')}: {arg} must be 16-byte aligned" in str(e)
                    and all((be.host(t).reshape(-1).view(np.uint32) == BK.POISON_WORD).all() for t in untouched))
        return False

    one = lambda ty, v: (ty * 1)(v)  # noqa: E731
    res = {}
    for off in (4, 8):
        for tr in (0, 1):
            res[f"wprep_tr{tr}_off{off}"] = refused("wfrag[i]", [frags[tr][:nf[tr] // 4 * 4]], "cfd_conv2d_wprep_batch", 1, one(ctypes.c_void_p, P(w)),
                                                   one(ctypes.c_void_p, P(frags[tr]) + off), one(ctypes.c_int, Ci), one(ctypes.c_int, Co),
                                                   one(ctypes.c_int, ks), one(ctypes.c_int, tr), be.stream)
        res[f"fwd_off{off}"] = refused("wfrag", [out], "cfd_conv2d_fwd_ex", P(x), P(w), P(b), P(out), P(fws), None, P(frags[0]) + off,
                                       B, Ci, Co, H, W, ks, be.stream)
        res[f"bwd_off{off}"] = refused("wfrag_t", [gin, gw, gb], "cfd_conv2d_bwd_ex", P(g), P(x), P(w), P(gin), P(gw), P(gb), P(bws),
                                       P(frags[1]) + off, B, Ci, Co, H, W, ks, be.stream)
    return res


@dataclasses.dataclass
class Row:
    id: str
    fn: object
    args: tuple
    accept: object
    kw: dict = dataclasses.field(default_factory=dict)
    knobs: dict = dataclasses.field(default_factory=dict)
    refuse: dict = dataclasses.field(default_factory=dict)  # allocation index -> argument named by the refusal, when shifted by 4
    place4: object = dataclasses.field(default_factory=dict)  # the nearest placement the contract allows under a shift of 4
    min16: bool = False      # the refused buffers need 16 bytes: a shift of 8 is refused like one of 4 (else: 8 bytes are enough)
    refuse8: str = ""        # the argument named under all8 where it is not the one named under all4
    each: bool = True        # the one-buffer-at-a-time sweep applies (False: the check compares two of its own runs bit for bit)
    emul_each: bool = False  # ... and runs on the emulator too (the launchers of this row have a gate or an over-aligned access)

    def run(self, be):
        with K.tuned(be, **self.knobs):
            return self.fn(be, *self.args, **self.kw)


T = K.TOL
HEAD = dict(sums=1e-5, scores=1e-5)
FNO = dict(nmse_loss=1e-5)

ROWS = [
    # ---- tests/kernel_checks.py: the FNO kernels, 64 x 64 (the 64-wide transforms, the v4 / VEC = 4 pointwise forms) -----------
    Row("spectral", K.check_spectral, (2, 3, 5, 64, 64), tol(T), emul_each=True),
    Row("spectral_c20", K.check_spectral, (1, 20, 20, 64, 64), tol(T)),
    Row("mix_wgrad", K.check_mix_wgrad, (3, 20, 20), tol(T), emul_each=True),
    Row("mix_wgrad_mfma", K.check_mix_wgrad, (3, 20, 20), tol(T), knobs=dict(mode_mfma=1, mode_bc=2), emul_each=True),
    Row("block", K.check_block, (1, 6, 7, 32, 64), tol(T), emul_each=True),
    Row("block_c20", K.check_block, (1, 20, 20, 64, 64), tol(T)),
    Row("block_batch_split", K.check_block_batch_split, (5, 2, 20, 64, 64), tol(T, fwd_bitwise=0.0, bwd_bitwise=0.0), each=False),
    Row("idft_epilogues", K.check_idft_epilogues, (3, 64, 64), tol(T), emul_each=True),
    Row("chanmix", K.check_chanmix, (2, 20, 20, 256, True), tol(T), emul_each=True),
    Row("stem", K.check_stem, (2, 64, 64, 5, 20, False), tol(T), emul_each=True),
    Row("head", K.check_head, (2, 20, 256, True, "nmse", False), tol(T, **HEAD), emul_each=True),
    Row("head_ext_tiles", K.check_head, (3, 20, 192, True, "nmse", True), tol(T, **HEAD), knobs=dict(head_blocks=2)),
    Row("head_train", K.check_head_train, (2, 20, 192, True, "nmse"), tol(T, sums=1e-5), knobs=dict(head_blocks=2), emul_each=True),
    Row("loss_and_adam", K.check_loss_and_adam, (), loss_adam, emul_each=True),
    Row("fno", K.check_fno_vs_oracle, (1, 5, 1, 64, 64), tol(1e-9, **FNO)),
    # (the flat parameter and gradient buffers -- allocations 4, 5 and 11, 12 -- hold the complex spectral weights: 8 bytes)
    Row("fno_train_step", K.check_fno_train_step_deferred, (), tol(1e-11, sums=1e-6, preds=0.0),
        kw=dict(B=1, C=8, L=1, H=64, W=64, which="mae"), each=False, place4={4: 8, 5: 8, 11: 8, 12: 8}),
    Row("stem_dft_fusion", K.check_stem_dft_fusion, (2, 20, 2, 5, False), all_zero, each=False),
    Row("fno_bf16_storage", K.check_fno_bf16_storage, (1, 4, 1, 32, 32), bf16_storage, each=False),
    # ---- dense layers -------------------------------------------------------------------------------------------------
    Row("gemm", K.check_gemm, (40, 24, 332, 0, 1), tol(T), emul_each=True),
    Row("gemm_tn", K.check_gemm, (20, 32, 700, 1, 0), tol(T)),
    Row("linear", K.check_linear, (24, 520, 20, "relu"), tol(T), emul_each=True),
    Row("linear_rowgemm6", K.check_linear_rowgemm6, (300, 40, 24, "relu", None), tol(T, y_vs_fp32_kernel=1e-12, gx_vs_fp32_kernel=1e-12),
        emul_each=True),
    Row("linear_chain_bwd", K.check_linear_chain_bwd, (36, 20, 24, "relu"), tol(T, differs_from_two_passes=0.0, gw_differs=0.0), each=False),
    Row("ffn_stack", K.check_ffn_stack, (70, [4, 12, 20, 8], "relu", False, True), tol(T), emul_each=True),
    Row("ffn_stacks", K.check_ffn_stacks, ([(70, [4, 12, 20, 8], "relu", False, True), (33, [4, 16, 8], "gelu", True, False)],), all_zero, each=False),
    Row("deeponet_inner", K.check_deeponet_inner, (3, 24, 256, 256, False), tol(T, gbias=1e-5), emul_each=True),
    Row("deeponet_inner_q", K.check_deeponet_inner, (3, 24, 64, 256, True), tol(T, gbias=1e-5)),
    Row("normact", K.check_normact, (5, (24,), "relu"), tol(T), emul_each=True),
    Row("bcast_rowdot", K.check_bcast_rowdot, (2, 8, 20), tol(T, gbias=1e-5), emul_each=True),
    Row("act", K.check_act, (1000, "gelu"), tol(T), emul_each=True),
    Row("rows_concat2", K.check_rows_concat2, (5, 128, 256, 4, 4), tol(T, differs=0.0), each=False),
    Row("mse_loss_strided", K.check_mse_loss_strided_labels, (7, 128, 256), tol(1e-5, sums_differ=0.0, scores_differ=0.0, gp_differ=0.0), each=False),
    Row("loss_scores_bwd", K.check_loss_scores_bwd, (), below(1e-6), emul_each=True),
    Row("adam_multi", K.check_adam_multi, (), below(2e-6), kw=dict(sizes=(8, 1024, 300, 4)), each=False),
    Row("adam_flat_unaligned", K.check_adam_flat_unaligned, (), zero, each=False),
    Row("scale_copy_multi", K.check_scale_copy_multi, (), zero, kw=dict(sizes=(8, 1024, 300, 4)), each=False),
    # ---- convolutions, BatchNorm, pooling ------------------------------------------------------------------------------
    Row("conv2d_k3", K.check_conv2d, (2, 4, 8, 8, 8, 3), tol(T), emul_each=True),
    Row("conv2d_k1", K.check_conv2d, (2, 4, 8, 8, 8, 1), tol(T), emul_each=True),
    Row("conv2d_k1_wide", K.check_conv2d, (3, 12, 2, 8, 8, 1), tol(T)),
    Row("conv2d_zeropad", K.check_conv2d_zeropad, (3, 8, 7, 6, 6, 3), tol(T), emul_each=True),
    # (8 inputs, then (out, stats, gin, gw, gb) per layer and pass: the first layer's records are allocations 9 and 14)
    Row("conv_prepared", K.check_conv_prepared, ([(2, 3, 12, 16, 16, 3), (1, 8, 16, 12, 12, 7)],), zero, each=False, refuse={9: "stats"},
        place4={9: 0, 14: 0}, min16=True),
    # stats: allocation 11 of the check (7 inputs, out, y, save_mean, save_rstd, stats); records are (m, m2, n, -) 16-byte units
    Row("conv_bn_stats", K.check_conv_bn_stats, (5, 12, 18, 16, 16, 3), tol(T), knobs=dict(conv6_grid=3), refuse={11: "stats"},
        place4={11: 0}, min16=True, emul_each=True),
    Row("batchnorm", K.check_batchnorm, (4, 12, 8, 8, True, True), tol(T), emul_each=True),
    # cfd_convt2_*: out (allocation 4) and gout (3) hold pixel pairs, 8-byte units
    Row("convt", K.check_convt, (3, 24, 12, 16, 16), tol(T), refuse={3: "gout", 4: "out"}, place4={3: 8, 4: 8}, emul_each=True),
    Row("convt_valu", K.check_convt, (3, 24, 12, 16, 16), tol(T), knobs=dict(convt_mfma=0), refuse={3: "gout", 4: "out"}, place4={3: 8, 4: 8}),
    # (allocations 0 .. 5 are the pooling buffers, 6 .. 8 the transposed convolution's x, w, b; its g / out are 9 and 10)
    Row("pool_convt_resid", K.check_pool_convt_resid, (3, 24, 12, 16, 16), tol(T, pool=0.0, pool_bwd=0.0), refuse={9: "gout", 10: "out"},
        place4={9: 8, 10: 8}, emul_each=True),
    # cfd_convt2_*_ex on a channel slice: matrix-pipe kernels only, 16-byte units (under all4 the dense call's `out` is refused first)
    Row("convt_strided", K.check_convt_strided, (2, 20, 8, 4, 8), zero, each=False, refuse={"any": "out"}, refuse8="gout", place4="all0", min16=True),
    Row("upsample_bilinear", K.check_upsample_bilinear, (1, 2, 4, 8), tol(T), emul_each=True),
    # x, gy and the three outputs of the one-pass kernels (allocations 0 .. 3): 16-byte units, no scalar form (cfd_dropout + cfd_gelu_*)
    Row("dropout_gelu", K.check_dropout_gelu, (4 * 1031, 0.2), dropout_gelu, refuse={0: "x", 1: "gy", 2: "y", 3: "gx"},
        place4={0: 0, 1: 0, 2: 0, 3: 0}, min16=True, emul_each=True),
    Row("dropout_step", K.check_dropout_step, (4 * 1031, 0.2, 0x1234567890ABCDEF, 7), zero, each=False, refuse={"any": "x"}, place4="all0", min16=True),
    # ---- the wide route (hidden 64), many modes, channel route (out_chan 3 and 8): smallest existing parametrizations ---------
    Row("wide_mix_wgrad", K.check_mix_wgrad, (2, 64, 64), tol(T)),
    Row("wide_spectral", K.check_spectral, (1, 64, 64, 64, 64), tol(T)),
    Row("wide_chanmix", K.check_chanmix, (2, 64, 64, 132, 1), tol(T), emul_each=True),
    Row("wide_block", K.check_block, (1, 40, 40, 64, 64), tol(T)),
    Row("wide_stem", K.check_stem, (2, 24, 28, 3, 64, True), tol(T)),
    Row("wide_chanmix_fwd", WK.check_chanmix_fwd, (2, 64, 64, 132, 1), tol(T)),
    Row("wide_stem_fwd", WK.check_stem_fwd, (2, 24, 28, 3, 64, True), tol(T)),
    Row("wide_head_fwd", WK.check_head_fwd, (2, 64, 152, 1), head_fwd, emul_each=True),
    Row("wide_head", K.check_head, (2, 64, 152, False, "mse", True), tol(T, **HEAD)),
    Row("wide_head_train", K.check_head_train, (2, 64, 152, False, "mse"), tol(T, sums=1e-5)),
    Row("wide_fno_forward", WK.check_fno_forward_vs_oracle, (1, 64, 2, 64, 64), tol(T), kw=dict(border=True)),
    Row("wide_fno", K.check_fno_vs_oracle, (1, 64, 2, 64, 64), tol(1e-9, **FNO), kw=dict(border=True)),
    Row("wide_refusals", WK.check_wide_refusals, (), all_true, each=False),
    Row("modes_spectral", K.check_spectral, (1, 2, 3, 64, 64, 16, 16), tol(T), emul_each=True),
    Row("modes_idft_epilogues", K.check_idft_epilogues, (3, 64, 64, 16, 16), tol(T)),
    Row("modes_mix_wgrad", K.check_mix_wgrad, (3, 4, 5, 16, 16, 64, 64), tol(T)),
    Row("modes_block", K.check_block, (1, 3, 4, 64, 64, 16, 16), tol(T)),
    Row("modes_fno", MK.check_fno_vs_oracle, (1, 6, 2, 64, 64, 16, 16), tol(1e-9, **FNO)),
    Row("modes_train_step", MK.check_train_step_deferred, (), tol(1e-9, bitwise=0.0), kw=dict(B=1, C=6, L=1, H=64, W=64, m1=20, m2=20),
        each=False, place4={4: 8, 5: 8, 11: 8, 12: 8}),
    Row("modes_refusals", MK.check_refusals, (), all_true, each=False),
    # ---- tests/range_checks.py: shifted buffers put the transforms on their scalar-load forms; these rows take them to a tall grid (the
    #      generic k_dft_fwd / k_idft at T = 6), to a grid with the Nyquist column (NJG = 1) and to the widest grid with 64-column tables,
    #      at full modes (NJ = 5: scalar loads wherever the buffers lie) ------------------------------------------------------------
    Row("range_tall_idft_epilogues", K.check_idft_epilogues, (3, 96, 64, 12, 12), tol(T)),
    Row("range_nyquist_spectral", K.check_spectral, (1, 2, 3, 16, 16, 8, 9), tol(T)),
    Row("range_block_grid_idft_epilogues", K.check_idft_epilogues, (3, 80, 68, 15, 16), tol(T)),
    Row("chan_head_fwd", WK.check_head_fwd, (2, 20, 152, 1), head_fwd, kw=dict(Co=3)),
    Row("chan_head_3", CK.check_head, (2, 20, 152, 0, 3, "nmse"), chan_head, emul_each=True),
    Row("chan_head_8", CK.check_head, (2, 20, 152, 1, 8, "mse"), chan_head),
    Row("chan_head_ext", CK.check_head, (2, 20, 152, 1, 3), chan_head, kw=dict(label_loss=False)),
    Row("chan_head_train_3", CK.check_head_train, (2, 20, 152, 1, 3, "nmse"), chan_head, emul_each=True),
    Row("chan_head_train_8", CK.check_head_train, (2, 20, 152, 0, 8, "mae"), chan_head),
    Row("chan_stem", CK.check_stem, (2, 24, 28, 5, 20, 3), tol(T), emul_each=True),
    Row("chan_fno_3", CK.check_fno_vs_oracle, (2, 20, 2, 24, 28, 3, 3), chan_model),
    Row("chan_fno_8", CK.check_fno_vs_oracle, (2, 20, 2, 24, 28, 8, 8), chan_model),
    Row("chan_train_step", CK.check_fno_train_step, (), tol(1e-9, sums=0.0, preds=0.0, params=0.0, grad_vs_immediate=0.0),
        kw=dict(B=2, C=20, L=2, H=24, W=28, cin=3, cout=3, which="nmse", flags=7), each=False, place4={4: 8, 5: 8, 11: 8, 12: 8}),
    Row("chan_refusals", CK.check_refusals, (), all_true, each=False),
    # ---- entry points the four modules leave out (checks above) ---------------------------------------------------------------
    Row("loss_sums_bwd", check_loss_sums_bwd, (), tol(T), emul_each=True),
    Row("deeponet_inner_ex", check_deeponet_inner_ex, (), tol(T), emul_each=True),
    Row("fno_train_phases", check_fno_train_phases, (False,), tol(1e-9)),
    Row("fno_train_phases_ex", check_fno_train_phases, (True,), tol(1e-9)),
    Row("conv_frag_refusals", check_conv_frag_refusals, (), all_true, each=False),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)

# Check functions that are no row of their own: two run a case at two sizes in one workspace (the dirty-buffer files' subject); the golden
# spectral check has one fixed shape, 66 x 65, whose planes are off the 16-byte grid whatever the pointer (modes_spectral covers the calls).
NOT_ROWS = {"check_dirty_reuse", "check_workspace_across_routes", "check_spectral_golden"}


class _Refused(Exception):
    def __init__(self, name, error):
        super().__init__(f"{name}: {error}")
        self.name, self.error = name, error


class _RefusalProbe:
    """Stands in for be.api while a refusal is expected: a call that raises CfdError must leave every buffer it was handed as it
    found it -- the out() buffers among its arguments that were all poison before the call are all poison after it, and the zeros()
    buffers (accumulated gradients, running statistics, optimizer state) hold the bytes they held."""

    def __init__(self, be):
        self._be, self._api = be, be.api

    def __getattr__(self, name):
        return getattr(self._api, name)

    def call(self, name, *args):
        ptrs = {a for a in args if isinstance(a, int)}
        clean = lambda: {p: what for p, what, h in self._be.payloads("out") if p in ptrs and h.size % 4 == 0 and
                         (h.view(np.uint32) == BK.POISON_WORD).all()}  # noqa: E731
        state = lambda: {p: (what, h.tobytes()) for p, what, h in self._be.payloads("zeros") if p in ptrs}  # noqa: E731
        before, kept = clean(), state()
        try:
            self._api.call(name, *args)
        except CfdError as e:
            self._be.sync()
            after = clean()
            assert after == before, f"{name} refused ({e}) after writing to {sorted(set(before.values()) - set(after.values()))}"
            now = state()
            assert now == kept, f"{name} refused ({e}) after writing to {sorted(w for p, (w, b) in kept.items() if now[p] != (w, b))}"
            raise _Refused(name, e) from e


def expect_refusal(be, row, shift, only, arg):
    """The row under a placement the contract refuses: CFD_ERR_UNSUPPORTED naming `arg`, nothing written, guard bands intact."""
    probe, api = _RefusalProbe(be), be.api
    be.api = probe
    try:
        with be.misaligned(shift, only=only):
            try:
                row.run(be)
            except _Refused as r:
                msg = str(r.error)
                assert f"(status {UNSUPPORTED})" in msg, msg
                named = msg.split("):", 1)[1].split(":", 1)[1]  # "<fn>: <argument> must be N-byte aligned"
                assert any(f" {a} must be " in named for a in ([arg] if isinstance(arg, str) else arg)) and "aligned" in named, (arg, msg)
            else:
                raise AssertionError(f"{row.id}: shift {shift} of buffer {only if only is not None else 'all'} was not refused")
    finally:
        be.api = api
        be.verify()


def _run(be, row, shift, only=None, place=None):
    try:
        with be.misaligned(shift, only=only, place=place):
            res = row.run(be)
            n = be.allocations
    finally:
        be.verify()
    row.accept(res)
    return n


def run_row(be, row, placement):
    """One table row under one placement (module docstring); raises AssertionError / CfdError where it does not hold."""
    if placement == "all0":
        return _run(be, row, 0)
    if placement in ("all4", "all8"):
        shift = int(placement[3])
        if not row.refuse or (shift == 8 and not row.min16):
            return _run(be, row, shift, place=row.place4 if shift == 4 and not row.refuse else None)
        expect_refusal(be, row, shift, None, (shift == 8 and row.refuse8) or sorted(set(row.refuse.values())))  # (whichever comes first)
        if row.place4 == "all0":
            return _run(be, row, 0)
        return _run(be, row, shift, place={k: min(v, shift) if shift == 8 else v for k, v in row.place4.items()})
    assert placement == "each4" and row.each, (row.id, placement)
    n = _run(be, row, 0)
    assert n >= 1 and all(k < n for k in row.refuse), (row.id, n)
    for k in range(n):
        if k in row.refuse:
            expect_refusal(be, row, 4, k, row.refuse[k])
        else:
            try:
                _run(be, row, 4, only=k)
            except Exception as e:
                raise AssertionError(f"{row.id}: buffer {k} of {n} alone shifted by 4 bytes: {type(e).__name__}: {e}") from e
    return n


def placements(row, emul):
    return ["all0", "all4", "all8"] + (["each4"] if row.each and (row.emul_each or not emul) else [])


# -- which row runs an entry point misaligned ------------------------------------------------------------------------------------
def _calls_of(fn, seen=None):
    """Entry points a check function calls, the module-level helpers it reaches included (run_fno, check_convt, ...)."""
    import inspect
    import re
    seen = set() if seen is None else seen
    if fn in seen:
        return set()
    seen.add(fn)
    src = inspect.getsource(fn)
    names = set(re.findall(r"""["'](cfd_\w+)["']""", src))
    names |= {n + "_ex" for n in names if f'"{n}" + sfx' in src}
    mod = sys.modules[fn.__module__]
    for helper in set(re.findall(r"\b([A-Za-z_]\w*)\(", src)) | set(re.findall(r"\b(?:K|WK|MK|CK|F)\.(\w+)\(", src)):
        for m in (mod, K, F):
            h = getattr(m, helper, None)
            if inspect.isfunction(h) and h.__module__.startswith("tests.") and h.__name__ != "tuned":
                names |= _calls_of(h, seen)
    return names


def entry_rows():
    """{entry point: [row ids]} for every entry point a row's check reaches."""
    out = {}
    for r in ROWS:
        for name in _calls_of(r.fn):
            out.setdefault(name, []).append(r.id)
    return out


# -- the child process of tests/test_emul_alignment.py -----------------------------------------------------------------------
def main(argv):
    """python -m tests.align_checks [--sanitize] ROW[:PLACEMENT,...] ...   One JSON line per (row, placement) on stdout."""
    sanitize = "--sanitize" in argv
    be = BK.NumpyBackend(sanitize=sanitize)
    failed = 0
    for spec in (a for a in argv if not a.startswith("--")):
        rid, _, pl = spec.partition(":")
        row = BY_ID[rid]
        for placement in (pl.split(",") if pl else placements(row, True)):
            t0 = time.time()
            sys.stderr.write(f"@@ {rid} {placement}\n")
            sys.stderr.flush()
            try:
                n, err = run_row(be, row, placement), None
            except Exception as e:  # (every failure is reported as a line: the parent asserts)
                n, err = None, f"{type(e).__name__}: {e}"
                failed += 1
            print(json.dumps({"row": rid, "placement": placement, "buffers": n, "error": err, "seconds": round(time.time() - t0, 2)}), flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
