"""The convolution stack (conv6.hip, convt6.hip, conv1.hip and the launchers of conv.hip) held to the fp32-exact class on every
kernel instantiation that can run: one table (ROWS) with a row per live instantiation and per edge the planners make, each row
saying what it reaches -- checked against the planner mirror (tests/conv_plan.py) by tests/test_emul_conv_exact.py -- and a bound
that comes from references only.  Used by tests/test_emul_conv_exact.py (CPU, SIMT emulator) and tests/test_gpu_conv_exact.py (MI355X).

The bound of an output:  max(EXACT_TOL, 2 x nMSE(chain32, ref64))
  ref64    the fp64 oracle (oracle/conv_oracle.py)
  chain32  the same contraction on the same fp32 inputs, accumulated ONE TERM AT A TIME in float32, every product rounded before it
           is added: plain (channel, ky, kx) order for the forward and the input gradient (there with the output pixels that
           replicate padding folds onto one input pixel innermost), (b, y, x) order for the weight and bias gradients, the bias added
           last.  Evaluated in NumPy on a seeded subsample of at most 4096 elements of the output (fewer where the contraction is long:
           samples x terms <= 2^22) -- the figure depends on the length of the contraction and on the data, not on which outputs.
The floor is the EXACT_TOL of the FNO's three-piece kernels.  The factor 2: the kernels add the same products in another, blocked
order, which is no worse than the sequential chain, and the six-product three-piece form leaves ~2^-24 per product, the size of the
one product rounding the chain has.  Nothing here is taken from what a kernel computes.
One exception, on the emulator backend only and for the four outputs of EMUL_ORDER: the emulator's MFMA twin adds an instruction's 32
products one at a time in fp32, and that order -- evaluated in NumPy float32, _seq6 -- is itself over the bound there; those outputs take
twice ITS figure.  The GPU file runs every row at the plain bound.
A row is well-formed only if every bound is below MAX_BOUND = 1e-11, half of the smallest figure the project gives for a lost piece
(2e-11 .. 5e-11), so that a pass excludes one; that limits the weight-gradient rows to about 15 000 pixels (chain nMSE ~ 3.3e-16 x terms).

Row = (B, Ci, Co, H, W, ks, conv6_grid); ks = 2 stands for ConvTranspose2d(2, stride 2), ks = 1 for the 1x1 convolutions;
conv6_grid = -1: the product's default of 512.  Both backends run a row at the SAME grid (the emulator build's default of 2 is not
used), so a row has one plan.  `reach` is what the row is there for, in the mirror's terms:
  fwd / ext     the k_conv6<KS, CC, EXT, MT, NI> instantiation of the forward / of the input gradient on the extended grid
  wg            k_conv6_wgrad<KS, MT, NKY>
  further keys  plan fields or predicates of reach_of() that must hold (the edge named in the comment)"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from oracle import conv_oracle as CO
from tests import conv_plan as CP
from tests import kernel_checks as K
from tests.range_checks import EXACT_TOL

MAX_BOUND = 1e-11
GRID = CP.PRODUCT_GRID
f32, f64 = np.float32, np.float64

Row = namedtuple("Row", "shape mode reach")


def R(*shape, mode="conv", **reach):
    assert len(shape) == 7
    return Row(tuple(shape), mode, reach)


# modes: conv = cfd_conv2d_fwd + cfd_conv2d_bwd (all outputs); zeropad = cfd_conv2d_zeropad_fwd / _bwd; stats = cfd_conv2d_fwd_stats +
# cfd_batchnorm_fwd_stats; gin / gw+gb / gw / gb = cfd_conv2d_bwd asked for that subset only; fwd+gin = forward and input gradient only (the
# rows whose pixel count puts a weight gradient's bound over MAX_BOUND); in+4 = `in` placed 4 bytes past the 16-byte boundary.
ROWS = [
    # ---- k_conv6, KS = 3, CC = 8 (at most 8 contracted channels) ----
    R(1, 3, 5, 1, 1, 3, -1, fwd=(3, 8, 0, 1, 5), ext=(3, 8, 1, 1, 3), wg=(3, 1, 3), fwd_tile=(4, 1, 64), direct=False),
    #   the smallest layer: one pixel; 64 one-row tiles of 4 share a workgroup, 1152 halo slots (NI = 5); nothing to write directly (H < 3)
    R(1, 3, 5, 2, 1, 3, -1, fwd=(3, 8, 0, 1, 3), ext=(3, 8, 1, 1, 3), direct=False),                # NI = 3 at 768 slots exactly (32 x 4 x 6)
    R(16, 3, 33, 65, 1, 3, -1, fwd=(3, 8, 0, 2, 3), ext=(3, 16, 1, 1, 5), wg=(3, 2, 3), ext_ksplit=3, wg_TW=4, fwd_tile=(4, 64, 1)),
    #   MT = 2 from 64 workgroups on (32 tiles x 2 groups); a 65-row column: a ragged second tile; 4-wide weight-gradient tiles
    R(130, 3, 33, 1, 52, 3, -1, fwd=(3, 8, 0, 2, 5), fwd_tile=(32, 1, 8), fwd_ragged_nb=True),         # one-row images: 8 x 3 x 34 = 816 slots under MT = 2
    R(33, 33, 1, 2, 32, 3, -1, ext=(3, 8, 1, 2, 3), fwd=(3, 16, 0, 1, 5), fwd_ksplit=3, direct=False),  # input gradient of a 1-channel head at MT = 2
    # ---- KS = 3, CC = 16 ----
    R(1, 9, 5, 5, 9, 3, -1, fwd=(3, 16, 0, 1, 3), ext=(3, 8, 1, 1, 3), direct=True),                 # the smallest CC = 16 layer with an interior
    R(31, 9, 33, 5, 26, 3, -1, fwd=(3, 16, 0, 2, 3), ext=(3, 16, 1, 1, 3), fwd_ragged_nb=True, ext_ksplit=3),  # NB = 2, 31 images: a half-empty last group
    R(16, 9, 33, 66, 2, 3, -1, fwd=(3, 16, 0, 2, 5), ext=(3, 16, 1, 1, 5), wg_TW=4),                 # 4 x 64 tiles: (6 x 66 -> 448) + 396 slots
    R(64, 33, 9, 1, 31, 3, -1, ext=(3, 16, 1, 2, 3), ext_tile=(33, 3, 2), fwd=(3, 16, 0, 1, 5)),     # a whole 33 x 3 extended image per tile, two per workgroup
    R(130, 33, 9, 7, 1, 3, -1, ext=(3, 16, 1, 2, 5), ext_ragged_nb=True),                            # 4 x 16 tiles of 4 images on the 9 x 3 extended grid
    R(3, 40, 40, 4, 4, 3, -1, fwd=(3, 16, 0, 1, 5), ext=(3, 16, 1, 1, 5), fwd_ksplit=3, ext_ksplit=3, wg=(3, 2, 3), direct=False, wg_TW=4),
    #   a deep U-Net level: split-K both ways (the fold of every pixel, k_splitk_sum), three output-channel groups
    R(20, 96, 40, 4, 4, 3, -1, fwd_ksplit=6, ext_tile=(6, 6, 7), ext_ragged_nb=True, ext_ksplit=3),    # ksplit = 6 of 6 chunks; 6 x 6 extended images, 7 a tile, 20 images
    # ---- KS = 5 ----
    R(1, 3, 5, 5, 1, 5, -1, fwd=(5, 8, 0, 1, 3), ext=(5, 8, 1, 1, 3), wg=(5, 1, 2)),
    R(5, 3, 5, 1, 1, 5, -1, fwd=(5, 8, 0, 1, 5), ext=(5, 8, 1, 1, 5), ext_tile=(5, 5, 10)),          # ten 5 x 5 extended images: 810 slots
    R(16, 3, 33, 65, 1, 5, -1, fwd=(5, 8, 0, 2, 3), wg=(5, 2, 2), ext_ksplit=5),                      # ksplit = nch = 5: one chunk per slice
    R(130, 1, 33, 2, 40, 5, -1, fwd=(5, 8, 0, 2, 5), fwd_tile=(40, 2, 3), fwd_ragged_nb=True),
    #   the only window in which KS = 5 runs MT = 2 with NI = 5: 769 .. 808 slots (3 x 6 x 44 = 792); a whole-image tile, 3 images each
    R(31, 33, 3, 1, 22, 5, -1, ext=(5, 8, 1, 2, 3), fwd=(5, 8, 0, 1, 5), fwd_ksplit=5),
    R(1, 130, 5, 4, 4, 5, -1, fwd_ksplit=9, fwd_ragged_k=True, direct=True),                           # 17 chunks on 9 slices of 2: the last slice has one
    R(1, 121, 5, 4, 4, 5, -1, fwd_ksplit=16, direct=True),                                             # 16 chunks, 16 slices
    # ---- KS = 7 (MT = 1 only) ----
    R(1, 3, 5, 17, 1, 7, -1, fwd=(7, 8, 0, 1, 3), ext=(7, 8, 1, 1, 3), wg=(7, 1, 2)),
    R(1, 1, 1, 2, 2, 7, -1, fwd=(7, 8, 0, 1, 5), ext=(7, 8, 1, 1, 5), direct=False),                 # an image smaller than the kernel, both ways
    R(2, 5, 128, 3, 3, 7, -1, wg=(7, 2, 2), ext_ksplit=16, direct=False),                              # input gradient on 16 slices: an interior exists, yet the full fold
    # ---- the tile search and the fold ----
    R(1, 3, 5, 64, 64, 3, -1, ext_tile=(23, 11, 1), direct=True),                                     # 66 x 66 extended grid: 23 x 11 tiles, not a power of two
    R(1, 3, 5, 4, 64, 3, -1, fwd_tile=(64, 4, 1), ext_tile=(42, 6, 1)),                               # TW = 64
    R(5, 3, 5, 2, 64, 3, -1, fwd_tile=(32, 2, 4), fwd_ragged_nb=True, direct=False),                  # H < 3 at ksplit = 1: k_fold_pad
    R(9, 3, 5, 6, 6, 3, -1, fwd_tile=(6, 6, 7), fwd_ragged_nb=True, wg_TW=4, direct=True),            # whole 6 x 6 images, 7 a workgroup, 9 images; gin direct + k_fold_border
    R(9, 12, 12, 8, 8, 3, -1, ext_tile=(10, 10, 2), ext_ragged_nb=True, direct=True),                 # the 8 x 8 U-Net level: two 10 x 10 extended images a tile
    # ---- persistent workgroups that walk several tiles (the conv6_grid knob) ----
    R(3, 20, 40, 9, 10, 3, 2, fwd_ksplit=2, ext_ksplit=3, fwd_gx=1, fwd_tile=(10, 9, 2)),
    R(2, 12, 12, 33, 32, 3, 3, fwd_gx=3, ext_gx=3, ext_tile=(34, 7, 1), direct=True),
    # ---- cfd_conv2d_bwd asked for a subset of its outputs: the workspace layout and the launch that carries the reduction differ ----
    *[R(9, 12, 12, 8, 8, 3, -1, mode=m, direct=True, wg=(3, 1, 3)) for m in ("gin", "gw+gb", "gw", "gb")],       # reduction rides in k_fold_border / runs alone
    *[R(3, 40, 40, 4, 4, 3, -1, mode=m, direct=False, wg=(3, 2, 3)) for m in ("gin", "gw+gb", "gw", "gb")],     # full fold: the weight gradient runs after it
    # ---- zero padding (cfd_conv2d_zeropad_*) ----
    R(3, 8, 7, 6, 5, 3, -1, mode="zeropad", zeropad=True, wg_TW=4),
    R(2, 5, 8, 9, 10, 5, -1, mode="zeropad", zeropad=True),
    R(2, 3, 8, 8, 9, 7, -1, mode="zeropad", zeropad=True),
    R(9, 12, 12, 8, 8, 3, -1, mode="zeropad", zeropad=True, ext_tile=(10, 10, 2)),
    # ---- the forward that emits BatchNorm statistics: k_conv6<3, MT, CC, false, 3, true> ----
    R(9, 3, 5, 8, 8, 3, -1, mode="stats", stats=("stats", 8, 1)),                                       # (three slots; a channel needs pixels for its variance to mean something)
    R(16, 3, 33, 65, 1, 3, -1, mode="stats", stats=("stats", 8, 2)),
    R(1, 9, 5, 5, 9, 3, -1, mode="stats", stats=("stats", 16, 1)),
    R(31, 9, 33, 5, 26, 3, -1, mode="stats", stats=("stats", 16, 2)),
    # ---- ConvTranspose2d(2, 2): k_convt6<BWD, 3, 4, false> (NT4) / <BWD, 3, 1, true> (KSPL), k_convt6_wgrad and the fp32 k_conv_wgrad<true> ----
    R(3, 20, 9, 4, 8, 2, -1, convt_fwd="KSPL", convt_bwd="KSPL", convt_wg="k_convt6_wgrad"),
    R(2, 3, 192, 63, 65, 2, -1, mode="fwd+gin", convt_fwd="NT4", convt_bwd="KSPL"),                  # 48 row tiles: 16 groups x 32 pixel blocks = 512 workgroups
    R(8, 145, 2, 63, 65, 2, -1, mode="fwd+gin", convt_fwd="KSPL", convt_bwd="NT4"),                  # 128 pixel blocks (the last ragged) x 4 groups
    R(2, 7, 5, 4, 6, 2, -1, convt_wg="fp32"),                                                         # W % 4 != 0
    R(1, 7, 5, 3, 4, 2, -1, convt_wg="fp32"),                                                         # H W % 8 != 0
    R(3, 20, 9, 4, 8, 2, -1, mode="in+4", convt_wg="fp32"),                                           # misaligned `in`
    R(2, 50, 26, 8, 8, 2, -1, convt_wg="k_convt6_wgrad", convt_emul_fwd="NT4", convt_emul_bwd="NT4"),  # several row / column groups; NT4 on the emulator build
    # ---- 1x1: k_conv1<DG, 3, 4, false> (NT4) / <DG, 3, 1, true> (KSPL), k_conv1_wgrad and the fp32 k_conv_wgrad<false> ----
    R(2, 11, 64, 4, 8, 1, -1, conv1_fwd="KSPL", conv1_bwd="KSPL", conv1_wg="k_conv1_wgrad"),
    R(8, 145, 146, 63, 65, 1, -1, mode="fwd+gin", conv1_fwd="NT4", conv1_bwd="NT4"),
    R(5, 3, 7, 3, 5, 1, -1, conv1_wg="fp32"),                                                         # H W % 8 != 0
    R(2, 11, 64, 4, 8, 1, -1, mode="in+4", conv1_wg="fp32"),                                          # misaligned `in`
    R(2, 50, 50, 2, 8, 1, -1, conv1_wg="k_conv1_wgrad", conv1_emul_fwd="NT4", conv1_emul_bwd="NT4"),
]
assert len({(r.shape, r.mode) for r in ROWS}) == len(ROWS)

# k_conv6 instantiations conv6_launch can name but conv6_plan never selects, on any shape the ABI accepts (the key does not depend on
# conv6_grid).  Confirmed by running the mirror over EVERY image size 1 .. 128 x 1 .. 128, every batch that changes a tile (1 .. 64, 130) and
# both sides of every channel threshold; tests/test_emul_conv_exact.py checks that the sweep of tests/conv_plan.py (the one the mirror
# is pinned on) selects all the others and none of these.
_KS7_MT2 = ("13 k-steps x 2 tiles x 3 KiB of fragments are 79 872 bytes; the smallest halo (NB = 1, 7 x 10 pixels, 3 pieces x 8 channels x 2 bytes) "
            "adds 3360 + 208 of offsets: over CFD_CONV6_MAX_LDS = 81 920, so mtw falls back to 1")
_KS3_CC8_EXT = ("NI = 5 needs more than 768 halo slots, i.e. a halo over 3x the tile's 256 pixels; the extended grid is at least 3 x 3, so the power-of-two "
                "tile is at least 4 x 4 (2.25x), a whole-image tile at least 3 x 3 (2.78x), any other searched tile has 128 pixels or more in at most 64 columns (2.1x)")
_KS5_EXT_MT2 = ("MT = 2 fits CFD_CONV6_MAX_LDS only up to 808 halo slots, NI = 5 starts at 769; on an extended grid (at least 5 x 5) the only tiles over 768 "
                "are 64 x 2 of two images (816) and ten 5 x 5 whole images (810)")
DEAD = {
    (7, 8, 0, 2, 3): _KS7_MT2, (7, 8, 0, 2, 5): _KS7_MT2, (7, 8, 1, 2, 3): _KS7_MT2, (7, 8, 1, 2, 5): _KS7_MT2,
    (3, 8, 1, 1, 5): _KS3_CC8_EXT, (3, 8, 1, 2, 5): _KS3_CC8_EXT,
    (5, 8, 1, 2, 5): _KS5_EXT_MT2,
}
LIVE = [k for k in CP.ALL_CONV6_KEYS if k not in DEAD]


def reach_of(row, emul=False):
    """What the mirror says a row reaches, under the names `reach` uses."""
    B, Ci, Co, H, W, ks, gk = row.shape
    grid = CP.resolve_grid(gk, GRID)
    out = {}
    if ks == 2:
        nt4 = CP.EMUL_NT4_MIN_WGS if emul else CP.NT4_MIN_WGS
        wg = CP.convt6_wg_plan(B, Ci, Co, H, W)
        out.update(convt_fwd=CP.convt6_form(B, Ci, Co, H, W, False, nt4)[2], convt_bwd=CP.convt6_form(B, Ci, Co, H, W, True, nt4)[2],
                   convt_wg=wg.key if wg.ok and row.mode != "in+4" else "fp32")
        out.update(convt_emul_fwd=CP.convt6_form(B, Ci, Co, H, W, False, CP.EMUL_NT4_MIN_WGS)[2],
                   convt_emul_bwd=CP.convt6_form(B, Ci, Co, H, W, True, CP.EMUL_NT4_MIN_WGS)[2])
        return out
    if ks == 1:
        nt4 = CP.EMUL_NT4_MIN_WGS if emul else CP.NT4_MIN_WGS
        wg = CP.conv1_wg_plan(B, Ci, Co, H * W)
        out.update(conv1_fwd=CP.conv1_form(B, Ci, Co, H * W, False, nt4)[2], conv1_bwd=CP.conv1_form(B, Ci, Co, H * W, True, nt4)[2],
                   conv1_wg=wg.key if wg.ok and row.mode != "in+4" else "fp32")
        out.update(conv1_emul_fwd=CP.conv1_form(B, Ci, Co, H * W, False, CP.EMUL_NT4_MIN_WGS)[2],
                   conv1_emul_bwd=CP.conv1_form(B, Ci, Co, H * W, True, CP.EMUL_NT4_MIN_WGS)[2])
        return out
    for name, ext in (("fwd", False), ("ext", True)):
        P = CP.conv6_plan(B, Ci, Co, H, W, ks, ext, grid)
        out[name] = P.key
        out[name + "_tile"] = (P.TW, P.TH, P.NB)
        out[name + "_ksplit"] = P.ksplit
        out[name + "_ragged_k"] = P.ksplit > 1 and P.nch % P.ksplit != 0
        out[name + "_ragged_nb"] = P.NB > 1 and B % P.NB != 0
        out[name + "_gx"] = P.gx
    wg = CP.wg6_plan(B, Ci, Co, H, W, ks, grid)
    out.update(wg=wg.key, wg_TW=wg.TW, direct=CP.gin_direct(B, Ci, Co, H, W, ks, grid), zeropad=CP.zeropad_covers(B, Ci, Co, H, W, ks, grid),
               stats=CP.stats_key(CP.conv6_plan(B, Ci, Co, H, W, ks, False, grid)))
    return out


def instantiations(row, emul=False):
    """The set of kernel instantiations a row RUNS (its mode decides which passes it calls)."""
    r, m = reach_of(row, emul), row.mode
    ks = row.shape[5]
    fwd, gin, gw = m in ("conv", "zeropad", "fwd+gin", "in+4", "stats"), m in ("conv", "zeropad", "fwd+gin", "in+4", "gin"), m in ("conv", "zeropad", "in+4", "gw+gb", "gw")
    if m == "stats":
        return {r["stats"]}
    s = set()
    if ks == 2:
        return s | ({("k_convt6", 0, r["convt_fwd"])} if fwd else set()) | ({("k_convt6", 1, r["convt_bwd"])} if gin else set()) | (
            {("convt_wg", r["convt_wg"])} if gw else set())
    if ks == 1:
        return s | ({("k_conv1", 0, r["conv1_fwd"])} if fwd else set()) | ({("k_conv1", 1, r["conv1_bwd"])} if gin else set()) | (
            {("conv1_wg", r["conv1_wg"])} if gw else set())
    return s | ({r["fwd"]} if fwd else set()) | ({r["ext"]} if gin else set()) | ({("wgrad",) + r["wg"]} if gw else set())


STREAM_KEYS = [(k, d, f) for k in ("k_convt6", "k_conv1") for d in (0, 1) for f in ("NT4", "KSPL")] + [
    (k, f) for k, f in (("convt_wg", "k_convt6_wgrad"), ("convt_wg", "fp32"), ("conv1_wg", "k_conv1_wgrad"), ("conv1_wg", "fp32"))]
EVERY_LIVE = LIVE + CP.ALL_STATS_KEYS + CP.ALL_WGRAD_KEYS + STREAM_KEYS


# ---- inputs: what the helpers of tests/kernel_checks.py draw for (shape, seed); the emulator test checks that they still agree ----
SEED = 31


def inputs_of(row):
    B, Ci, Co, H, W, ks, _ = row.shape
    if row.mode == "stats":
        rng = np.random.default_rng(36)
        x = rng.standard_normal((B, Ci, H, W)).astype(f32)
        w = (rng.standard_normal((Co, Ci, ks, ks)) / np.sqrt(Ci * ks * ks)).astype(f32)
        b = (rng.standard_normal((Co,)) * 0.2 + 3.0 * rng.standard_normal((Co,))).astype(f32)
        return dict(x=x, w=w, b=b)
    if ks == 2:
        rng = np.random.default_rng(34)
        x = np.maximum(rng.standard_normal((B, Ci, H, W)), 0).astype(f32)
        w = (rng.standard_normal((Ci, Co, 2, 2)) / np.sqrt(Ci)).astype(f32)
        b = rng.standard_normal((Co,)).astype(f32) * 0.1
        return dict(x=x, w=w, b=b, g=rng.standard_normal((B, Co, 2 * H, 2 * W)).astype(f32))
    rng = np.random.default_rng(41 if row.mode == "zeropad" else SEED)
    x = rng.standard_normal((B, Ci, H, W)).astype(f32)
    w = (rng.standard_normal((Co, Ci, ks, ks)) / np.sqrt(Ci * ks * ks)).astype(f32)
    b = rng.standard_normal((Co,)).astype(f32) * 0.2
    return dict(x=x, w=w, b=b, g=rng.standard_normal((B, Co, H, W)).astype(f32))


def outputs_of(row):
    """The outputs a row asserts at its bound."""
    pre = "convt_" if row.shape[5] == 2 else ""
    fwd = "convt" if row.shape[5] == 2 else "out"
    return {"conv": (fwd, pre + "gin", pre + "gw", pre + "gb"), "in+4": (fwd, pre + "gin", pre + "gw", pre + "gb"), "zeropad": ("out", "gin", "gw", "gb"),
            "stats": ("out",), "fwd+gin": (fwd, pre + "gin"), "gin": ("gin",), "gw+gb": ("gw", "gb"), "gw": ("gw",), "gb": ("gb",)}[row.mode]


def refs_of(row, I):
    """name -> fp64 oracle result, for the outputs the row asserts."""
    x, w, b = (I[k].astype(f64) for k in ("x", "w", "b"))
    ks, names, ref = row.shape[5], outputs_of(row), {}
    if ks == 2:
        if "convt" in names:
            ref["convt"] = CO.convt2(x, w, b)
        if len(names) > 1 or names[0] != "convt":
            ref["convt_gin"], ref["convt_gw"], ref["convt_gb"] = CO.convt2_bwd(I["g"].astype(f64), x, w)
    elif row.mode == "zeropad":
        p = ks // 2
        pad4 = ((0, 0), (0, 0), (p, p), (p, p))
        xp, gp = np.pad(x, pad4), np.pad(I["g"].astype(f64), pad4)
        ref["out"] = CO.conv2d(xp, w, b)[:, :, p:-p, p:-p]
        gx, ref["gw"], ref["gb"] = CO.conv2d_bwd(gp, xp, w)
        ref["gin"] = gx[:, :, p:-p, p:-p]
    else:
        if "out" in names:
            ref["out"] = CO.conv2d(x, w, b)
        if names != ("out",):
            ref["gin"], ref["gw"], ref["gb"] = CO.conv2d_bwd(I["g"].astype(f64), x, w)
    return {k: ref[k] for k in names}


# ---- chain32 ----
MAX_SAMPLES, MAX_WORK = 4096, 1 << 22


def _sample(shape, nterms, rng):
    size = int(np.prod(shape))
    n = min(MAX_SAMPLES, size, max(16, MAX_WORK // max(nterms, 1)))
    flat = np.sort(rng.choice(size, n, replace=False)) if n < size else np.arange(size)
    return flat, np.unravel_index(flat, shape)


def _seq32(A, Bm, last=None):
    """sum_k A[:, k] Bm[:, k] one term at a time in float32, product rounded first; `last` is added at the end."""
    A, Bm = np.ascontiguousarray(A.T, f32), np.ascontiguousarray(Bm.T, f32)
    acc = np.zeros(A.shape[1], f32)
    for k in range(A.shape[0]):
        acc += A[k] * Bm[k]
    return acc + last.astype(f32) if last is not None else acc


def three_pieces(a):
    """cfd_split8x3: truncating bf16 pieces, p[0] + p[1] + p[2] == a exactly."""
    a = np.ascontiguousarray(a, f32)
    top = lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(f32)
    hi = top(a)
    mid = top(a - hi)
    return hi, mid, a - hi - mid


PIECE_PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))  # PA[] / PB[] of conv6.hip: the six products, small terms first


def _seq6(A, Bm, last=None):
    """The order of the EMULATOR's twin of v_mfma_f32_16x16x32_bf16 (tests/emul/include/cfd_intrinsics.h: "the hardware's internal
    summation order is not architected, so the emulator sums in k order in fp32"): the terms in k-steps of 32, per k-step the six piece
    products one after the other, each added to the fp32 accumulator one slot at a time -- six roundings of the accumulator per
    term where the sequential chain has one.  (bf16 x bf16 is exact in fp32.)"""
    pa, pb = three_pieces(A.T), three_pieces(Bm.T)
    acc = np.zeros(A.shape[0], f32)
    for k0 in range(0, A.shape[1], 32):
        for i, j in PIECE_PRODUCTS:
            for k in range(k0, min(k0 + 32, A.shape[1])):
                acc += pa[i][k] * pb[j][k]
    return acc + last.astype(f32) if last is not None else acc


@functools.lru_cache(maxsize=None)
def _fold_pairs(y, H, ks, zpad):
    """(tap, output pixel) pairs along one axis whose tap reads input pixel y: clamp(p + k - pad) == y (zero padding: p + k - pad == y)."""
    pad = ks // 2
    prs = []
    for k in range(ks):
        for p in sorted({min(max(y - k + pad + d, 0), H - 1) for d in range(-pad, pad + 1)}):
            q = p + k - pad
            if (q == y) if zpad else (min(max(q, 0), H - 1) == y):
                prs.append((k, p))
    return tuple(prs)


def _pairs_table(ys, H, ks, zpad):
    prs = [_fold_pairs(int(y), H, ks, zpad) for y in ys]
    L = max(len(p) for p in prs)
    kk, pp, ok = (np.zeros((len(ys), L), np.int64) for _ in range(3))
    for s, p in enumerate(prs):
        if p:
            kk[s, :len(p)], pp[s, :len(p)], ok[s, :len(p)] = [a for a, _ in p], [c for _, c in p], 1
    return kk, pp, ok.astype(f32)


def chain32(row, I, name, seed=0, how=None):
    """(flat indices into output `name`, its chain32 values there).  `how`: the evaluation of sum_k A[:, k] Bm[:, k] (+ last), _seq32 unless given."""
    how = how or _seq32
    rng = np.random.default_rng([seed, len(name)] + list(row.shape[:6]))
    x, w, b, g = I["x"], I["w"], I["b"], I.get("g")
    B, Ci, Co, H, W, ks, _ = row.shape
    n4 = lambda *a: [v[:, None, None, None] for v in a]
    if ks == 2:
        if name == "convt":
            flat, (sb, so, sy, sx) = _sample((B, Co, 2 * H, 2 * W), Ci, rng)
            return flat, how(x[sb, :, sy // 2, sx // 2], w[:, so, sy % 2, sx % 2].T, b[so])
        if name == "convt_gin":
            flat, (sb, si, sy, sx) = _sample((B, Ci, H, W), 4 * Co, rng)
            sb4, sy4, sx4 = n4(sb, sy, sx)
            o, ky, kx = np.arange(Co)[None, :, None, None], np.arange(2)[None, None, :, None], np.arange(2)[None, None, None, :]
            return flat, how(g[sb4, o, 2 * sy4 + ky, 2 * sx4 + kx].reshape(len(flat), -1), w[si].reshape(len(flat), -1))
        if name == "convt_gw":
            flat, (si, so, sky, skx) = _sample((Ci, Co, 2, 2), B * H * W, rng)
            A = np.stack([x[:, i].reshape(-1) for i in si])
            return flat, how(A, np.stack([g[:, o, ky::2, kx::2].reshape(-1) for o, ky, kx in zip(so, sky, skx)]))
        flat, (so,) = _sample((Co,), B * 4 * H * W, rng)
        A = np.stack([g[:, o].reshape(-1) for o in so])
        return flat, how(A, np.ones_like(A))
    zpad = row.mode == "zeropad"
    p = ks // 2
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)), mode="constant" if zpad else "edge")
    if name == "out":
        flat, (sb, so, sy, sx) = _sample((B, Co, H, W), Ci * ks * ks, rng)
        sb4, sy4, sx4 = n4(sb, sy, sx)
        c, ky, kx = np.arange(Ci)[None, :, None, None], np.arange(ks)[None, None, :, None], np.arange(ks)[None, None, None, :]
        return flat, how(w[so].reshape(len(flat), -1), xp[sb4, c, sy4 + ky, sx4 + kx].reshape(len(flat), -1), b[so])
    if name == "gin":
        L = (p + 1) * (p + 2) // 2 if p else 1
        flat, (sb, si, sy, sx) = _sample((B, Ci, H, W), Co * max(L, ks) ** 2, rng)
        ky, py, oky = _pairs_table(sy, H, ks, zpad)
        kx, px, okx = _pairs_table(sx, W, ks, zpad)
        o = np.arange(Co)[None, :, None, None]
        A = w[o, si[:, None, None, None], ky[:, None, :, None], kx[:, None, None, :]] * (oky[:, None, :, None] * okx[:, None, None, :])
        Bm = g[sb[:, None, None, None], o, py[:, None, :, None], px[:, None, None, :]]
        return flat, how(A.reshape(len(flat), -1), Bm.reshape(len(flat), -1))
    if name == "gw":
        flat, (so, si, sky, skx) = _sample((Co, Ci, ks, ks), B * H * W, rng)
        A = np.stack([g[:, o].reshape(-1) for o in so])
        return flat, how(A, np.stack([xp[:, i, ky:ky + H, kx:kx + W].reshape(-1) for i, ky, kx in zip(si, sky, skx)]))
    flat, (so,) = _sample((Co,), B * H * W, rng)
    A = np.stack([g[:, o].reshape(-1) for o in so])
    return flat, how(A, np.ones_like(A))


def nmse(a, ref):
    a, ref = np.asarray(a, f64), np.asarray(ref, f64)
    return float(((a - ref) ** 2).sum() / max((ref ** 2).sum(), 1e-300))


# Outputs that exceed their bound on the EMULATOR only, because of the order in which its MFMA twin adds (see _seq6): evaluated in NumPy
# float32, that order alone is over the bound on each of them (tests/test_emul_conv_exact.py asserts it), so on that backend their bound
# is 2 x the figure of that order.  On the GPU -- whose matrix pipe adds the 32 products of an instruction before it rounds into the
# accumulator -- they keep the plain bound like every other row.  Longest contractions of the three-piece kernels in the table next to the floor:
EMUL_ORDER = {
    ((2, 5, 128, 3, 3, 7, -1), "conv"): ("out",),               # 245 terms in 16 output-channel groups x 13 k-steps
    ((2, 5, 8, 9, 10, 5, -1), "zeropad"): ("gin",),             # 200 terms
    ((2, 3, 8, 8, 9, 7, -1), "zeropad"): ("gin",),              # 392 terms
    ((2, 3, 192, 63, 65, 2, -1), "fwd+gin"): ("convt_gin",),    # 768 terms
}


def bounds_of(row, backend="gpu"):
    """name -> (bound, nMSE of the reference order it comes from) for every output the row asserts; computed once per row and process."""
    bd = dict(_bounds_of(row.shape, row.mode))
    if backend == "emul":
        bd.update(_emul_bounds_of(row.shape, row.mode))
    return bd


@functools.lru_cache(maxsize=None)
def _bounds_of(shape, mode):
    row = Row(shape, mode, None)
    I = inputs_of(row)
    ref = refs_of(row, I)
    out = {}
    for name in outputs_of(row):
        flat, c = chain32(row, I, name)
        e = nmse(c, ref[name].reshape(-1)[flat])
        out[name] = (max(EXACT_TOL, 2.0 * e), e)
    return out


@functools.lru_cache(maxsize=None)
def _emul_bounds_of(shape, mode):
    row = Row(shape, mode, None)
    names = EMUL_ORDER.get((shape, mode), ())
    if not names:
        return {}
    I = inputs_of(row)
    ref = refs_of(row, I)
    out = {}
    for name in names:
        flat, c = chain32(row, I, name, how=_seq6)
        e = nmse(c, ref[name].reshape(-1)[flat])
        out[name] = (2.0 * e, e)
    return out


# ---- running a row on a backend ----
def run_row(be, row):
    """name -> (kernel nMSE against the fp64 oracle, bound) for the row's asserted outputs, plus "other": what the helper returned
    for the outputs that keep their present bound (K.TOL), and "inputs_agree"."""
    B, Ci, Co, H, W, ks, gk = row.shape
    keep, m = {}, row.mode
    want = {"gin": ("gin",), "gw+gb": ("gw", "gb"), "gw": ("gw",), "gb": ("gb",), "fwd+gin": ("gin",)}.get(m, ("gin", "gw", "gb"))
    with K.tuned(be, conv6_grid=CP.resolve_grid(gk, GRID)):
        if ks == 2:
            res = K.check_convt(be, B, Ci, Co, H, W, keep=keep, want=want, shift_in=4 if m == "in+4" else 0)
        elif m == "zeropad":
            res = K.check_conv2d_zeropad(be, B, Ci, Co, H, W, ks, keep=keep)
        elif m == "stats":
            res = K.check_conv_bn_stats(be, B, Ci, Co, H, W, ks, keep=keep)
        else:
            res = K.check_conv2d(be, B, Ci, Co, H, W, ks, seed=SEED, keep=keep, want=want, shift_in=4 if m == "in+4" else 0)
    assert res is not None, "the layer is not covered by the entry the row is about"
    I = inputs_of(row)
    agree = all(np.array_equal(I[k], keep[k]) for k in I)
    bd = bounds_of(row, be.name)
    names = outputs_of(row)
    out = {n: (res[n], bd[n][0]) for n in names}
    out["other"] = {k: v for k, v in res.items() if k not in names}
    out["inputs_agree"] = agree
    out["untouched"] = all(np.all(v.view(np.uint32) == 0x7FC07FC0) for v in keep.get("untouched", {}).values())
    return out


def assert_row(res, row):
    assert res.pop("inputs_agree"), "tests/conv_exact_checks.inputs_of no longer draws what tests/kernel_checks.py draws"
    assert res.pop("untouched"), "an output that was not asked for was written"
    other = res.pop("other")
    bad = {k: v for k, v in other.items() if not (v < K.TOL)}
    assert not bad, (row.shape, row.mode, bad)
    print(row.shape, row.mode, {k: f"{v[0]:.2e} / {v[1]:.2e}" for k, v in res.items()})
    bad = {k: v for k, v in res.items() if not (v[0] < v[1])}
    assert not bad, (row.shape, row.mode, "kernel nMSE, bound:", bad)


# ---- what a lost third piece looks like, from references only ----
def bf16_round(a):
    u = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(f32)


def two_pieces(a):
    hi = bf16_round(a)
    return hi + bf16_round(a - hi)
