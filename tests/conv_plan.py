"""A pure-Python mirror of the host-side planners of the convolution stack: which kernel instantiation a shape runs and with what
plan.  No GPU, no library: tests/test_cpu_conv_plan.py pins it to the real host code, tests/conv_exact_checks.py uses it to say what
every row of its table reaches.

Mirrored (cfdbench_amd/csrc): cfd_conv_tile_shape (conv.hip); conv6_frag, conv6_plan, wg6_plan, cfd_conv6_zeropad_covers
(conv6.hip); the NT4 / KSPL choice of convt6_launch and convt6_wg_plan (convt6.hip); the same of conv1_launch and conv1_wg_plan
(conv1.hip); wgrad_plan, chan_sum_ws_bytes and the workspace formulas of the C ABI (conv.hip).

`grid` is the number of persistent workgroups of a conv6 launch, resolved: the conv6_grid knob where it is positive, else the build's
CFD_CONV6_GRID (512 in the product, 2 in the emulator build) -- resolve_grid().

What the C ABI shows of a plan, and so what the sweep of tests/test_cpu_conv_plan.py can pin:
  cfd_conv2d_fwd_workspace_bytes - cfd_conv2d_wfrag_bytes(.., 0)          coverage and ksplit of the forward (with B, Co, H, W known)
  cfd_conv2d_bwd_workspace_bytes                                          the same of the input gradient (its fragments: CC, KSTEPS,
                                                                          MTall, nch), the weight gradient's pixel groups
  cfd_conv2d_fwd_stats_slots                                              gx, where ks = 3, ksplit = 1 and NI = 3 (0 otherwise: so NI at ks = 3)
  cfd_conv2d_zeropad_supported                                            coverage of all three passes, ksplit of the input gradient
  cfd_convt2_bwd_workspace_bytes                                          convt6_wg_plan's groups
NOT observable through any entry: the tile (TW, TH, NB) except through gx and ksplit, MT (mtw), NI at ks = 5 / 7 and in the input-gradient
direction, and the NT4 / KSPL form of k_convt6 / k_conv1.  For those this mirror, written from the planner's text, is the only witness."""
from __future__ import annotations

import functools
import random
from collections import namedtuple

MAX_LDS = 80 * 1024        # CFD_CONV6_MAX_LDS
MT2_MIN_WGS = 64           # CFD_CONV6_MT2_MIN_WGS
PRODUCT_GRID = 512         # CFD_CONV6_GRID of the product build
EMUL_GRID = 2              # ... of tests/emul/build_emul.py
NT4_MIN_WGS = 512          # CFD_CONVT6_NT4_MIN_WGS / CFD_CONV1_NT4_MIN_WGS of the product build
EMUL_NT4_MIN_WGS = 2       # ... of the emulator build
BN_SPLIT = 64


def resolve_grid(knob, build_default=PRODUCT_GRID):
    return knob if knob > 0 else build_default


def align_up(n, a=256):
    return (n + a - 1) // a * a


def cdiv(a, b):
    return (a + b - 1) // b


@functools.lru_cache(maxsize=None)
def _tile_shape(Hd, Wd, Bc):
    TW = 32 if Wd >= 32 else (16 if Wd > 8 else (8 if Wd > 4 else 4))
    rows = 256 // TW
    th = 1
    while th < min(Hd, rows):
        th <<= 1
    TH = min(th, rows)

    def cost(tw, thh):
        nb = 256 // (tw * thh)
        return float(cdiv(Wd, tw)) * cdiv(Hd, thh) / float(min(nb, Bc))

    best = cost(TW, TH) * 0.97
    btw, bth = TW, TH
    for tw in range(4, min(64, Wd) + 1):
        for thh in range(1, min(256 // tw, Hd) + 1):
            if tw * thh < 128 and not (tw == Wd and thh == Hd):
                continue
            c = cost(tw, thh)
            if c < best - 1e-9 or (c < best + 1e-9 and tw > btw):
                best, btw, bth = c, tw, thh
    return btw, bth, 256 // (btw * bth)


def tile_shape(Hd, Wd, B):
    """cfd_conv_tile_shape: (TW, TH, NB).  (NB <= 64, so a batch above 64 costs what 64 does.)"""
    return _tile_shape(Hd, Wd, min(B, 64))


Frag = namedtuple("Frag", "CC KSTEPS MTall nch bytes ok")


def conv6_frag(Ci, Co, ks, ext):
    if ks not in (3, 5, 7) or Ci < 1 or Co < 1:
        return Frag(0, 0, 0, 0, 0, False)
    Cm, Cs = (Ci, Co) if ext else (Co, Ci)
    CC = 8 if (ks >= 5 or Cs <= 8) else 16
    PPS = 32 // CC
    KSTEPS = cdiv(ks * ks, PPS)
    MTall = cdiv(Cm, 16)
    nch = cdiv(Cs, CC)
    return Frag(CC, KSTEPS, MTall, nch, align_up(nch * KSTEPS * MTall * 3 * 1024), nch * KSTEPS * MTall * 64 < 1 << 31)


def wfrag_bytes(Ci, Co, ks, ext):
    """cfd_conv2d_wfrag_bytes"""
    if Ci < 1 or Co < 1 or Ci > 192 or Co > 192:
        return 0
    F = conv6_frag(Ci, Co, ks, ext)
    return F.bytes if F.ok else 0


Plan6 = namedtuple("Plan6", "ok key TW TH NB tiles_x tiles_y ptiles CC KSTEPS MTall nch mtw mgroups ksplit per gx NI plane lds wfrag_bytes split_bytes")


def conv6_plan(B, Ci, Co, H, W, ks, ext, grid):
    """conv6_plan; key = (KS, CC, EXT, MT, NI) of the k_conv6 instantiation conv6_launch picks (None: not covered).  `per` = channel
    chunks of a split-K slice (the last slice has nch - (ksplit - 1) per of them)."""
    if ks not in (3, 5, 7):
        return Plan6(False, None, *([0] * 20))
    PAD = ks // 2
    Hd, Wd = (H + 2 * PAD, W + 2 * PAD) if ext else (H, W)
    Cm, Cs = (Ci, Co) if ext else (Co, Ci)
    F = conv6_frag(Ci, Co, ks, ext)
    TW, TH, NB = tile_shape(Hd, Wd, B)

    def slots_of(nb):
        npx = nb * (TH + ks - 1) * (TW + ks - 1)
        return npx if F.CC == 8 else ((npx + 63) & ~63) + npx

    while NB > 1 and slots_of(NB) > 5 * 256:
        NB -= 1
    tiles_x, tiles_y = cdiv(Wd, TW), cdiv(Hd, TH)
    LH, LW = TH + ks - 1, TW + ks - 1
    ptiles = cdiv(B, NB) * tiles_x * tiles_y

    def lds_of(mtw):
        return 3 * NB * LH * LW * F.CC * 2 + F.KSTEPS * mtw * 3 * 1024 + F.KSTEPS * 16

    plane = slots_of(NB)
    NI = 3 if plane <= 3 * 256 else 5
    mtw = 2 if F.MTall >= 2 else 1
    if mtw == 2 and (lds_of(2) > MAX_LDS or ptiles * ((F.MTall + 1) // 2) < MT2_MIN_WGS):
        mtw = 1
    mgroups = cdiv(F.MTall, mtw)
    wgs = ptiles * mgroups
    ksplit, per = 1, F.nch
    gx = grid // mgroups
    if wgs < 256 and F.nch > 1:
        best = -1
        for k in range(1, min(F.nch, 16) + 1):
            p = cdiv(F.nch, k)
            if cdiv(F.nch, p) != k:
                continue
            g1 = min(max(grid // (mgroups * k), 1), ptiles)
            trips = cdiv(ptiles, g1) * p
            if best < 0 or trips < best:
                best, ksplit, per, gx = trips, k, p, g1
    gx = min(max(gx, 1), ptiles)
    lds = lds_of(mtw)
    split = align_up(ksplit * B * Cm * Hd * Wd * 4) if ksplit > 1 else 0
    small = B * Cs * H * W <= 1 << 29 and B * Cm * Hd * Wd <= 1 << 29
    ok = small and lds <= 150 * 1024 and plane <= 5 * 256 and F.ok and ptiles < 1 << 30
    key = (ks, F.CC, int(ext), mtw, NI) if ok else None
    return Plan6(ok, key, TW, TH, NB, tiles_x, tiles_y, ptiles, F.CC, F.KSTEPS, F.MTall, F.nch, mtw, mgroups, ksplit, per, gx, NI, plane,
                 lds, F.bytes, split)


def conv6_ws_bytes(B, Ci, Co, H, W, ks, ext, grid):
    P = conv6_plan(B, Ci, Co, H, W, ks, ext, grid)
    return P.wfrag_bytes + P.split_bytes if P.ok else 0


def stats_key(P):
    """The k_conv6<3, MT, CC, false, 3, true> form a forward plan runs when it emits statistics (None: it cannot)."""
    return ("stats", P.CC, P.mtw) if P.ok and P.key[0] == 3 and not P.key[2] and P.ksplit == 1 and P.NI == 3 else None


def stats_slots(B, Ci, Co, H, W, ks, grid):
    """cfd_conv2d_fwd_stats_slots"""
    if B <= 0:
        return 0
    P = conv6_plan(B, Ci, Co, H, W, ks, False, grid)
    return P.gx if stats_key(P) else 0


def gin_direct(B, Ci, Co, H, W, ks, grid):
    """conv6_run: the input-gradient kernel writes the interior of gin itself and k_fold_border folds the rim (False: k_fold_pad
    folds every pixel of the extended grid)."""
    P = conv6_plan(B, Ci, Co, H, W, ks, True, grid)
    return P.ok and P.ksplit == 1 and H >= 3 and W >= 3


Wg6 = namedtuple("Wg6", "ok key TW TH tiles_x tiles_y HP ntiles groups chunks mtw mgroups nkg lds part_bytes")


def wg6_plan(B, Ci, Co, H, W, ks, grid, mul=1):
    """wg6_plan; key = (KS, MT, NKY) of k_conv6_wgrad."""
    if ks not in (3, 5, 7):
        return Wg6(False, None, *([0] * 13))
    NKY = 3 if ks == 3 else 2
    TW = 8 if (W >= 8 or ks >= 5) else 4
    TH = 16 // TW
    tiles_x, tiles_y = cdiv(W, TW), cdiv(H, TH)
    LW, LH = TW + ks - 1, TH + NKY - 1
    HP = LH * LW
    ntiles = cdiv(B, 8) * tiles_x * tiles_y
    chunks = cdiv(Ci, 16)
    MTall = cdiv(Co, 16)
    mtw = 2 if MTall >= 2 else 1
    mgroups = cdiv(MTall, mtw)
    nkg = cdiv(ks, NKY)
    want = max((mul if mul > 0 else 1) * grid // (chunks * mgroups * nkg), 1)
    cap = (32 << 20) // (Co * Ci * ks * ks * 4 + 1)
    want = max(min(want, cap), 1)
    groups = min(want, ntiles)
    stage = 3 * HP * 256 + 3 * 16 * mtw * 256
    red = 4 * (9 if ks == 3 else ks) * 256 * 4
    lds = max(stage, red)
    part = align_up(groups * (Co * Ci * ks * ks + Co) * 4)
    ok = lds <= 150 * 1024 and HP * 16 <= 3 * 256 and B * Ci * H * W < 1 << 30 and B * Co * H * W < 1 << 30
    return Wg6(ok, (ks, mtw, NKY) if ok else None, TW, TH, tiles_x, tiles_y, HP, ntiles, groups, chunks, mtw, mgroups, nkg, lds, part)


def zeropad_covers(B, Ci, Co, H, W, ks, grid):
    """cfd_conv2d_zeropad_supported"""
    if B < 1:
        return False
    Pe = conv6_plan(B, Ci, Co, H, W, ks, True, grid)
    return bool(conv6_plan(B, Ci, Co, H, W, ks, False, grid).ok and Pe.ok and Pe.ksplit == 1 and H >= 3 and W >= 3
                and wg6_plan(B, Ci, Co, H, W, ks, grid).ok)


def wgrad_plan(total_px, R, J):
    """wgrad_plan (conv.hip): (chunk_px, nchunk) of the exact-fp32 k_conv_wgrad."""
    tiles = cdiv(R, 32) * cdiv(J, 64)
    want = cdiv(2048, tiles)
    cap = (32 << 20) // (R * J * 4 + 1)
    want = max(min(want, cap), 1)
    chunk = max(cdiv(total_px, want), 64)
    chunk = cdiv(chunk, 16) * 16
    return chunk, cdiv(total_px, chunk)


def chan_sum_ws_bytes(C):
    return align_up((C * BN_SPLIT * 2 + C) * 4)


def part_reduce_G(nchunk):
    """cfd_conv_part_reduce_job: thread groups per element of the partial-slice reduction."""
    return 16 if nchunk >= 128 else (4 if nchunk >= 24 else 1)


StreamWg = namedtuple("StreamWg", "ok key ksteps per groups mgroups ngroups bytes")


def _stream_wg_plan(B, px_img, rows, cols, n_out, small, name):
    if B < 1 or not small:
        return StreamWg(False, None, 0, 0, 0, 0, 0, 0)
    ksteps = cdiv(B * px_img, 32)
    mgroups = (cdiv(rows, 16) + 2) // 3
    ngroups = (cdiv(cols, 16) + 2) // 3
    want = max(1024 // (mgroups * ngroups), 1)
    want = min(want, cdiv(ksteps, 8))
    cap = (16 << 20) // (n_out * 4 + 1)
    want = max(min(want, cap), 1)
    per = cdiv(ksteps, want)
    groups = cdiv(ksteps, per)
    return StreamWg(True, name, ksteps, per, groups, mgroups, ngroups, align_up(groups * n_out * 4))


def convt6_small(B, Ci, Co, H, W):
    return B * Ci * H * W < 1 << 31 and B * Co * 4 * H * W < 1 << 31


def convt6_wg_plan(B, Ci, Co, H, W):
    """convt6_wg_plan at a dense gradient (key "k_convt6_wgrad"; not ok: the fp32 k_conv_wgrad<true> serves)."""
    fits = W % 4 == 0 and (H * W) % 8 == 0 and convt6_small(B, Ci, Co, H, W)
    return _stream_wg_plan(B, H * W, Ci, 4 * Co, Ci * 4 * Co + Co, fits, "k_convt6_wgrad")


def conv1_small(B, Ci, Co, HW):
    return B * Ci * HW < 1 << 31 and B * Co * HW < 1 << 31


def conv1_wg_plan(B, Ci, Co, HW):
    """conv1_wg_plan (key "k_conv1_wgrad"; not ok: the fp32 k_conv_wgrad<false> serves)."""
    return _stream_wg_plan(B, HW, Co, Ci, Co * Ci + Co, HW % 8 == 0 and conv1_small(B, Ci, Co, HW), "k_conv1_wgrad")


def _stream_form(total, M, nt4_min_wgs):
    mgroups = (cdiv(M, 16) + 2) // 3
    return "NT4" if cdiv(total, 256) * mgroups >= nt4_min_wgs else "KSPL"


def convt6_form(B, Ci, Co, H, W, bwd, nt4_min_wgs=NT4_MIN_WGS):
    """convt6_launch: ("k_convt6", BWD, "NT4" | "KSPL") -- four pixel tiles per wave, or one tile with the K steps dealt to the waves."""
    return ("k_convt6", int(bwd), _stream_form(B * H * W, Ci if bwd else 4 * Co, nt4_min_wgs))


def conv1_form(B, Ci, Co, HW, dgrad, nt4_min_wgs=NT4_MIN_WGS):
    """conv1_launch: ("k_conv1", DG, "NT4" | "KSPL")."""
    return ("k_conv1", int(dgrad), _stream_form(B * HW, Ci if dgrad else Co, nt4_min_wgs))


# ---- the workspace entries of the C ABI (conv.hip) ----
def fwd_workspace_bytes(B, Ci, Co, H, W, ks, grid):
    """cfd_conv2d_fwd_workspace_bytes"""
    if B <= 0:
        return 0
    return conv6_ws_bytes(B, Ci, Co, H, W, ks, False, grid)


def bwd_workspace_bytes(B, Ci, Co, H, W, ks, grid):
    """cfd_conv2d_bwd_workspace_bytes"""
    if B <= 0:
        return 0
    pad = ks // 2
    ext = align_up(B * Ci * (H + 2 * pad) * (W + 2 * pad) * 4)
    _, nchunk = wgrad_plan(B * H * W, Co, Ci * ks * ks)
    part = align_up(nchunk * Co * Ci * ks * ks * 4)
    wg = wg6_plan(B, Ci, Co, H, W, ks, grid)
    if wg.ok:
        part = wg.part_bytes
    if ks == 1:
        part = max(part, conv1_wg_plan(B, Ci, Co, H * W).bytes)
    Pe = conv6_plan(B, Ci, Co, H, W, ks, True, grid)
    dg = ext + (Pe.wfrag_bytes + Pe.split_bytes if Pe.ok else 0)
    m = dg + part if (Pe.ok and wg.ok) else max(dg, part)
    return max(m, chan_sum_ws_bytes(Co))


def convt2_bwd_workspace_bytes(B, Ci, Co, H, W):
    """cfd_convt2_bwd_workspace_bytes"""
    if B <= 0:
        return 0
    _, nchunk = wgrad_plan(B * H * W, Ci, Co * 4)
    a = align_up(nchunk * Ci * Co * 4 * 4)
    return max(a, convt6_wg_plan(B, Ci, Co, H, W).bytes, chan_sum_ws_bytes(Co))


def conv6_keys(B, Ci, Co, H, W, ks, grid):
    """Every conv6.hip instantiation cfd_conv2d_fwd + cfd_conv2d_bwd run on a shape: the k_conv6 keys of both directions and the
    k_conv6_wgrad key (as ("wgrad", KS, MT, NKY))."""
    keys = set()
    for ext in (False, True):
        P = conv6_plan(B, Ci, Co, H, W, ks, ext, grid)
        if P.ok:
            keys.add(P.key)
    wg = wg6_plan(B, Ci, Co, H, W, ks, grid)
    if wg.ok:
        keys.add(("wgrad",) + wg.key)
    return keys


ALL_CONV6_KEYS = [(ks, cc, ext, mt, ni) for ks, cc in ((3, 8), (3, 16), (5, 8), (7, 8)) for ext in (0, 1) for mt in (1, 2) for ni in (3, 5)]
ALL_STATS_KEYS = [("stats", cc, mt) for cc in (8, 16) for mt in (1, 2)]
ALL_WGRAD_KEYS = [("wgrad", ks, mt, 3 if ks == 3 else 2) for ks in (3, 5, 7) for mt in (1, 2)]


# ---- the seeded sweep over the accepted range that tests/test_cpu_conv_plan.py pins the mirror on ----
GRIDS = (-1, 2, 512)  # conv6_grid: the build default, the emulator build's value, the product's value


def sweep(n=3200, seed=20261020):
    """(B, Ci, Co, H, W, ks, conv6_grid): half of the draws uniform over the range, the others from the values where a planner changes
    its mind (tile widths, channel chunks of 8 / 16, output-channel tiles of 16 / 32, images smaller than a kernel), one in eight a
    thin image in a large batch."""
    rnd = random.Random(seed)
    edge_c = [1, 2, 7, 8, 9, 15, 16, 17, 24, 31, 32, 33, 47, 48, 49, 64, 65, 96, 128, 129, 160, 191, 192]
    edge_p = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16, 17, 20, 31, 32, 33, 40, 62, 63, 64, 65, 66, 96, 127, 128]
    edge_b = [1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65, 128, 129, 130]
    out = []
    thin = [1, 2, 3, 4, 5, 6, 7]
    for i in range(n):
        if i % 2:
            s = (rnd.randint(1, 130), rnd.randint(1, 192), rnd.randint(1, 192), rnd.randint(1, 128), rnd.randint(1, 128))
        elif i % 8 == 0:  # thin images in large batches: the only shapes whose halo exceeds three times the tile (NI = 5 under MT = 2)
            hw = (rnd.choice(thin), rnd.randint(1, 128))
            s = (rnd.randint(100, 130), rnd.choice(edge_c), rnd.choice(edge_c), *(hw if rnd.random() < 0.5 else hw[::-1]))
        else:
            s = (rnd.choice(edge_b), rnd.choice(edge_c), rnd.choice(edge_c), rnd.choice(edge_p), rnd.choice(edge_p))
        out.append((*s, rnd.choice([3, 5, 7]), GRIDS[i % 3]))
    # k = 5 runs two output-channel tiles on five halo items only in a window of 769 .. 808 halo slots, which thirteen image sizes in
    # large batches reach: too few for a random draw, so three of them are named
    for s in ((130, 1, 33, 2, 40, 5), (130, 8, 192, 3, 10, 5), (120, 5, 40, 4, 7, 5)):
        out += [(*s, g) for g in GRIDS]
    return out


SWEEP = sweep()
