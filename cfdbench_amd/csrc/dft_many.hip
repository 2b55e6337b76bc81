// Many-modes route of the truncated real DFT pair (plans with m1 > 15 or m2 > 16 or W > 80, up to 2 m1 <= H and m2 <= W/2 + 1 on grids
// up to 128 x 128; plan.cpp: cfd_plan_create_many).  The narrow kernels of spectral.hip deal the kept modes to 16 lane slots; here each image
// is two real GEMM stages on the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32: fp32 products, accumulation in fixed k order), no atomics:
//   forward  xh = rfft2(x)[K, :m2]:  P = X (H x W) . T1 (W x [cos | -sin] of 2 m2),  then  xh = (T2C - i T2S) (2 m1 x H) . P
//   inverse  out = irfft2 of the kept modes:  U = (TAC + i TAS) (H x 2 m1) . z,  then  out = [Re U | Im U] (H x 2 m2) . TB (2 m2 x W)
// 256-thread workgroups, persistent over work items, four waves dealing the 16 x 16 output tiles of a stage between them.  LDS is bounded
// (CFD_MANY_LDS_CAP) by what a work item is:
//   forward  (image, group of 16-column tiles of l): the image streams through LDS in bands of RB rows (stage W is independent per row), the
//            group's columns of T1 and of P stay in LDS (stage H needs P whole, but only the group's columns of it);
//   inverse  (image, band of RB rows): both stages are independent per output row; z, the band of U and -- where it fits -- TB stay in LDS.
// With one group / one band of all rows this is the whole-image form (an image, both tables of the W stage and the stage result in LDS).
// The table of the H stage (up to 128 KB at H = 128) is read from global memory, where it stays cache-resident; so is TB where z and TB do
// not fit together (full modes above about 106 x 106).  Every output element is one accumulator chain over k ascending in steps of 4
// whatever the split, so the split changes no result bit.
#include "cfd_common.h"
#include "cfd_launch.h"

#define CFD_MANY_LDS_CAP 163840    // dynamic LDS a workgroup may ask for: the 160 KB of a CU
#define CFD_MANY_LDS_HALF 81920    // two workgroups per CU
#define CFD_MANY_BLOCKS 512        // persistent grid: two workgroups per CU at most

// LDS pitches: an A-operand plane (16 rows x 4 k of one MFMA) reads conflict-free when pitch / 4 is odd, a B-operand plane (4 k-rows x 16
// columns) when pitch / 16 is odd
__host__ __device__ static inline int many_pitch_a(int n) { return (n / 4) % 2 ? n : n + 4; }     // n: a multiple of 4
__host__ __device__ static inline int many_pitch_b(int n) { return (n / 16) % 2 ? n : n + 16; }   // n: a multiple of 16

// How a launch is cut into work items (host; the kernels take the numbers as arguments).
struct ManyFwdCfg {
    int RB;    // rows of the image band in LDS: a multiple of 16, <= Hp
    int G;     // groups of l tiles; G == 1 keeps T1's own column layout ([Re | Im] at offset m2, N1p columns)
    int nlg;   // 16-column tiles of l per group
    int ioff;  // LDS column of Im l0 (Re l0 is column 0): m2 with one group, 16 nlg otherwise
    int nc;    // LDS columns of T1 / P: N1p with one group, 32 nlg otherwise
    size_t lds;
};
struct ManyInvCfg {
    int RB;    // rows of U per work item: a multiple of 16, <= Hp
    int tbl;   // TB in LDS (1) or read from global memory (0)
    size_t lds;
};

static size_t many_fwd_lds(const CfdManyDims& d, int RB, int nc) {
    const int LX = many_pitch_a(d.Wk), LT = many_pitch_b(nc);
    return ((size_t)RB * LX + (size_t)d.Wk * LT + (size_t)d.Hp * LT) * sizeof(float);
}
static size_t many_inv_lds(const CfdManyDims& d, int m2, int RB, int tbl) {
    const int LZ = many_pitch_b((m2 + 15) / 16 * 16), LU = many_pitch_a(d.K2), LB = many_pitch_b(d.Wq);
    return (2 * (size_t)d.R4 * LZ + (size_t)RB * LU + (tbl ? (size_t)d.K2 * LB : 0)) * sizeof(float);
}
static int many_largest_band(size_t fixed, size_t per_row, int Hp, size_t budget) {  // 0: not even 16 rows fit
    if (fixed + 16 * per_row > budget) return 0;
    const int rb = (int)((budget - fixed) / per_row) / 16 * 16;
    return rb < Hp ? rb : Hp;
}

// nimg <= 0: the launch-independent choice (the largest LDS a launch of this plan asks for).  A launch with few images takes more, smaller
// items (more groups / shorter bands) until there are CFD_MANY_BLOCKS of them; that only lowers the LDS.
static ManyFwdCfg many_fwd_cfg(int H, int W, int m1, int m2, int nimg) {
    const CfdManyDims d = cfd_many_dims(H, W, m1, m2);
    const int nl = (m2 + 15) / 16;
    auto with_groups = [&](int G, size_t budget) {
        ManyFwdCfg c;
        c.G = G;
        c.nlg = (nl + G - 1) / G;
        c.G = (nl + c.nlg - 1) / c.nlg;
        c.ioff = c.G == 1 ? m2 : 16 * c.nlg;
        c.nc = c.G == 1 ? d.N1p : 32 * c.nlg;
        const size_t fixed = many_fwd_lds(d, 0, c.nc), per_row = (size_t)many_pitch_a(d.Wk) * sizeof(float);
        c.RB = many_largest_band(fixed, per_row, d.Hp, budget);
        c.lds = many_fwd_lds(d, c.RB, c.nc);
        return c;
    };
    ManyFwdCfg c = with_groups(1, CFD_MANY_LDS_CAP);
    if (W > 80) {
        // two workgroups per CU: shorter bands first (the image is still read once), then groups (each group reads the image)
        int G = 1;
        c = with_groups(G, CFD_MANY_LDS_HALF);
        while (c.RB == 0 && G < nl) c = with_groups(++G, CFD_MANY_LDS_HALF);
    }
    // (W <= 80: the whole-image form of every plan of that range fits the cap and is kept as measured)
    if (nimg > 0) {
        const size_t budget = c.lds;
        int G = c.G;
        while ((long)nimg * c.G < CFD_MANY_BLOCKS / 2 && G < nl) {
            const ManyFwdCfg n = with_groups(++G, budget);
            if (n.RB == 0) break;
            c = n;
        }
    }
    return c;
}
static ManyInvCfg many_inv_cfg(int H, int W, int m1, int m2, int nimg) {
    const CfdManyDims d = cfd_many_dims(H, W, m1, m2);
    const size_t per_row = (size_t)many_pitch_a(d.K2) * sizeof(float);
    ManyInvCfg c;
    c.tbl = 1;
    c.RB = many_largest_band(many_inv_lds(d, m2, 0, 1), per_row, d.Hp, W > 80 ? CFD_MANY_LDS_HALF : CFD_MANY_LDS_CAP);
    if (c.RB == 0) c.RB = many_largest_band(many_inv_lds(d, m2, 0, 1), per_row, d.Hp, CFD_MANY_LDS_CAP);
    if (c.RB == 0) {  // z and TB do not fit together: TB from global memory
        c.tbl = 0;
        c.RB = many_largest_band(many_inv_lds(d, m2, 0, 0), per_row, d.Hp, CFD_MANY_LDS_CAP);
    }
    if (nimg > 0 && c.RB > 0) {
        const int tiles = d.Hp / 16, want = (CFD_MANY_BLOCKS + nimg - 1) / nimg;  // bands per image that fill the grid
        const int bands = want < tiles ? want : tiles;
        const int rb = (tiles + bands - 1) / bands * 16;
        if (rb < c.RB) c.RB = rb;
    }
    c.lds = many_inv_lds(d, m2, c.RB, c.tbl);
    return c;
}

// the one LDS figure of a plan and direction: what the launchers ask for at most (cfd_spectral_transform_lds_bytes)
static size_t many_lds_bytes(int H, int W, int m1, int m2, int inverse) {
    if (inverse) {
        const ManyInvCfg c = many_inv_cfg(H, W, m1, m2, 0);
        return c.RB ? c.lds : (size_t)CFD_MANY_LDS_CAP + 1;
    }
    const ManyFwdCfg c = many_fwd_cfg(H, W, m1, m2, 0);
    return c.RB ? c.lds : (size_t)CFD_MANY_LDS_CAP + 1;
}

extern "C" int cfd_spectral_transform_lds_bytes(int H, int W, int m1, int m2, int inverse) {
    if (H < 2 || H > 128 || W < 2 || W > 128 || m1 < 1 || 2 * m1 > H || m2 < 1 || m2 > W / 2 + 1) return 0;
    if (!(m1 > 15 || m2 > 16 || W > 80)) return 0;  // a narrow plan (plan.cpp: cfd_plan_create)
    return (int)many_lds_bytes(H, W, m1, m2, inverse);
}

// xh[img][r][l] (complex) = sum_{x,y} f(x[img][x][y]) e^{-2 pi i (K[r] x / H + l y / W)}, f = GELU with ACT.  Work item it = g * nimg + img
// (group-major, so that a workgroup's contiguous share of the items restages T1 at most G times).
template <bool ACT>
__global__ __launch_bounds__(256) void k_dft_many(const float* __restrict__ x, float2* __restrict__ xh, const float* __restrict__ tab,
                                                  int nimg, int H, int W, int m1, int m2, int RB, int G, int nlg, int ioff, int nc) {
    CFD_DYN_SHARED(float, smem);
    const CfdManyDims d = cfd_many_dims(H, W, m1, m2);
    const int LX = many_pitch_a(d.Wk), LT = many_pitch_b(nc);
    float* xs = smem;               // [RB][LX]  a band of the image, zero outside H x W
    float* t1 = xs + RB * LX;       // [Wk][LT]  the group's columns of T1: Re l0 + j at column j, Im l0 + j at column ioff + j
    float* ps = t1 + d.Wk * LT;     // [Hp][LT]  P = sum_y f(x) e^{-2 pi i l y / W}, same columns
    const float* t2c = tab + d.Wk * d.N1p;
    const float* t2s = t2c + d.R2p * d.Hk;
    const int tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nw = nthr >> 6;
    const int i16 = tid & 15, k4 = (tid >> 4) & 3;
    const int M = 2 * m1 * m2;
    const int nc1 = nc / 16, nrt = d.R2p / 16;
    const long nitems = (long)nimg * G;
    const int it0 = (int)(nitems * blockIdx.x / gridDim.x), it1 = (int)(nitems * (blockIdx.x + 1) / gridDim.x);
    int gcur = -1;
    for (int it = it0; it < it1; ++it) {
        const int g = it / nimg, img = it - g * nimg;
        const int l0g = g * nlg * 16;  // first l of the group
        __syncthreads();  // the previous item's readers of t1 and ps are done
        if (g != gcur) {
            gcur = g;
            for (int i = tid; i < d.Wk * nc; i += nthr) {
                const int y = i / nc, c = i - y * nc;
                const bool imag = c >= ioff;
                const int l = l0g + (imag ? c - ioff : c);
                t1[y * LT + c] = l < m2 ? tab[y * d.N1p + (imag ? m2 + l : l)] : 0.f;
            }
        }
        const float* src = x + (size_t)img * H * W;
        for (int xb = 0; xb < d.Hp; xb += RB) {
            const int rows = d.Hp - xb < RB ? d.Hp - xb : RB;
            if (xb) __syncthreads();  // the previous band's readers of xs are done
            for (int i = tid; i < rows * d.Wk; i += nthr) {
                const int r = i / d.Wk, c = i - r * d.Wk;
                float v = 0.f;
                if (xb + r < H && c < W) {
                    v = src[(xb + r) * W + c];
                    if (ACT) v = cfd_gelu(v);
                }
                xs[r * LX + c] = v;
            }
            __syncthreads();
            // stage W: ps[x][c] = sum_y xs[x][y] t1[y][c]
            const int nt1 = (rows / 16) * nc1;
            for (int t = wave; t < nt1; t += nw) {
                const int x0 = (t / nc1) * 16, c0 = (t % nc1) * 16;
                const float* a = xs + (x0 + i16) * LX + k4;
                const float* b = t1 + k4 * LT + c0 + i16;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int y = 0; y < d.Wk; y += 4) acc = cfd_mfma16x16x4(a[y], b[y * LT], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) ps[(xb + x0 + 4 * k4 + r) * LT + c0 + i16] = acc[r];
            }
        }
        __syncthreads();
        // stage H: xh[r][l] = sum_x (T2C[r][x] - i T2S[r][x]) (P[x][l] + i P[x][m2 + l]).  Columns l >= m2 of a tile read column m2 - 1
        // (their results are not stored; an MFMA column depends on its own B column only).
        const int lend = l0g + nlg * 16 < m2 ? l0g + nlg * 16 : m2;  // one past the group's last l
        const int nlt = (lend - l0g + 15) / 16, nt2 = nrt * nlt;
        for (int t = wave; t < nt2; t += nw) {
            const int r0 = (t / nlt) * 16, l0 = l0g + (t % nlt) * 16;
            const int l = l0 + i16 < m2 ? l0 + i16 : m2 - 1;
            const float* ac = t2c + (r0 + i16) * d.Hk + k4;
            const float* as = t2s + (r0 + i16) * d.Hk + k4;
            const float* br = ps + k4 * LT + (l - l0g);
            const float* bi = br + ioff;
            f32x4 re = {0.f, 0.f, 0.f, 0.f}, im = {0.f, 0.f, 0.f, 0.f};
            for (int xx = 0; xx < d.Hk; xx += 4) {
                const float c = ac[xx], s = as[xx], pr = br[xx * LT], pi = bi[xx * LT];
                re = cfd_mfma16x16x4(c, pr, re);
                re = cfd_mfma16x16x4(s, pi, re);
                im = cfd_mfma16x16x4(c, pi, im);
                im = cfd_mfma16x16x4(-s, pr, im);
            }
            float2* o = xh + (size_t)img * M;
            const int col = l0 + i16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 4 * k4 + r;
                if (row < 2 * m1 && col < m2) o[row * m2 + col] = make_float2(re[r], im[r]);
            }
        }
    }
}

// out[img][x][y] = epi( (1/HW) sum_{r,l} c_l Re(z[img][r][l] e^{+2 pi i (K[r] x / H + l y / W)}) ):  EPI 0 plain, 1 + addend,
// 2 (+ addend) * gelu'(aprev).  addend may alias out (each pixel is read and written by the same lane).  Work item it = img * nb + band
// (a workgroup's contiguous share of the items stages z once per image); TBL: TB in LDS, else read from the plan's table.
template <int EPI, bool TBL>
__global__ __launch_bounds__(256) void k_idft_many(const float2* __restrict__ z, const float* addend, const float* __restrict__ aprev,
                                                   float* out, const float* __restrict__ tab, int nimg, int H, int W, int m1, int m2, int RB) {
    CFD_DYN_SHARED(float, smem);
    const CfdManyDims d = cfd_many_dims(H, W, m1, m2);
    const int LZ = many_pitch_b((m2 + 15) / 16 * 16), LU = many_pitch_a(d.K2), LB = TBL ? many_pitch_b(d.Wq) : d.Wq;
    float* zr = smem;               // [R4][LZ]  Re z, zero in rows >= 2 m1
    float* zi = zr + d.R4 * LZ;     // [R4][LZ]  Im z
    float* us = zi + d.R4 * LZ;     // [RB][LU]  the band's rows of [Re U | Im U], zero in columns >= 2 m2
    float* tbs = us + RB * LU;      // [K2][LB]  TB (TBL)
    const float* tb = TBL ? tbs : tab;
    const float* tac = tab + d.K2 * d.Wq;
    const float* tas = tac + d.Hp * d.R4;
    const int tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nw = nthr >> 6;
    const int i16 = tid & 15, k4 = (tid >> 4) & 3;
    for (int i = tid; i < 2 * d.R4 * LZ + RB * LU; i += nthr) zr[i] = 0.f;
    if (TBL)
        for (int i = tid; i < d.K2 * d.Wq; i += nthr) tbs[(i / d.Wq) * LB + i % d.Wq] = tab[i];
    const int HW = H * W, M = 2 * m1 * m2;
    const int nl = (m2 + 15) / 16, ny = d.Wq / 16;
    const int nb = (d.Hp + RB - 1) / RB;
    const long nitems = (long)nimg * nb;
    const int it0 = (int)(nitems * blockIdx.x / gridDim.x), it1 = (int)(nitems * (blockIdx.x + 1) / gridDim.x);
    int icur = -1;
    for (int it = it0; it < it1; ++it) {
        const int img = it / nb, xb = (it - img * nb) * RB;
        const int rows = d.Hp - xb < RB ? d.Hp - xb : RB;
        __syncthreads();  // the zero fill and TB are staged / the previous item's readers of z and us are done
        if (img != icur) {
            icur = img;
            const float2* zsrc = z + (size_t)img * M;
            for (int i = tid; i < M; i += nthr) {
                const int r = i / m2, l = i - r * m2;
                const float2 v = zsrc[i];
                zr[r * LZ + l] = v.x;
                zi[r * LZ + l] = v.y;
            }
            __syncthreads();
        }
        // stage H: U[x][l] = sum_r (TAC[x][r] + i TAS[x][r]) z[r][l]
        const int ntA = (rows / 16) * nl;
        for (int t = wave; t < ntA; t += nw) {
            const int x0 = (t / nl) * 16, l0 = (t % nl) * 16;
            const int l = l0 + i16 < m2 ? l0 + i16 : m2 - 1;
            const float* ac = tac + (xb + x0 + i16) * d.R4 + k4;
            const float* as = tas + (xb + x0 + i16) * d.R4 + k4;
            const float* bzr = zr + k4 * LZ + l;
            const float* bzi = zi + k4 * LZ + l;
            f32x4 ur = {0.f, 0.f, 0.f, 0.f}, ui = {0.f, 0.f, 0.f, 0.f};
            for (int r = 0; r < d.R4; r += 4) {
                const float c = ac[r], s = as[r], a = bzr[r * LZ], b = bzi[r * LZ];
                ur = cfd_mfma16x16x4(c, a, ur);
                ur = cfd_mfma16x16x4(-s, b, ur);
                ui = cfd_mfma16x16x4(c, b, ui);
                ui = cfd_mfma16x16x4(s, a, ui);
            }
            const int col = l0 + i16;
            if (col < m2) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    us[(x0 + 4 * k4 + r) * LU + col] = ur[r];
                    us[(x0 + 4 * k4 + r) * LU + m2 + col] = ui[r];
                }
            }
        }
        __syncthreads();
        // stage W: out[x][y] = sum_c us[x][c] TB[c][y]
        const int ntB = (rows / 16) * ny;
        for (int t = wave; t < ntB; t += nw) {
            const int x0 = (t / ny) * 16, y0 = (t % ny) * 16;
            const float* a = us + (x0 + i16) * LU + k4;
            const float* b = tb + k4 * LB + y0 + i16;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < d.K2; c += 4) acc = cfd_mfma16x16x4(a[c], b[c * LB], acc);
            const int y = y0 + i16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int xr = xb + x0 + 4 * k4 + r;
                if (xr < H && y < W) {
                    const size_t idx = (size_t)img * HW + xr * W + y;
                    float v = acc[r];
                    if (EPI >= 1) v += addend[idx];
                    if (EPI == 2) v *= cfd_gelu_grad(aprev[idx]);
                    out[idx] = v;
                }
            }
        }
    }
}

static int many_blocks(long items) { return items < CFD_MANY_BLOCKS ? (int)items : CFD_MANY_BLOCKS; }

int cfd_int_dft_many(const cfd_plan* p, const float* x, float* xh, int nimg, int act_in, void* stream) {
    CFD_REQUIRE(p && p->many && p->d_many_fwd, CFD_ERR_INVALID_ARG, "cfd_spectral_dft: not a many-modes plan");
    if (nimg == 0) return CFD_OK;
    hipStream_t st = (hipStream_t)stream;
    const ManyFwdCfg c = many_fwd_cfg(p->H, p->W, p->m1, p->m2, nimg);
    CFD_REQUIRE(c.RB > 0 && c.lds <= many_lds_bytes(p->H, p->W, p->m1, p->m2, 0) && c.lds <= CFD_MANY_LDS_CAP, CFD_ERR_UNSUPPORTED,
                "cfd_spectral_dft: plan %dx%d modes (%d, %d) needs more than %d bytes of LDS", p->H, p->W, p->m1, p->m2, CFD_MANY_LDS_CAP);
    CFD_REQUIRE((long)nimg * c.G <= 0x7fffffffL, CFD_ERR_UNSUPPORTED, "cfd_spectral_dft: %d images in %d groups exceed the index range", nimg, c.G);
    CFD_PROF_W(act_in ? "k_dft_many_act" : "k_dft_many", st, (double)nimg * (4.0 * p->H * p->W + 16.0 * p->m1 * p->m2),
               (double)nimg * (4.0 * p->H * p->W * p->m2 + 16.0 * p->H * p->m1 * p->m2));
    const int blocks = many_blocks((long)nimg * c.G);
    int rc = CFD_OK;
    with_bools([&](auto A) {
        rc = cfd_allow_lds<k_dft_many<CFD_B(A)>>(c.lds, "cfd_spectral_dft");
        if (rc != CFD_OK) return;
        hipLaunchKernelGGL(k_dft_many<CFD_B(A)>, dim3(blocks), dim3(256), c.lds, st, x, (float2*)xh, (const float*)p->d_many_fwd, nimg, p->H, p->W,
                           p->m1, p->m2, c.RB, c.G, c.nlg, c.ioff, c.nc);
    }, act_in != 0);
    CFD_TRY(rc);
    CFD_LAUNCH_CHECK("cfd_spectral_dft(many modes)");
    return CFD_OK;
}

int cfd_int_idft_many(const cfd_plan* p, const float* z, const float* addend, const float* aprev, float* out, int nimg, int epi, void* stream) {
    CFD_REQUIRE(p && p->many && p->d_many_inv, CFD_ERR_INVALID_ARG, "cfd_spectral_idft: not a many-modes plan");
    if (nimg == 0) return CFD_OK;
    hipStream_t st = (hipStream_t)stream;
    const ManyInvCfg c = many_inv_cfg(p->H, p->W, p->m1, p->m2, nimg);
    CFD_REQUIRE(c.RB > 0 && c.lds <= many_lds_bytes(p->H, p->W, p->m1, p->m2, 1) && c.lds <= CFD_MANY_LDS_CAP, CFD_ERR_UNSUPPORTED,
                "cfd_spectral_idft: plan %dx%d modes (%d, %d) needs more than %d bytes of LDS", p->H, p->W, p->m1, p->m2, CFD_MANY_LDS_CAP);
    const CfdManyDims d = cfd_many_dims(p->H, p->W, p->m1, p->m2);
    const long items = (long)nimg * ((d.Hp + c.RB - 1) / c.RB);
    CFD_REQUIRE(items <= 0x7fffffffL, CFD_ERR_UNSUPPORTED, "cfd_spectral_idft: %d images exceed the index range", nimg);
    CFD_PROF_W(epi == 0 ? "k_idft_many" : (epi == 1 ? "k_idft_many_add" : "k_idft_many_add_dgelu"), st,
               (double)nimg * (4.0 * p->H * p->W * (1 + epi) + 16.0 * p->m1 * p->m2),
               (double)nimg * (4.0 * p->H * p->W * p->m2 + 16.0 * p->H * p->m1 * p->m2));
    const float2* zz = (const float2*)z;
    const float* tab = (const float*)p->d_many_inv;
    const int blocks = many_blocks(items);
    int rc = CFD_OK;
    cfd_dispatch([&](auto E, auto T) {
        rc = cfd_allow_lds<k_idft_many<CFD_I(E), CFD_B(T)>>(c.lds, "cfd_spectral_idft");
        if (rc != CFD_OK) return;
        hipLaunchKernelGGL((k_idft_many<CFD_I(E), CFD_B(T)>), dim3(blocks), dim3(256), c.lds, st, zz, addend, aprev, out, tab, nimg, p->H, p->W,
                           p->m1, p->m2, c.RB);
    }, cfd_among<0, 1, 2>(epi), (bool)c.tbl);
    CFD_TRY(rc);
    CFD_LAUNCH_CHECK("cfd_spectral_idft(many modes)");
    return CFD_OK;
}
