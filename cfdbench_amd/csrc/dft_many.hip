// Many-modes route of the truncated real DFT pair (plans with m1 > 15 or m2 > 16, up to 2 m1 <= H and m2 <= W/2 + 1; plan.cpp:
// cfd_plan_create_many).  The narrow kernels of spectral.hip deal the kept modes to 16 lane slots; here each image is two real GEMM stages
// on the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32: fp32 products, accumulation in fixed k order), no atomics:
//   forward  xh = rfft2(x)[K, :m2]:  P = X (H x W) . T1 (W x [cos | -sin] of 2 m2),  then  xh = (T2C - i T2S) (2 m1 x H) . P
//   inverse  out = irfft2 of the kept modes:  U = (TAC + i TAS) (H x 2 m1) . z,  then  out = [Re U | Im U] (H x 2 m2) . TB (2 m2 x W)
// One 256-thread workgroup per image at a time (persistent: the workgroups stride over the images), four waves dealing the 16 x 16 output
// tiles of a stage between them.  The image, the stage result and the table of the W stage sit in LDS; the table of the H stage (up to
// 128 KB at H = 128) is read from global memory, where it stays cache-resident.
#include "cfd_common.h"

// LDS pitches: an A-operand plane (16 rows x 4 k of one MFMA) reads conflict-free when pitch / 4 is odd, a B-operand plane (4 k-rows x 16
// columns) when pitch / 16 is odd
static inline int many_pitch_a(int n) { return (n / 4) % 2 ? n : n + 4; }     // n: a multiple of 4
static inline int many_pitch_b(int n) { return (n / 16) % 2 ? n : n + 16; }   // n: a multiple of 16
__device__ __forceinline__ int many_pitch_a_d(int n) { return (n / 4) % 2 ? n : n + 4; }
__device__ __forceinline__ int many_pitch_b_d(int n) { return (n / 16) % 2 ? n : n + 16; }

static size_t many_fwd_lds_floats(const CfdManyDims& d) {
    const int LX = many_pitch_a(d.Wk), LT = many_pitch_b(d.N1p);
    return (size_t)d.Hp * LX + (size_t)d.Wk * LT + (size_t)d.Hp * LT;
}
static size_t many_inv_lds_floats(const CfdManyDims& d, int m2) {
    const int LZ = many_pitch_b((m2 + 15) / 16 * 16), LU = many_pitch_a(d.K2), LB = many_pitch_b(d.Wq);
    return 2 * (size_t)d.R4 * LZ + (size_t)d.Hp * LU + (size_t)d.K2 * LB;
}

// xh[img][r][l] (complex) = sum_{x,y} f(x[img][x][y]) e^{-2 pi i (K[r] x / H + l y / W)}, f = GELU with ACT
template <bool ACT>
__global__ __launch_bounds__(256) void k_dft_many(const float* __restrict__ x, float2* __restrict__ xh, const float* __restrict__ tab,
                                                  int nimg, int H, int W, int m1, int m2) {
    CFD_DYN_SHARED(float, smem);
    const CfdManyDims d = cfd_many_dims(H, W, m1, m2);
    const int LX = many_pitch_a_d(d.Wk), LT = many_pitch_b_d(d.N1p);
    float* xs = smem;               // [Hp][LX]  the image, zero outside H x W
    float* t1 = xs + d.Hp * LX;     // [Wk][LT]  T1
    float* ps = t1 + d.Wk * LT;     // [Hp][LT]  P = [Re | Im] of sum_y f(x) e^{-2 pi i l y / W}
    const float* t2c = tab + d.Wk * d.N1p;
    const float* t2s = t2c + d.R2p * d.Hk;
    const int tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nw = nthr >> 6;
    const int i16 = tid & 15, k4 = (tid >> 4) & 3;
    for (int i = tid; i < d.Hp * LX; i += nthr) xs[i] = 0.f;
    for (int i = tid; i < d.Wk * d.N1p; i += nthr) t1[(i / d.N1p) * LT + i % d.N1p] = tab[i];
    const int HW = H * W, M = 2 * m1 * m2;
    const int nc1 = d.N1p / 16, nt1 = (d.Hp / 16) * nc1;
    const int nl = (m2 + 15) / 16, nt2 = (d.R2p / 16) * nl;
    for (int img = blockIdx.x; img < nimg; img += gridDim.x) {
        __syncthreads();  // the tables are staged / the previous image's readers of xs and ps are done
        const float* src = x + (size_t)img * HW;
        for (int i = tid; i < HW; i += nthr) {
            const int r = i / W, c = i - r * W;
            const float v = src[i];
            xs[r * LX + c] = ACT ? cfd_gelu(v) : v;
        }
        __syncthreads();
        // stage W: ps[x][c] = sum_y xs[x][y] t1[y][c]
        for (int t = wave; t < nt1; t += nw) {
            const int x0 = (t / nc1) * 16, c0 = (t % nc1) * 16;
            const float* a = xs + (x0 + i16) * LX + k4;
            const float* b = t1 + k4 * LT + c0 + i16;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int y = 0; y < d.Wk; y += 4) acc = cfd_mfma16x16x4(a[y], b[y * LT], acc);
#pragma unroll
            for (int r = 0; r < 4; ++r) ps[(x0 + 4 * k4 + r) * LT + c0 + i16] = acc[r];
        }
        __syncthreads();
        // stage H: xh[r][l] = sum_x (T2C[r][x] - i T2S[r][x]) (ps[x][l] + i ps[x][m2 + l]).  Columns l >= m2 of a tile read column m2 - 1
        // (their results are not stored; an MFMA column depends on its own B column only).
        for (int t = wave; t < nt2; t += nw) {
            const int r0 = (t / nl) * 16, l0 = (t % nl) * 16;
            const int l = l0 + i16 < m2 ? l0 + i16 : m2 - 1;
            const float* ac = t2c + (r0 + i16) * d.Hk + k4;
            const float* as = t2s + (r0 + i16) * d.Hk + k4;
            const float* br = ps + k4 * LT + l;
            const float* bi = br + m2;
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
// 2 (+ addend) * gelu'(aprev).  addend may alias out (each pixel is read and written by the same lane).
template <int EPI>
__global__ __launch_bounds__(256) void k_idft_many(const float2* __restrict__ z, const float* addend, const float* __restrict__ aprev,
                                                   float* out, const float* __restrict__ tab, int nimg, int H, int W, int m1, int m2) {
    CFD_DYN_SHARED(float, smem);
    const CfdManyDims d = cfd_many_dims(H, W, m1, m2);
    const int LZ = many_pitch_b_d((m2 + 15) / 16 * 16), LU = many_pitch_a_d(d.K2), LB = many_pitch_b_d(d.Wq);
    float* zr = smem;               // [R4][LZ]  Re z, zero in rows >= 2 m1
    float* zi = zr + d.R4 * LZ;     // [R4][LZ]  Im z
    float* us = zi + d.R4 * LZ;     // [Hp][LU]  [Re U | Im U], zero in columns >= 2 m2
    float* tb = us + d.Hp * LU;     // [K2][LB]  TB
    const float* tac = tab + d.K2 * d.Wq;
    const float* tas = tac + d.Hp * d.R4;
    const int tid = threadIdx.x, nthr = blockDim.x, wave = tid >> 6, nw = nthr >> 6;
    const int i16 = tid & 15, k4 = (tid >> 4) & 3;
    for (int i = tid; i < 2 * d.R4 * LZ + d.Hp * LU; i += nthr) zr[i] = 0.f;
    for (int i = tid; i < d.K2 * d.Wq; i += nthr) tb[(i / d.Wq) * LB + i % d.Wq] = tab[i];
    const int HW = H * W, M = 2 * m1 * m2;
    const int nl = (m2 + 15) / 16, ntA = (d.Hp / 16) * nl;
    const int ny = d.Wq / 16, ntB = (d.Hp / 16) * ny;
    for (int img = blockIdx.x; img < nimg; img += gridDim.x) {
        __syncthreads();
        const float2* zsrc = z + (size_t)img * M;
        for (int i = tid; i < M; i += nthr) {
            const int r = i / m2, l = i - r * m2;
            const float2 v = zsrc[i];
            zr[r * LZ + l] = v.x;
            zi[r * LZ + l] = v.y;
        }
        __syncthreads();
        // stage H: U[x][l] = sum_r (TAC[x][r] + i TAS[x][r]) z[r][l]
        for (int t = wave; t < ntA; t += nw) {
            const int x0 = (t / nl) * 16, l0 = (t % nl) * 16;
            const int l = l0 + i16 < m2 ? l0 + i16 : m2 - 1;
            const float* ac = tac + (x0 + i16) * d.R4 + k4;
            const float* as = tas + (x0 + i16) * d.R4 + k4;
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
        for (int t = wave; t < ntB; t += nw) {
            const int x0 = (t / ny) * 16, y0 = (t % ny) * 16;
            const float* a = us + (x0 + i16) * LU + k4;
            const float* b = tb + k4 * LB + y0 + i16;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int c = 0; c < d.K2; c += 4) acc = cfd_mfma16x16x4(a[c], b[c * LB], acc);
            const int y = y0 + i16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int xr = x0 + 4 * k4 + r;
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

// persistent grid: two workgroups per CU at most (the LDS of the 64 x 64 plans: 57 KB forward, 64 KB inverse)
static int many_blocks(int nimg) { return nimg < 2 * 256 ? nimg : 2 * 256; }

template <typename K>
static void many_lds_attr(K kern, size_t lds, size_t& set) {  // > 64 KB of dynamic LDS needs the attribute (once per size per kernel)
    if (lds > 64 * 1024 && lds > set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        set = lds;
    }
}

int cfd_int_dft_many(const cfd_plan* p, const float* x, float* xh, int nimg, int act_in, void* stream) {
    CFD_REQUIRE(p && p->many && p->d_many_fwd, CFD_ERR_INVALID_ARG, "cfd_spectral_dft: not a many-modes plan");
    if (nimg == 0) return CFD_OK;
    hipStream_t st = (hipStream_t)stream;
    const CfdManyDims d = cfd_many_dims(p->H, p->W, p->m1, p->m2);
    const size_t lds = many_fwd_lds_floats(d) * sizeof(float);
    CFD_PROF_W(act_in ? "k_dft_many_act" : "k_dft_many", st, (double)nimg * (4.0 * p->H * p->W + 16.0 * p->m1 * p->m2),
               (double)nimg * (4.0 * p->H * p->W * p->m2 + 16.0 * p->H * p->m1 * p->m2));
    static size_t set0 = 0, set1 = 0;
    if (act_in) {
        many_lds_attr(k_dft_many<true>, lds, set1);
        hipLaunchKernelGGL(k_dft_many<true>, dim3(many_blocks(nimg)), dim3(256), lds, st, x, (float2*)xh, (const float*)p->d_many_fwd, nimg,
                           p->H, p->W, p->m1, p->m2);
    } else {
        many_lds_attr(k_dft_many<false>, lds, set0);
        hipLaunchKernelGGL(k_dft_many<false>, dim3(many_blocks(nimg)), dim3(256), lds, st, x, (float2*)xh, (const float*)p->d_many_fwd, nimg,
                           p->H, p->W, p->m1, p->m2);
    }
    CFD_LAUNCH_CHECK("cfd_spectral_dft(many modes)");
    return CFD_OK;
}

int cfd_int_idft_many(const cfd_plan* p, const float* z, const float* addend, const float* aprev, float* out, int nimg, int epi, void* stream) {
    CFD_REQUIRE(p && p->many && p->d_many_inv, CFD_ERR_INVALID_ARG, "cfd_spectral_idft: not a many-modes plan");
    if (nimg == 0) return CFD_OK;
    hipStream_t st = (hipStream_t)stream;
    const CfdManyDims d = cfd_many_dims(p->H, p->W, p->m1, p->m2);
    const size_t lds = many_inv_lds_floats(d, p->m2) * sizeof(float);
    CFD_PROF_W(epi == 0 ? "k_idft_many" : (epi == 1 ? "k_idft_many_add" : "k_idft_many_add_dgelu"), st,
               (double)nimg * (4.0 * p->H * p->W * (1 + epi) + 16.0 * p->m1 * p->m2),
               (double)nimg * (4.0 * p->H * p->W * p->m2 + 16.0 * p->H * p->m1 * p->m2));
    const float2* zz = (const float2*)z;
    const float* tab = (const float*)p->d_many_inv;
    const int blocks = many_blocks(nimg);
    static size_t set0 = 0, set1 = 0, set2 = 0;
    if (epi == 0) {
        many_lds_attr(k_idft_many<0>, lds, set0);
        hipLaunchKernelGGL(k_idft_many<0>, dim3(blocks), dim3(256), lds, st, zz, addend, aprev, out, tab, nimg, p->H, p->W, p->m1, p->m2);
    } else if (epi == 1) {
        many_lds_attr(k_idft_many<1>, lds, set1);
        hipLaunchKernelGGL(k_idft_many<1>, dim3(blocks), dim3(256), lds, st, zz, addend, aprev, out, tab, nimg, p->H, p->W, p->m1, p->m2);
    } else {
        many_lds_attr(k_idft_many<2>, lds, set2);
        hipLaunchKernelGGL(k_idft_many<2>, dim3(blocks), dim3(256), lds, st, zz, addend, aprev, out, tab, nimg, p->H, p->W, p->m1, p->m2);
    }
    CFD_LAUNCH_CHECK("cfd_spectral_idft(many modes)");
    return CFD_OK;
}
