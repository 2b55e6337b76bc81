// Wide-channel route of the FNO (hidden width 33 .. 128): the kernels the forward pass needs where a layer has more than 32
// input or output channels.  The <= 32 kernels of spectral.hip / pointwise.hip / head.hip hold a whole channel set in one
// register tile or one MFMA K step; these loop over channels at run time instead.  Exact fp32 FMA chains (fp32-exact class
// like the rest of the package), every output a single chain in a fixed order: deterministic, no atomics.
//
//   k_wide_cgemm   per kept mode a complex GEMM: the forward mix (B x Cin).(Cin x Cout), the adjoint mix with conj(W)
//                  and the spectral weight gradient sum_b conj(x[b,i]) g[b,o] (scaled by c_l / HW)
//   k_wide_chanmix 1x1 convolution over NCHW (GELU on load of the stored pre-activation, optional transpose of W)
//   k_wide_stem    lifting layer fc0 with C > 32 output channels
//   k_wide_head    projection head Linear(C, 128) -> GELU -> Linear(128, out_chan), mask, and the masked loss partial sums
//   k_wide_head_bwd_px  the head's backward per pixel: hidden activations, d loss / d preds and d loss / d hidden pre-activation
//   k_wide_wgrad_part   weight + bias gradients sum_px U[u][px] V[v][px] (1x1 conv, lifting layer, both head layers): pixel tiles
//                  through LDS, one partial record per workgroup, reduced in a fixed order by k_wide_wgrad_reduce
#include "cfd_common.h"
#include "cfd_launch.h"
#include "cfd_tail.h"  // CFD_HEAD_HD

namespace {

// ---- mode-domain complex GEMM ---------------------------------------------------------------------------------------------
// Operand element (row r, column k, kept mode m): base + r * sr + k * sk + m, where a SPLIT operand (the spectral weights, one
// tensor per half of the kept modes: weights1 for rows 0 .. m1-1 of the (2 m1, m2) mode grid, weights2 for the rest) picks
// p1 / p2 by m < half and indexes with m mod half.
struct COp {
    const float2* p1;
    const float2* p2;  // NULL: not split
    long sr, sk;
};
struct COut {
    float2* p1;
    float2* p2;
    long sr, sc;
};

__device__ __forceinline__ const float2* cop_at(const COp& o, int m, int half) {
    return o.p2 ? (m < half ? o.p1 + m : o.p2 + (m - half)) : o.p1 + m;
}

#define WIDE_TR 4  // rows per lane
#define WIDE_TC 8  // columns per lane
#define WIDE_WPB 4 // waves per workgroup (each its own row tile)

// out[r][c][m] = scale[m] * sum_k A'[r][k][m] B'[k][c][m]  (A' = conj(A) with CA, B' = conj(B) with CB); lane = kept mode,
// wave = tile of WIDE_TR rows, blockIdx.z = tile of WIDE_TC columns.  Rows / columns past the end load clamped addresses and
// are never stored.
template <bool CA, bool CB>
__global__ __launch_bounds__(64 * WIDE_WPB) void k_wide_cgemm(const COp A, const COp Bm, const COut O, int R, int K, int N, int M,
                                                              int half, const float* __restrict__ clhw, int m2) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = blockIdx.x * 64 + lane;
    if (m >= M) return;
    const int r0 = (blockIdx.y * WIDE_WPB + wave) * WIDE_TR, c0 = blockIdx.z * WIDE_TC;
    if (r0 >= R) return;
    const float2* a = cop_at(A, m, half);
    const float2* b = cop_at(Bm, m, half);
    long ar[WIDE_TR], bc[WIDE_TC];
#pragma unroll
    for (int i = 0; i < WIDE_TR; ++i) ar[i] = (long)(r0 + i < R ? r0 + i : R - 1) * A.sr;
#pragma unroll
    for (int j = 0; j < WIDE_TC; ++j) bc[j] = (long)(c0 + j < N ? c0 + j : N - 1) * Bm.sr;
    float2 acc[WIDE_TR][WIDE_TC];
#pragma unroll
    for (int i = 0; i < WIDE_TR; ++i)
#pragma unroll
        for (int j = 0; j < WIDE_TC; ++j) acc[i][j] = make_float2(0.f, 0.f);
    for (int k = 0; k < K; ++k) {
        float2 av[WIDE_TR], bv[WIDE_TC];
#pragma unroll
        for (int i = 0; i < WIDE_TR; ++i) {
            av[i] = a[ar[i] + (long)k * A.sk];
            if (CA) av[i].y = -av[i].y;
        }
#pragma unroll
        for (int j = 0; j < WIDE_TC; ++j) {
            bv[j] = b[bc[j] + (long)k * Bm.sk];
            if (CB) bv[j].y = -bv[j].y;
        }
#pragma unroll
        for (int i = 0; i < WIDE_TR; ++i)
#pragma unroll
            for (int j = 0; j < WIDE_TC; ++j) {
                acc[i][j].x = fmaf(av[i].x, bv[j].x, acc[i][j].x);
                acc[i][j].x = fmaf(-av[i].y, bv[j].y, acc[i][j].x);
                acc[i][j].y = fmaf(av[i].x, bv[j].y, acc[i][j].y);
                acc[i][j].y = fmaf(av[i].y, bv[j].x, acc[i][j].y);
            }
    }
    const float sc = clhw ? clhw[m % m2] : 1.f;
    float2* o = O.p2 ? (m < half ? O.p1 + m : O.p2 + (m - half)) : O.p1 + m;
#pragma unroll
    for (int i = 0; i < WIDE_TR; ++i)
#pragma unroll
        for (int j = 0; j < WIDE_TC; ++j)
            if (r0 + i < R && c0 + j < N)
                o[(long)(r0 + i) * O.sr + (long)(c0 + j) * O.sc] = make_float2(acc[i][j].x * sc, acc[i][j].y * sc);
}

template <bool CA, bool CB>
void launch_cgemm(const COp& A, const COp& Bm, const COut& O, int R, int K, int N, int M, int half, const float* clhw, int m2,
                  hipStream_t st) {
    const dim3 grid((unsigned)((M + 63) / 64), (unsigned)((R + WIDE_TR * WIDE_WPB - 1) / (WIDE_TR * WIDE_WPB)),
                    (unsigned)((N + WIDE_TC - 1) / WIDE_TC));
    hipLaunchKernelGGL((k_wide_cgemm<CA, CB>), grid, dim3(64 * WIDE_WPB), 0, st, A, Bm, O, R, K, N, M, half, clhw, m2);
}

// ---- 1x1 convolution ---------------------------------------------------------------------------------------------------------
// out[b][o][p] = bias[o] + sum_i W(o, i) f(in[b][i][p]),  W(o, i) = w[o * Ci + i] (transpose: w[i * Co + o]), f = GELU with ACT.
// Lane = pixel (flattened over batch entries), blockIdx.y = chunk of 32 output channels whose weights sit in LDS [i][o].
#define WIDE_OC 32
template <bool ACT>
__global__ __launch_bounds__(256) void k_wide_chanmix(const float* __restrict__ in, const float* __restrict__ w,
                                                      const float* __restrict__ bias, float* __restrict__ out, int B, int Ci,
                                                      int Co, int HW, int transpose, const float* __restrict__ dg) {
    __shared__ float s_w[CFD_WIDE_MAX * WIDE_OC];
    __shared__ float s_b[WIDE_OC];
    const int o0 = blockIdx.y * WIDE_OC;
    for (int t = threadIdx.x; t < Ci * WIDE_OC; t += blockDim.x) {
        const int i = t / WIDE_OC, o = o0 + t % WIDE_OC;
        s_w[t] = o < Co ? (transpose ? w[(size_t)i * Co + o] : w[(size_t)o * Ci + i]) : 0.f;
    }
    for (int t = threadIdx.x; t < WIDE_OC; t += blockDim.x) s_b[t] = (bias && o0 + t < Co) ? bias[o0 + t] : 0.f;
    __syncthreads();
    const long total = (long)B * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long b = idx / HW, p = idx - b * HW;
        float acc[WIDE_OC];
#pragma unroll
        for (int o = 0; o < WIDE_OC; ++o) acc[o] = s_b[o];
        const float* src = in + (size_t)b * Ci * HW + p;
        for (int i = 0; i < Ci; ++i) {
            float v = src[(size_t)i * HW];
            if (ACT) v = cfd_gelu(v);
#pragma unroll
            for (int o = 0; o < WIDE_OC; ++o) acc[o] = fmaf(s_w[i * WIDE_OC + o], v, acc[o]);
        }
        float* dst = out + (size_t)b * Co * HW + p;
        const float* dgp = dg ? dg + (size_t)b * Co * HW + p : nullptr;  // epilogue * gelu'(dg) (an input gradient through GELU)
#pragma unroll
        for (int o = 0; o < WIDE_OC; ++o)
            if (o0 + o < Co) {
                float v = acc[o];
                if (dgp) v *= cfd_gelu_grad2(cfd_f2{dgp[(size_t)(o0 + o) * HW], 0.f}).x;
                dst[(size_t)(o0 + o) * HW] = v;
            }
    }
}

int grid_blocks(long total, int cap) {
    long g = (total + 255) / 256;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// ---- lifting layer ----------------------------------------------------------------------------------------------------------
// out[b][o][p] = bias[o] + sum_f w[o * F + f] feat_f(b, p), features [inputs, mask, grid_x(row), grid_y(col), case params]
// (fno2d.py:195-214), F <= 32; lane = pixel, the features in registers, the weights uniform over the wave.
__global__ __launch_bounds__(256) void k_wide_stem(const float* __restrict__ inputs, const float* __restrict__ mask,
                                                   const float* __restrict__ cp, const float* __restrict__ gx,
                                                   const float* __restrict__ gy, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out, int B, int in_chan,
                                                   int P, int C, int H, int W) {
    const int HW = H * W, F = in_chan + 3 + P;
    const long total = (long)B * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int b = (int)(idx / HW), p = (int)(idx - (long)b * HW);
        float f[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) {
            float v = 0.f;
            if (k < in_chan) v = inputs[((size_t)b * in_chan + k) * HW + p];
            else if (k == in_chan) v = mask ? mask[(size_t)b * HW + p] : 1.f;
            else if (k == in_chan + 1) v = gx[p / W];
            else if (k == in_chan + 2) v = gy[p % W];
            else if (k < F) v = cp[(size_t)b * P + (k - in_chan - 3)];
            f[k] = v;
        }
        for (int o = 0; o < C; ++o) {
            float acc = bias[o];
            const float* wo = w + (size_t)o * F;
#pragma unroll
            for (int k = 0; k < 32; ++k)
                if (k < F) acc = fmaf(wo[k], f[k], acc);
            out[((size_t)b * C + o) * HW + p] = acc;
        }
    }
}

// ---- projection head -------------------------------------------------------------------------------------------------------
// preds[b][k][p] = mask * (b2[k] + sum_j w2[k][j] gelu(b1[j] + sum_c w1[j][c] f(a[b][c][p]))), k < Co <= NCO (2, or 8 for out_chan 3 .. 8); lane = pixel with
// its CMAX input channels in registers, the 128 hidden units in a rolled loop (weights uniform over the wave).  With a label,
// each workgroup leaves {sum d^2, sum |d|, sum (label*mask)^2} of its pixels (d = preds - label*mask) in part[blockIdx.x].
template <int CMAX, bool ACT, int NCO = 2>
__global__ __launch_bounds__(256) void k_wide_head(const float* __restrict__ a, const float* __restrict__ mask,
                                                   const float* __restrict__ label, const float* __restrict__ w1,
                                                   const float* __restrict__ b1, const float* __restrict__ w2,
                                                   const float* __restrict__ b2, float* __restrict__ preds, float* __restrict__ part,
                                                   int B, int C, int Co, int HW) {
    __shared__ float s_red[3][256];
    const long total = (long)B * HW;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long b = idx / HW, p = idx - b * HW;
        float x[CMAX];
        const float* src = a + (size_t)b * C * HW + p;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            float v = c < C ? src[(size_t)c * HW] : 0.f;
            if (ACT) v = cfd_gelu(v);
            x[c] = v;
        }
        float o[NCO];  // fc2 accumulators, one FMA chain over the hidden units per channel
#pragma unroll
        for (int k = 0; k < NCO; ++k) o[k] = 0.f;
        for (int j = 0; j < CFD_HEAD_HD; ++j) {
            const float* wj = w1 + (size_t)j * C;
            float z = b1[j];
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) z = fmaf(wj[c], x[c], z);
            const float h = cfd_gelu(z);
#pragma unroll
            for (int k = 0; k < NCO; ++k)
                if (k < Co) o[k] = fmaf(w2[k * CFD_HEAD_HD + j], h, o[k]);
        }
        const float mv = mask ? mask[(size_t)b * HW + p] : 1.f;
#pragma unroll
        for (int k = 0; k < NCO; ++k) {
            if (k >= Co) break;
            const float pr = (o[k] + b2[k]) * mv;
            preds[((size_t)b * Co + k) * HW + p] = pr;
            if (label) {
                const float l = label[((size_t)b * Co + k) * HW + p] * mv;
                const float d = pr - l;
                s0 = fmaf(d, d, s0);
                s1 += fabsf(d);
                s2 = fmaf(l, l, s2);
            }
        }
    }
    if (!part) return;
    s_red[0][threadIdx.x] = s0, s_red[1][threadIdx.x] = s1, s_red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {  // fixed tree: deterministic
        if ((int)threadIdx.x < s)
            for (int r = 0; r < 3; ++r) s_red[r][threadIdx.x] += s_red[r][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 3) part[(size_t)blockIdx.x * 3 + threadIdx.x] = s_red[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void k_wide_loss_final(const float* __restrict__ part, int nblk, float count, float* __restrict__ sums,
                                                        int all) {
    if (threadIdx.x != 0) return;
    float a = 0.f, b = 0.f, c = 0.f;
    for (int k = 0; k < nblk; ++k) { a += part[k * 3]; b += part[k * 3 + 1]; c += part[k * 3 + 2]; }
    sums[0] = a, sums[1] = b;
    if (all) sums[2] = c, sums[3] = count;  // (the training step takes them from cfd_label_energy_coef)
}

#define WIDE_HEAD_BLOCKS 1024

// ---- head backward, per pixel ------------------------------------------------------------------------------------------------
// Lane = pixel of a batch chunk.  Writes h[j] = gelu(z[j]) (hbuf), d loss / d raw output (dout = (gext + coef0 2 d + coef1 sign d)
// * mask, d = preds - label*mask) and d loss / d z[j] = gelu'(z[j]) sum_k w2[k][j] dout[k] (zbuf, which holds z[j] in between).
template <int CMAX, bool ACT, int NCO = 2>
__global__ __launch_bounds__(256) void k_wide_head_bwd_px(const float* __restrict__ a, const float* __restrict__ mask,
                                                          const float* __restrict__ label, const float* __restrict__ preds,
                                                          const float* __restrict__ gext, const float* __restrict__ coef,
                                                          const float* __restrict__ w1, const float* __restrict__ b1,
                                                          const float* __restrict__ w2, float* __restrict__ zbuf, float* __restrict__ hbuf,
                                                          float* __restrict__ dout, int B, int C, int Co, int HW) {
    constexpr int HD = CFD_HEAD_HD;
    const long total = (long)B * HW;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long b = idx / HW, p = idx - b * HW;
        float x[CMAX];
        const float* src = a + (size_t)b * C * HW + p;
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            float v = c < C ? src[(size_t)c * HW] : 0.f;
            if (ACT) v = cfd_gelu(v);
            x[c] = v;
        }
        float* zp = zbuf + (size_t)b * HD * HW + p;
        float* hp = hbuf + (size_t)b * HD * HW + p;
        for (int j = 0; j < HD; ++j) {
            const float* wj = w1 + (size_t)j * C;
            float z = b1[j];
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) z = fmaf(wj[c], x[c], z);
            zp[(size_t)j * HW] = z;
            hp[(size_t)j * HW] = cfd_gelu(z);
        }
        const float mv = mask ? mask[(size_t)b * HW + p] : 1.f;
        float d[NCO];
#pragma unroll
        for (int k = 0; k < NCO; ++k) d[k] = 0.f;
#pragma unroll
        for (int k = 0; k < NCO; ++k) {
            if (k >= Co) break;
            const size_t e = ((size_t)b * Co + k) * HW + p;
            float g = gext ? gext[e] : 0.f;
            if (label) {
                const float dd = preds[e] - label[e] * mv;
                g = fmaf(coef[0], 2.f * dd, g);
                g = fmaf(coef[1], (float)((dd > 0.f) - (dd < 0.f)), g);
            }
            d[k] = g * mv;
            dout[e] = d[k];
        }
        for (int j = 0; j < HD; ++j) {
            float gh = w2[j] * d[0];  // d/dg = sum_k w2[k][j] dout[k], in channel order
#pragma unroll
            for (int k = 1; k < NCO; ++k)
                if (k < Co) gh = fmaf(w2[k * HD + j], d[k], gh);
            zp[(size_t)j * HW] = gh * cfd_gelu_grad2(cfd_f2{zp[(size_t)j * HW], 0.f}).x;
        }
    }
}

// ---- weight gradients ----------------------------------------------------------------------------------------------------
// part[blockIdx.x][u][v] (+)= sum over this workgroup's pixel tiles of U[b][u][p] V'[b][v][p], u < NU, v <= NV, where V' is V (GELU
// on load with act), or the lifting layer's features (feat), and row NV of V' is all ones (the bias gradient).  64-pixel tiles of
// the flattened (entry, pixel) index go through LDS; thread (to, ti) of 16 x 16 owns rows to + 16 a and columns ti + 16 c.
struct WideV {
    const float* t;  // (B, NV, HW) rows, or NULL: features
    int act;
    const float *inputs, *mask, *cp, *gx, *gy;
    int in_chan, P, W;
};
#define WIDE_WG_UP 129  // LDS pitch of a U pixel row (floats)
#define WIDE_WG_VP 133
template <int NA, int NC>
__global__ __launch_bounds__(256) void k_wide_wgrad_part(const float* __restrict__ U, int NU, const WideV vs, int NV, int B, int HW,
                                                         float* __restrict__ part, int accumulate) {
    __shared__ float sU[64 * WIDE_WG_UP];
    __shared__ float sV[64 * WIDE_WG_VP];
    const int to = threadIdx.x >> 4, ti = threadIdx.x & 15;
    const long total = (long)B * HW, ntile = (total + 63) / 64;
    float acc[NA][NC];
#pragma unroll
    for (int x = 0; x < NA; ++x)
#pragma unroll
        for (int y = 0; y < NC; ++y) acc[x][y] = 0.f;
    for (long tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
        for (int e = threadIdx.x; e < NU * 64; e += 256) {
            const int u = e >> 6, px = e & 63;
            const long q = tile * 64 + px;
            float v = 0.f;
            if (q < total) { const long b = q / HW, p = q - b * HW; v = U[((size_t)b * NU + u) * HW + p]; }
            sU[px * WIDE_WG_UP + u] = v;
        }
        for (int e = threadIdx.x; e < (NV + 1) * 64; e += 256) {
            const int r = e >> 6, px = e & 63;
            const long q = tile * 64 + px;
            float v = 0.f;
            if (q < total) {
                const long b = q / HW, p = q - b * HW;
                if (r == NV) v = 1.f;
                else if (vs.t) { v = vs.t[((size_t)b * NV + r) * HW + p]; if (vs.act) v = cfd_gelu(v); }
                else if (r < vs.in_chan) v = vs.inputs[((size_t)b * vs.in_chan + r) * HW + p];
                else if (r == vs.in_chan) v = vs.mask ? vs.mask[(size_t)b * HW + p] : 1.f;
                else if (r == vs.in_chan + 1) v = vs.gx[p / vs.W];
                else if (r == vs.in_chan + 2) v = vs.gy[p % vs.W];
                else v = vs.cp[(size_t)b * vs.P + (r - vs.in_chan - 3)];
            }
            sV[px * WIDE_WG_VP + r] = v;
        }
        __syncthreads();
        for (int px = 0; px < 64; ++px) {
            float uu[NA], vv[NC];
#pragma unroll
            for (int x = 0; x < NA; ++x) uu[x] = (to + 16 * x < NU) ? sU[px * WIDE_WG_UP + to + 16 * x] : 0.f;
#pragma unroll
            for (int y = 0; y < NC; ++y) vv[y] = (ti + 16 * y <= NV) ? sV[px * WIDE_WG_VP + ti + 16 * y] : 0.f;
#pragma unroll
            for (int x = 0; x < NA; ++x)
#pragma unroll
                for (int y = 0; y < NC; ++y) acc[x][y] = fmaf(uu[x], vv[y], acc[x][y]);
        }
        __syncthreads();
    }
    float* dst = part + (size_t)blockIdx.x * NU * (NV + 1);
#pragma unroll
    for (int x = 0; x < NA; ++x)
#pragma unroll
        for (int y = 0; y < NC; ++y) {
            const int u = to + 16 * x, v = ti + 16 * y;
            if (u < NU && v <= NV) {
                float* d = dst + (size_t)u * (NV + 1) + v;
                *d = accumulate ? *d + acc[x][y] : acc[x][y];
            }
        }
}

// gw[u][v] = sum_g part[g][u][v] (v < NV), gb[u] = sum_g part[g][u][NV], in record order
__global__ __launch_bounds__(256) void k_wide_wgrad_reduce(const float* __restrict__ part, int G, int NU, int NV, float* __restrict__ gw,
                                                           float* __restrict__ gb) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, n = NU * (NV + 1);
    if (e >= n) return;
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += part[(size_t)g * n + e];
    const int u = e / (NV + 1), v = e - u * (NV + 1);
    if (v < NV) gw[(size_t)u * NV + v] = s;
    else if (gb) gb[u] = s;
}

#define WIDE_WG_BLOCKS 512
int wgrad_grid(long npx) {
    const long t = (npx + 63) / 64;
    return (int)(t < 1 ? 1 : (t > WIDE_WG_BLOCKS ? WIDE_WG_BLOCKS : t));
}
size_t wgrad_part_bytes(int G, int NU, int NV) { return (size_t)G * NU * (NV + 1) * sizeof(float); }

void launch_wgrad_part(const float* U, int NU, const WideV& vs, int NV, int B, int HW, float* part, int G, int accumulate, hipStream_t st) {
    // (rows of U per tile; a tile of four rows takes five columns of V, the others nine)
    cfd_dispatch([&](auto TU) {
        hipLaunchKernelGGL((k_wide_wgrad_part<CFD_I(TU), CFD_I(TU) == 4 ? 5 : 9>), dim3(G), dim3(256), 0, st, U, NU, vs, NV, B, HW, part, accumulate);
    }, cfd_among<1, 4, 8>(NU <= 16 ? 1 : (NU <= 64 && NV + 1 <= 80) ? 4 : 8));
}
void launch_wgrad_reduce(const float* part, int G, int NU, int NV, float* gw, float* gb, hipStream_t st) {
    const int n = NU * (NV + 1);
    hipLaunchKernelGGL(k_wide_wgrad_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, G, NU, NV, gw, gb);
}

// batch entries per chunk of the head backward: its two (chunk, 128, HW) hidden-unit planes stay near 64 MB
int head_chunk(int B, int HW) {
    const int bc = 65536 / (HW > 0 ? HW : 1);
    return bc < 1 ? 1 : (bc > B ? B : bc);
}

}  // namespace

// Forward (conj_t = 0: z[b,o] = sum_i x[b,i] W[i,o]) or adjoint (conj_t = 1: z[b,i] = sum_o x[b,o] conj(W[i,o])) mode mixing.
int cfd_int_wide_mix(const cfd_plan* p, const float* xh, const float* w1, const float* w2, float* z, int B, int Cin, int Cout,
                     int conj_t, void* stream) {
    const int half = p->m1 * p->m2, M = 2 * half;
    const int Cr = conj_t ? Cout : Cin, Cz = conj_t ? Cin : Cout;
    hipStream_t st = (hipStream_t)stream;
    CFD_PROF_W(conj_t ? "k_wide_mix_adj" : "k_wide_mix", st, 8.0 * M * ((double)B * (Cin + Cout) + (double)Cin * Cout),
               8.0 * B * (double)Cin * Cout * M);
    const COp A{(const float2*)xh, nullptr, (long)Cr * M, (long)M};
    const COut O{(float2*)z, nullptr, (long)Cz * M, (long)M};
    // (conj_t: row = i, k = o; else row = o, k = i)
    const COp W{(const float2*)w1, (const float2*)w2, conj_t ? (long)Cout * half : (long)half, conj_t ? (long)half : (long)Cout * half};
    with_bools([&](auto T) { launch_cgemm<false, CFD_B(T)>(A, W, O, B, Cr, Cz, M, half, nullptr, p->m2, st); }, conj_t != 0);
    CFD_LAUNCH_CHECK("cfd_spectral_mix(wide)");
    return CFD_OK;
}

// gw[i,o,mode] = (c_l / HW) sum_b conj(xh[b,i,mode]) gh[b,o,mode], the batch summed in order by one lane per output.
int cfd_int_wide_wgrad(const cfd_plan* p, const float* xh, const float* gh, float* gw1, float* gw2, int B, int Cin, int Cout,
                       void* stream) {
    const int half = p->m1 * p->m2, M = 2 * half;
    hipStream_t st = (hipStream_t)stream;
    CFD_PROF_W("k_wide_spec_wgrad", st, 8.0 * M * ((double)B * (Cin + Cout) + (double)Cin * Cout), 8.0 * B * (double)Cin * Cout * M);
    const COp A{(const float2*)xh, nullptr, (long)M, (long)Cin * M};     // (row = i, k = b)
    const COp G{(const float2*)gh, nullptr, (long)M, (long)Cout * M};    // (row = o, k = b)
    const COut O{(float2*)gw1, (float2*)gw2, (long)Cout * half, (long)half};
    launch_cgemm<true, false>(A, G, O, Cin, B, Cout, M, half, (const float*)p->d_clhw, p->m2, st);
    CFD_LAUNCH_CHECK("cfd_spectral_wgrad(wide)");
    return CFD_OK;
}

int cfd_int_wide_chanmix(const float* in, const float* w, const float* bias, float* out, int B, int Ci, int Co, int HW, int act_in,
                         int transpose, void* stream, const float* dgelu) {
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)grid_blocks((long)B * HW, 2048), (unsigned)((Co + WIDE_OC - 1) / WIDE_OC));
    CFD_PROF_W(transpose ? "k_wide_chanmix_t" : (act_in ? "k_wide_chanmix_act" : "k_wide_chanmix"), st,
               4.0 * B * HW * ((double)Ci * grid.y + Co), 2.0 * B * HW * (double)Ci * Co);
    with_bools([&](auto A) {
        hipLaunchKernelGGL(k_wide_chanmix<CFD_B(A)>, grid, dim3(256), 0, st, in, w, bias, out, B, Ci, Co, HW, transpose, dgelu);
    }, act_in != 0);
    CFD_LAUNCH_CHECK("cfd_chanmix(wide)");
    return CFD_OK;
}

int cfd_int_wide_stem_fwd(const cfd_plan* p, const float* inputs, const float* mask, const float* case_params, const float* w,
                          const float* bias, float* out, int B, int in_chan, int P, int C, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const long total = (long)B * p->H * p->W;
    CFD_PROF_W("k_wide_stem", st, total * (4.0 * (in_chan + 1) + 4.0 * C), 2.0 * total * (double)C * (in_chan + 3 + P));
    hipLaunchKernelGGL(k_wide_stem, dim3(grid_blocks(total, 4096)), dim3(256), 0, st, inputs, mask, case_params, (const float*)p->d_gx,
                       (const float*)p->d_gy, w, bias, out, B, in_chan, P, C, p->H, p->W);
    CFD_LAUNCH_CHECK("cfd_fno_stem_fwd(wide)");
    return CFD_OK;
}

static size_t wide_head_bwd_layout(int B, int C, int Co, int HW, size_t* off) {  // zbuf | hbuf | dout | part1 | part2
    const int bc = head_chunk(B, HW), G = wgrad_grid((long)bc * HW);
    size_t o = 0;
    const size_t sz[5] = {(size_t)bc * CFD_HEAD_HD * HW * sizeof(float), (size_t)bc * CFD_HEAD_HD * HW * sizeof(float),
                          (size_t)bc * Co * HW * sizeof(float), wgrad_part_bytes(G, CFD_HEAD_HD, C), wgrad_part_bytes(G, Co, CFD_HEAD_HD)};
    for (int k = 0; k < 5; ++k) { if (off) off[k] = o; o += cfd_align_up(sz[k], 256); }
    return o;
}

size_t cfd_int_wide_head_workspace_bytes(int B, int C, int Co, int HW) {
    const size_t fwd = (size_t)grid_blocks((long)B * HW, WIDE_HEAD_BLOCKS) * 3 * sizeof(float);
    const size_t bwd = B > 0 ? wide_head_bwd_layout(B, C, Co, HW, nullptr) : 0;
    return fwd > bwd ? fwd : bwd;
}

int cfd_int_wide_head_bwd(const float* a, const float* mask, const float* label, const float* preds, const float* gext, const float* coef,
                          const float* w1, const float* b1, const float* w2, float* ga, float* gw1, float* gb1, float* gw2, float* gb2,
                          void* ws, int B, int C, int Co, int HW, int act_in, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    size_t off[5];
    wide_head_bwd_layout(B, C, Co, HW, off);
    char* base = (char*)ws;
    float *zbuf = (float*)(base + off[0]), *hbuf = (float*)(base + off[1]), *dout = (float*)(base + off[2]);
    float *part1 = (float*)(base + off[3]), *part2 = (float*)(base + off[4]);
    const int bc = head_chunk(B, HW), G = wgrad_grid((long)bc * HW);
    const WideV va{nullptr, act_in, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1};
    for (int b0 = 0; b0 < B; b0 += bc) {  // chunks in order; the partial records accumulate across them (deterministic)
        const int nb = B - b0 < bc ? B - b0 : bc;
        const size_t ea = (size_t)b0 * C * HW, eo = (size_t)b0 * Co * HW;
        CFD_PROF_W("k_wide_head_bwd_px", st, 4.0 * nb * HW * (C + 4.0 * CFD_HEAD_HD + 3.0 * Co), 2.0 * nb * HW * (double)CFD_HEAD_HD * (C + Co));
        cfd_dispatch([&](auto CM, auto A, auto N) {
            hipLaunchKernelGGL((k_wide_head_bwd_px<CFD_I(CM), CFD_B(A), CFD_I(N)>), dim3(grid_blocks((long)nb * HW, 2048)), dim3(256), 0, st, a + ea,
                               mask ? mask + (size_t)b0 * HW : nullptr, label ? label + eo : nullptr, preds ? preds + eo : nullptr,
                               gext ? gext + eo : nullptr, coef, w1, b1, w2, zbuf, hbuf, dout, nb, C, Co, HW);
        }, cfd_among<64, 128>(C <= 64 ? 64 : 128), act_in != 0, cfd_among<2, 8>(Co <= 2 ? 2 : 8));
        CFD_LAUNCH_CHECK("cfd_fno_head_bwd(wide px)");
        // d loss / d a = W1^T dz (* gelu'(a) where the head reads GELU(a))
        CFD_TRY(cfd_int_wide_chanmix(zbuf, w1, nullptr, ga + ea, nb, CFD_HEAD_HD, C, HW, 0, 1, stream, act_in ? a + ea : nullptr));
        WideV va_c = va;
        va_c.t = a + ea;
        CFD_PROF_W("k_wide_wgrad_part", st, 4.0 * nb * HW * (CFD_HEAD_HD + C), 2.0 * nb * HW * (double)CFD_HEAD_HD * (C + 1));
        launch_wgrad_part(zbuf, CFD_HEAD_HD, va_c, C, nb, HW, part1, G, b0 > 0, st);
        const WideV vh{hbuf, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1};
        launch_wgrad_part(dout, Co, vh, CFD_HEAD_HD, nb, HW, part2, G, b0 > 0, st);
        CFD_LAUNCH_CHECK("cfd_fno_head_bwd(wide wgrad)");
    }
    CFD_PROF_W("k_wide_wgrad_reduce", st, 0.0, 0.0);
    launch_wgrad_reduce(part1, G, CFD_HEAD_HD, C, gw1, gb1, st);
    launch_wgrad_reduce(part2, G, Co, CFD_HEAD_HD, gw2, gb2, st);
    CFD_LAUNCH_CHECK("cfd_fno_head_bwd(wide reduce)");
    return CFD_OK;
}

size_t cfd_int_wide_chan_wgrad_workspace_bytes(int B, int Ci, int Co, int HW) {
    return B > 0 ? wgrad_part_bytes(wgrad_grid((long)B * HW), Co, Ci) : 0;
}

// gw[o][i] = sum_{b,p} g[b,o,p] f(in[b,i,p]), gb[o] = sum g (the 1x1 conv's weight gradient; Ci, Co <= 128)
int cfd_int_wide_chan_wgrad(const float* g, const float* in, float* gw, float* gb, void* ws, int B, int Ci, int Co, int HW, int act_in,
                            void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int G = wgrad_grid((long)B * HW);
    const WideV v{in, act_in, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, 1};
    CFD_PROF_W("k_wide_wgrad_part", st, 4.0 * B * HW * (Ci + Co), 2.0 * B * HW * (double)Co * (Ci + 1));
    launch_wgrad_part(g, Co, v, Ci, B, HW, (float*)ws, G, 0, st);
    CFD_PROF_W("k_wide_wgrad_reduce", st, 0.0, 0.0);
    launch_wgrad_reduce((const float*)ws, G, Co, Ci, gw, gb, st);
    CFD_LAUNCH_CHECK("cfd_chan_wgrad(wide)");
    return CFD_OK;
}

// lifting-layer gradient gw[c][f] = sum g[b,c,p] feat_f(b,p), gb[c] = sum g, C > 32 (features as k_wide_stem)
int cfd_int_wide_stem_bwd(const cfd_plan* p, const float* g, const float* inputs, const float* mask, const float* case_params, float* gw,
                          float* gb, void* ws, int B, int in_chan, int P, int C, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int HW = p->H * p->W, F = in_chan + 3 + P, G = wgrad_grid((long)B * HW);
    const WideV v{nullptr, 0, inputs, mask, case_params, (const float*)p->d_gx, (const float*)p->d_gy, in_chan, P, p->W};
    CFD_PROF_W("k_wide_wgrad_part", st, 4.0 * B * HW * (C + in_chan + 1), 2.0 * B * HW * (double)C * (F + 1));
    launch_wgrad_part(g, C, v, F, B, HW, (float*)ws, G, 0, st);
    launch_wgrad_reduce((const float*)ws, G, C, F, gw, gb, st);
    CFD_LAUNCH_CHECK("cfd_fno_stem_bwd(wide)");
    return CFD_OK;
}

int cfd_int_wide_head_fwd(const float* a, const float* mask, const float* label, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* preds, float* sums, void* ws, int B, int C, int Co, int HW, int act_in, void* stream,
                          int all_sums) {
    hipStream_t st = (hipStream_t)stream;
    const int blocks = grid_blocks((long)B * HW, WIDE_HEAD_BLOCKS);
    float* part = label ? (float*)ws : nullptr;
    CFD_PROF_W("k_wide_head", st, B * HW * (4.0 * C + 4.0 * (1 + (label ? 2 : 1) * Co)), 2.0 * B * HW * (double)CFD_HEAD_HD * (C + Co));
    cfd_dispatch([&](auto CM, auto A, auto N) {  // (out_chan 3 .. 8: eight accumulators)
        hipLaunchKernelGGL((k_wide_head<CFD_I(CM), CFD_B(A), CFD_I(N)>), dim3(blocks), dim3(256), 0, st, a, mask, label, w1, b1, w2, b2, preds, part,
                           B, C, Co, HW);
    }, cfd_among<64, 128>(C <= 64 ? 64 : 128), act_in != 0, cfd_among<2, 8>(Co <= 2 ? 2 : 8));
    CFD_LAUNCH_CHECK("cfd_fno_head_fwd(wide)");
    if (label) {
        hipLaunchKernelGGL(k_wide_loss_final, dim3(1), dim3(64), 0, st, (const float*)part, blocks, (float)((double)B * Co * HW), sums,
                           all_sums);
        CFD_LAUNCH_CHECK("cfd_fno_head_fwd(wide loss)");
    }
    return CFD_OK;
}
