// Domain padding of the Auto-FNO (Fno2d(padding = p), src/models/fno/fno2d.py:219-226): the two boundaries between the H x W data grid and
// the (H + p) x (W + p) grid the FnoBlocks run on.
//   F.pad(fc0(features), [0, p, 0, p])    fno2d.py:217-221   -> k_stem_pad  (lifting layer written straight into the padded layout)
//   x[..., :-p, :-p]                      fno2d.py:225-226   -> k_pad_crop  (a_L in front of the head, g_0 in front of the lifting layer's gradient)
//   its adjoint (zero band)                                  -> k_pad_embed (the head's d loss / d a_L)
// All three are fp32 streaming kernels: workgroup (x, y) = (image, chunk of its plane), both grid-stride; 16-byte accesses when W and W + p
// are multiples of 4 and every pointer is 16-byte aligned (then a group of four columns is interior or band as a whole), 4-byte accesses
// otherwise.  The band is WRITTEN on every call: the workspace is the caller's and may hold anything.
#include "cfd_common.h"
#include "cfd_launch.h"

namespace {

// grid of a launch over n planes of `units` work items each: 256 items per workgroup and trip, at most 16 chunks per plane, 4096 workgroups
dim3 plane_grid(long n, int units) {
    int gy = (units + 255) / 256;
    gy = gy < 1 ? 1 : (gy > 16 ? 16 : gy);
    const long cap = 4096 / gy;
    return dim3((unsigned)(n < 1 ? 1 : (n > cap ? cap : n)), (unsigned)gy);
}

template <int VEC>
__device__ __forceinline__ void st_vec(float* dst, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else dst[0] = v[0];
}
template <int VEC>
__device__ __forceinline__ void ld_vec(const float* src, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(src);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = src[0];
    }
}

}  // namespace

// out[b][o][row][col] (B, C, H + pad, W + pad) = bias[o] + sum_f w[o * F + f] feat_f(b, row, col) for row < H and col < W, 0.0f in the band
// (the reference pads AFTER fc0: no bias there).  Features [inputs, mask or 1, grid_x(row), grid_y(col), case params] (fno2d.py:195-214),
// F <= 32, one fmaf per feature in that order on top of the bias -- k_stem_fwd's chain, so an interior value is the unpadded stem's bit for
// bit.  The coordinates are the DATA grid's np.linspace(0, 1, n) as float32 (make_grids, plan.cpp: (float)((double)i * (1.0 / (n - 1))),
// the last one exactly 1; rx, ry are the two reciprocals, made on the host in double): thread t tabulates one of the H + W <= 254 values
// in LDS, and workgroup (0, 0) leaves the table in `coords` (gx at 0, gy at CFD_PAD_COORD_GY; may be NULL) for the backward pass.
// One kernel for every hidden width 1 .. 128: weights in LDS as [channel][32] (16 KB), uniform over the wave; lane = VEC pixels of a row
// with their features in registers.
template <int VEC>
__global__ __launch_bounds__(256) void k_stem_pad(const float* __restrict__ inputs, const float* __restrict__ mask,
                                                  const float* __restrict__ cp, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ coords,
                                                  int B, int in_chan, int P, int C, int H, int W, int pad, double rx, double ry, CfdDiv dv) {
    __shared__ __attribute__((aligned(16))) float s_w[CFD_WIDE_MAX * 32];
    __shared__ float s_b[CFD_WIDE_MAX];
    __shared__ float s_g[256];
    const int F = in_chan + 3 + P, Hp = H + pad, Wp = W + pad, HW = H * W;
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < C * F; i += 256) s_w[(i / F) * 32 + i % F] = w[i];
    for (int i = tid; i < C; i += 256) s_b[i] = bias[i];
    {
        float g = 0.f;
        if (tid < H) g = tid == H - 1 ? 1.0f : (float)((double)tid * rx);
        else if (tid < H + W) g = tid - H == W - 1 ? 1.0f : (float)((double)(tid - H) * ry);
        s_g[tid] = g;
        if (coords && blockIdx.x == 0 && blockIdx.y == 0) {
            if (tid < H) coords[tid] = g;
            else if (tid < H + W) coords[CFD_PAD_COORD_GY + tid - H] = g;
        }
    }
    __syncthreads();
    const int upr = Wp / VEC, units = Hp * upr;  // VEC divides W and Wp (checked by the launcher)
    const size_t plane = (size_t)Hp * Wp;
    for (int b = (int)blockIdx.x; b < B; b += (int)gridDim.x) {
        for (int u = (int)blockIdx.y * 256 + tid; u < units; u += (int)gridDim.y * 256) {
            const int row = (int)cfd_div((unsigned)u, dv), col = (u - row * upr) * VEC;
            float* dst = out + (size_t)b * C * plane + (size_t)row * Wp + col;
            float acc[VEC];
            if (row >= H || col >= W) {  // band
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = 0.0f;
                for (int o = 0; o < C; ++o) st_vec<VEC>(dst + (size_t)o * plane, acc);
                continue;
            }
            const int p = row * W + col;
            float f[32][VEC];
#pragma unroll
            for (int k = 0; k < 32; ++k) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) f[k][v] = 0.f;
                if (k < in_chan) ld_vec<VEC>(inputs + ((size_t)b * in_chan + k) * HW + p, f[k]);
                else if (k == in_chan) {
                    if (mask) ld_vec<VEC>(mask + (size_t)b * HW + p, f[k]);
                    else {
#pragma unroll
                        for (int v = 0; v < VEC; ++v) f[k][v] = 1.f;
                    }
                } else if (k == in_chan + 1) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) f[k][v] = s_g[row];
                } else if (k == in_chan + 2) {
#pragma unroll
                    for (int v = 0; v < VEC; ++v) f[k][v] = s_g[H + col + v];
                } else if (k < F) {
                    const float c1 = cp[(size_t)b * P + (k - in_chan - 3)];
#pragma unroll
                    for (int v = 0; v < VEC; ++v) f[k][v] = c1;
                }
            }
            for (int o = 0; o < C; ++o) {
                const float* wo = s_w + o * 32;
                const float bo = s_b[o];
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[v] = bo;
#pragma unroll
                for (int k = 0; k < 32; ++k)
                    if (k < F) {
                        const float wk = wo[k];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[v] = fmaf(wk, f[k][v], acc[v]);
                    }
                st_vec<VEC>(dst + (size_t)o * plane, acc);
            }
        }
    }
}

// out (n, H, W) = in (n, H + pad, W + pad)[:, :H, :W]: a raw copy (consumers keep applying GELU on load)
template <int VEC>
__global__ __launch_bounds__(256) void k_pad_crop(const float* __restrict__ in, float* __restrict__ out, long n, int H, int W, int pad,
                                                  CfdDiv dv) {
    const int Wp = W + pad, upr = W / VEC, units = H * upr;
    const size_t pin = (size_t)(H + pad) * Wp, pout = (size_t)H * W;
    for (long img = blockIdx.x; img < n; img += gridDim.x) {
        const float* src = in + (size_t)img * pin;
        float* dst = out + (size_t)img * pout;
        for (int u = (int)blockIdx.y * 256 + (int)threadIdx.x; u < units; u += (int)gridDim.y * 256) {
            const int row = (int)cfd_div((unsigned)u, dv), col = (u - row * upr) * VEC;
            float v[VEC];
            ld_vec<VEC>(src + (size_t)row * Wp + col, v);
            st_vec<VEC>(dst + (size_t)row * W + col, v);
        }
    }
}

// out (n, H + pad, W + pad): interior = in (n, H, W), band = 0.0f (the adjoint of the crop)
template <int VEC>
__global__ __launch_bounds__(256) void k_pad_embed(const float* __restrict__ in, float* __restrict__ out, long n, int H, int W, int pad,
                                                   CfdDiv dv) {
    const int Hp = H + pad, Wp = W + pad, upr = Wp / VEC, units = Hp * upr;
    const size_t pin = (size_t)H * W, pout = (size_t)Hp * Wp;
    for (long img = blockIdx.x; img < n; img += gridDim.x) {
        const float* src = in + (size_t)img * pin;
        float* dst = out + (size_t)img * pout;
        for (int u = (int)blockIdx.y * 256 + (int)threadIdx.x; u < units; u += (int)gridDim.y * 256) {
            const int row = (int)cfd_div((unsigned)u, dv), col = (u - row * upr) * VEC;
            float v[VEC];
#pragma unroll
            for (int k = 0; k < VEC; ++k) v[k] = 0.0f;
            if (row < H && col < W) ld_vec<VEC>(src + (size_t)row * W + col, v);
            st_vec<VEC>(dst + (size_t)row * Wp + col, v);
        }
    }
}

static bool pad_vec4(int W, int pad, uintptr_t ptrs) { return W % 4 == 0 && (W + pad) % 4 == 0 && ptrs % 16 == 0; }

#define CFD_PAD_REQUIRE(fn)                                                                                                          \
    CFD_REQUIRE(H >= 2 && W >= 2 && pad >= 1 && H + pad <= 128 && W + pad <= 128, CFD_ERR_INVALID_ARG, "%s: grid %dx%d, pad %d", fn, H, W, pad)

int cfd_int_stem_pad(const float* inputs, const float* mask, const float* case_params, const float* w, const float* bias, float* out,
                     float* coords, int B, int in_chan, int P, int C, int H, int W, int pad, void* stream) {
    CFD_REQUIRE(inputs && w && bias && out && (P == 0 || case_params), CFD_ERR_INVALID_ARG, "cfd_fno_stem_pad: NULL pointer");
    CFD_REQUIRE(B >= 1 && in_chan >= 1 && P >= 0 && C >= 1, CFD_ERR_INVALID_ARG, "cfd_fno_stem_pad: bad sizes");
    CFD_PAD_REQUIRE("cfd_fno_stem_pad");
    CFD_REQUIRE(in_chan + 3 + P <= 32 && C <= CFD_WIDE_MAX, CFD_ERR_UNSUPPORTED,
                "cfd_fno_stem_pad: features=%d (max 32) / hidden=%d (max %d) unsupported", in_chan + 3 + P, C, CFD_WIDE_MAX);
    hipStream_t st = (hipStream_t)stream;
    const int Hp = H + pad, Wp = W + pad;
    const double rx = 1.0 / (double)(H - 1), ry = 1.0 / (double)(W - 1);
    CFD_PROF_W("k_stem_pad", st, (double)B * (4.0 * H * W * (in_chan + 1) + 4.0 * C * Hp * Wp), 2.0 * B * H * W * (double)C * (in_chan + 3 + P));
    cfd_dispatch([&](auto V) {  // (V pixels of a padded row per thread)
        hipLaunchKernelGGL(k_stem_pad<CFD_I(V)>, plane_grid(B, Hp * (Wp / CFD_I(V))), dim3(256), 0, st, inputs, mask, case_params, w, bias, out,
                           coords, B, in_chan, P, C, H, W, pad, rx, ry, cfd_div_make((unsigned)(Wp / CFD_I(V))));
    }, cfd_among<4, 1>(pad_vec4(W, pad, (uintptr_t)inputs | (uintptr_t)mask | (uintptr_t)out) ? 4 : 1));
    CFD_LAUNCH_CHECK("cfd_fno_stem_pad");
    return CFD_OK;
}

int cfd_int_pad_crop(const float* in, float* out, long n, int H, int W, int pad, void* stream) {
    CFD_REQUIRE(in && out && n >= 1, CFD_ERR_INVALID_ARG, "cfd_fno_pad_crop: NULL pointer / empty tensor");
    CFD_PAD_REQUIRE("cfd_fno_pad_crop");
    hipStream_t st = (hipStream_t)stream;
    CFD_PROF_W("k_pad_crop", st, 8.0 * n * H * W, 0.0);
    cfd_dispatch([&](auto V) {
        hipLaunchKernelGGL(k_pad_crop<CFD_I(V)>, plane_grid(n, H * (W / CFD_I(V))), dim3(256), 0, st, in, out, n, H, W, pad,
                           cfd_div_make((unsigned)(W / CFD_I(V))));
    }, cfd_among<4, 1>(pad_vec4(W, pad, (uintptr_t)in | (uintptr_t)out) ? 4 : 1));
    CFD_LAUNCH_CHECK("cfd_fno_pad_crop");
    return CFD_OK;
}

int cfd_int_pad_embed(const float* in, float* out, long n, int H, int W, int pad, void* stream) {
    CFD_REQUIRE(in && out && n >= 1, CFD_ERR_INVALID_ARG, "cfd_fno_pad_embed: NULL pointer / empty tensor");
    CFD_PAD_REQUIRE("cfd_fno_pad_embed");
    hipStream_t st = (hipStream_t)stream;
    const int Hp = H + pad, Wp = W + pad;
    CFD_PROF_W("k_pad_embed", st, 4.0 * n * ((double)H * W + (double)Hp * Wp), 0.0);
    cfd_dispatch([&](auto V) {
        hipLaunchKernelGGL(k_pad_embed<CFD_I(V)>, plane_grid(n, Hp * (Wp / CFD_I(V))), dim3(256), 0, st, in, out, n, H, W, pad,
                           cfd_div_make((unsigned)(Wp / CFD_I(V))));
    }, cfd_among<4, 1>(pad_vec4(W, pad, (uintptr_t)in | (uintptr_t)out) ? 4 : 1));
    CFD_LAUNCH_CHECK("cfd_fno_pad_embed");
    return CFD_OK;
}
