// Gradients of the Auto-FNO with respect to its inputs and case parameters: the adjoint of the lifting layer's columns that multiply them
// (fc0 over cat([inputs, mask, grid_x, grid_y, case_params]), src/models/fno/fno2d.py:195-215), taken from g0 = d loss / d fc0 output on
// the data grid.  What autograd computes behind Fno2d.forward when `inputs` / `case_params` require a gradient (a differentiated rollout):
//   d_inputs[b, i, px]  = sum_c w[c, i] g0[b, c, px]
//   d_case_params[b, k] = sum_c w[c, in_chan + 3 + k] sum_px g0[b, c, px]  =  sum_px sum_c w[c, in_chan + 3 + k] g0[b, c, px]
// ONE streaming pass over g0 serves both (the second form of the case-parameter sum: P running sums per lane instead of C).  Memory bound:
// 4 B C HW bytes in, 4 B in_chan HW out.
//
// Workgroup (s, b) = batch entry b, units s * 256 + tid, + S * 256, ... of its plane (a unit = VEC consecutive pixels); lane = one unit:
// it walks the C channel planes (four loads in flight), NI input-channel accumulators per pixel in registers.  The weights lie in LDS,
// zero-padded to NI / 32 columns and uniform over the wave.  More than NI = 8 input channels: the channel walk repeats per group of eight.
// Case parameters: the lane sums meet in cfd_wave_sum, the four waves in LDS in wave order, and the workgroup's P sums go out as ONE record
// part[(b * S + s) * P + k]; k_ingrad_cp adds the S records of an entry in order s = 0 .. S - 1.  With S == 1 the workgroup writes
// d_case_params itself and no record exists.  No atomics: the result depends on the shape, S and VEC alone.
#include "cfd_common.h"
#include "cfd_launch.h"

namespace {

template <int VEC>
__device__ __forceinline__ void ig_ld(const float* src, float (&v)[VEC]) {
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(src);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else if constexpr (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2*>(src);
        v[0] = t.x; v[1] = t.y;
    } else {
        v[0] = src[0];
    }
}
template <int VEC>
__device__ __forceinline__ void ig_st(float* dst, const float (&v)[VEC]) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
    else if constexpr (VEC == 2) *reinterpret_cast<float2*>(dst) = make_float2(v[0], v[1]);
    else dst[0] = v[0];
}

// CP: the case-parameter sums are asked for.  d_in may be NULL (then only the sums are taken), part == NULL means S == 1.
template <int VEC, int NI, bool CP>
__global__ __launch_bounds__(256) void k_ingrad(const float* __restrict__ g0, const float* __restrict__ w, float* __restrict__ d_in,
                                                float* __restrict__ d_cp, float* __restrict__ part, int in_chan, int P, int C, int HW) {
    __shared__ __attribute__((aligned(16))) float s_wi[CFD_WIDE_MAX * NI];
    __shared__ __attribute__((aligned(16))) float s_wp[CP ? CFD_WIDE_MAX * 32 : 4];
    __shared__ float s_red[4 * 32];
    const int tid = (int)threadIdx.x, b = (int)blockIdx.y, S = (int)gridDim.x;
    const int F = in_chan + 3 + P, units = HW / VEC;  // VEC divides HW (the launcher's choice)
    const float* gb = g0 + (size_t)b * C * HW;
    if constexpr (CP) {
        for (int i = tid; i < C * 32; i += 256) {
            const int c = i >> 5, k = i & 31;
            s_wp[i] = k < P ? w[c * F + in_chan + 3 + k] : 0.f;
        }
    }
    float q[CP ? 32 : 1];
#pragma unroll
    for (int k = 0; k < (CP ? 32 : 1); ++k) q[k] = 0.f;
    const int groups = d_in ? (in_chan + NI - 1) / NI : 1;
    for (int grp = 0; grp < groups; ++grp) {
        const int i0 = grp * NI;
        __syncthreads();  // (the previous group's readers are done with s_wi)
        for (int i = tid; i < C * NI; i += 256) {
            const int c = i / NI, k = i0 + i % NI;
            s_wi[i] = (d_in && k < in_chan) ? w[c * F + k] : 0.f;
        }
        __syncthreads();
        const bool sums = CP && grp == 0;
        for (int u = (int)blockIdx.x * 256 + tid; u < units; u += S * 256) {
            const float* src = gb + (size_t)u * VEC;
            float acc[NI][VEC];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int v = 0; v < VEC; ++v) acc[i][v] = 0.f;
            auto step = [&](int c, const float (&g)[VEC]) {
                if (d_in) {  // (the case-parameter-only form takes the sums alone)
                    const float* wi = s_wi + c * NI;
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const float wv = wi[i];
#pragma unroll
                        for (int v = 0; v < VEC; ++v) acc[i][v] = fmaf(wv, g[v], acc[i][v]);
                    }
                }
                if constexpr (CP) {
                    if (sums) {
                        float gs = g[0];
                        if constexpr (VEC == 4) gs = (g[0] + g[1]) + (g[2] + g[3]);
                        else if constexpr (VEC == 2) gs = g[0] + g[1];
                        const float* wp = s_wp + c * 32;
#pragma unroll
                        for (int k4 = 0; k4 < 8; ++k4)
                            if (4 * k4 < P) {
#pragma unroll
                                for (int k = 4 * k4; k < 4 * k4 + 4; ++k) q[k] = fmaf(wp[k], gs, q[k]);
                            }
                    }
                }
            };
            int c = 0;
            for (; c + 4 <= C; c += 4) {  // four channel planes in flight
                float g[4][VEC];
#pragma unroll
                for (int j = 0; j < 4; ++j) ig_ld<VEC>(src + (size_t)(c + j) * HW, g[j]);
#pragma unroll
                for (int j = 0; j < 4; ++j) step(c + j, g[j]);
            }
            for (; c < C; ++c) {
                float g[VEC];
                ig_ld<VEC>(src + (size_t)c * HW, g);
                step(c, g);
            }
            if (d_in) {
                float* dst = d_in + ((size_t)b * in_chan + i0) * HW + (size_t)u * VEC;
#pragma unroll
                for (int i = 0; i < NI; ++i)
                    if (i0 + i < in_chan) ig_st<VEC>(dst + (size_t)i * HW, acc[i]);
            }
        }
    }
    if constexpr (CP) {
        const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < P) {  // (uniform: the sums beyond P are zero and nobody reads them)
                const float s = cfd_wave_sum(q[k]);
                if (lane == 0) s_red[wave * 32 + k] = s;
            }
        __syncthreads();
        if (tid < P) {
            const float tot = ((s_red[tid] + s_red[32 + tid]) + s_red[64 + tid]) + s_red[96 + tid];
            if (part) part[((size_t)b * S + blockIdx.x) * P + tid] = tot;
            else d_cp[(size_t)b * P + tid] = tot;
        }
    }
}

// d_cp[b][k] = the S records of entry b in order
__global__ __launch_bounds__(256) void k_ingrad_cp(const float* __restrict__ part, float* __restrict__ d_cp, int n, int S, int P) {
    const int e = (int)blockIdx.x * 256 + (int)threadIdx.x;  // (b, k)
    if (e >= n) return;
    const int b = e / P, k = e - b * P;
    const float* src = part + (size_t)b * S * P + k;
    float tot = 0.f;
    for (int s = 0; s < S; ++s) tot += src[(size_t)s * P];
    d_cp[e] = tot;
}

}  // namespace

int cfd_int_fno_ingrad(const float* g0, const float* w, float* d_inputs, float* d_case_params, void* ws, size_t ws_bytes, int B, int in_chan,
                       int P, int C, int HW, void* stream) {
    if (P == 0) d_case_params = nullptr;
    if (!d_inputs && !d_case_params) return CFD_OK;
    CFD_REQUIRE(g0 && w, CFD_ERR_INVALID_ARG, "cfd_fno_ingrad: NULL pointer");
    CFD_REQUIRE(B >= 1 && in_chan >= 1 && P >= 0 && C >= 1 && HW >= 1, CFD_ERR_INVALID_ARG, "cfd_fno_ingrad: bad sizes");
    CFD_REQUIRE(in_chan + 3 + P <= 32 && C <= CFD_WIDE_MAX, CFD_ERR_UNSUPPORTED,
                "cfd_fno_ingrad: features=%d (max 32) / hidden=%d (max %d) unsupported", in_chan + 3 + P, C, CFD_WIDE_MAX);
    CFD_REQUIRE(B <= 65535, CFD_ERR_UNSUPPORTED, "cfd_fno_ingrad: B=%d (max 65535)", B);
    CFD_REQUIRE_I31((long)B * C * HW, "cfd_fno_ingrad");
    hipStream_t st = (hipStream_t)stream;
    // include/cfdbench_amd.h, "Alignment": the 16- or 8-byte form only when g0, d_inputs and the plane length all allow it
    const uintptr_t ptrs = (uintptr_t)g0 | (uintptr_t)d_inputs;
    const int vec = (HW % 4 == 0 && ptrs % 16 == 0) ? 4 : (HW % 2 == 0 && ptrs % 8 == 0) ? 2 : 1;
    // S workgroups per batch entry: one trip per lane until the device has ~4 workgroups per CU, then longer walks
    const int chunks = (HW / vec + 255) / 256;
    int S = (1024 + B - 1) / B;
    S = S < chunks ? S : chunks;
    S = S > 64 ? 64 : S;
    float* part = nullptr;
    if (d_case_params && S > 1) {
        // the records must fit the scratch the caller has: fewer, longer partials where they would not (S == 1 needs none).  Against the
        // lifting layer's scratch (workgroups x C x (features + 1) floats; 1024 workgroups at large batches) the S B P < 2048 P floats of
        // the records overflow only at hidden = 1, from about B = 500 with P >= 11; tests/test_gpu_fno_ingrad.py runs that shape
        // (B = 500, hidden 1, 33 x 33, P = 12: S = 3 is cut to 2; minutes on the emulator, so on the device only).
        const size_t per = (size_t)B * P * sizeof(float);
        const size_t fit = (ws && ((uintptr_t)ws % 4) == 0) ? ws_bytes / per : 0;
        if ((size_t)S > fit) S = fit < 1 ? 1 : (int)fit;
        if (S > 1) part = (float*)ws;
    }
    const dim3 grid((unsigned)S, (unsigned)B);
    {
        CFD_PROF_W("k_ingrad", st, 4.0 * B * HW * ((double)C + (d_inputs ? in_chan : 0)),
                   2.0 * B * HW * (double)C * ((d_inputs ? in_chan : 0) + (d_case_params ? P : 0)));
        cfd_dispatch([&](auto V, auto N, auto CP) {
            hipLaunchKernelGGL((k_ingrad<CFD_I(V), CFD_I(N), CFD_B(CP)>), grid, dim3(256), 0, st, g0, w, d_inputs, d_case_params, part, in_chan, P,
                               C, HW);
        }, cfd_among<4, 2, 1>(vec), cfd_among<4, 8>(in_chan <= 4 ? 4 : 8), d_case_params != nullptr);
        CFD_LAUNCH_CHECK("cfd_fno_ingrad");
    }
    if (part) {
        CFD_PROF_W("k_ingrad_cp", st, 0.0, 0.0);  // partial sums are an implementation detail
        const int n = B * P;
        hipLaunchKernelGGL(k_ingrad_cp, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const float*)part, d_case_params, n, S, P);
        CFD_LAUNCH_CHECK("cfd_fno_ingrad(reduce)");
    }
    return CFD_OK;
}
