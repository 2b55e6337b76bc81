// Training objectives beside mse / nmse / mae: the relative L2 norm per sample, nMSE per sample and nMSE per channel.
//   LpLoss(d=2, p=2).rel     src/models/fno/utilities3.py:165-214     -> k_obj_part + k_obj_final (value), k_obj_bwd (d value / d preds)
// The gradient on the predictions enters the FNO's backward pass as gpreds_ext; nothing of the head knows about these kernels.
// Definitions, the layout of `rec` and the rounding order: include/cfdbench_amd.h, "Training objectives".
//
// Three launches for value + gradient.  k_obj_part: one workgroup per (slice, part), 16-byte loads, d formed in fp32, d * d and
// (label * mask)^2 exact in fp64 and accumulated there -- per thread in element order, then through LDS on a fixed tree -- one record
// per workgroup.  k_obj_final: ONE workgroup adds the records of every group (a sample: Co * NP neighbouring records, a thread each; a
// channel: B * NP strided records, the whole workgroup each) and leaves (E_g, S_g) per group, the batch-global sums and the value, so no
// workgroup of k_obj_bwd re-adds records: it loads its group's two doubles.  k_obj_bwd: elementwise, coefficient in fp64, one rounding.
// All three are bound by HBM: 12 bytes per element forward (8 without a mask of its own: the mask row is shared by Co slices), 16 to 20
// backward.  No atomics: two calls give the same bits, and the scalar form owns the same elements in the same order as the 16-byte form.
#include <initializer_list>

#include "cfd_common.h"
#include "cfd_launch.h"

#define OBJ_PART_ELEMS 4096  // what one workgroup sums at most while HW <= 4096 * CFD_OBJ_MAX_PARTS: four 16-byte units per thread
#define OBJ_TRIPS 4          // independent 16-byte loads per buffer a thread has in flight

// (an fp64 as two 32-bit words: rec is a float buffer on any 4-byte boundary, like the clip buffer of optim.hip)
__device__ __forceinline__ void obj_store_f64(float* q, double d) {
    unsigned long long u;
    __builtin_memcpy(&u, &d, 8);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    __builtin_memcpy(q, &lo, 4);
    __builtin_memcpy(q + 1, &hi, 4);
}
__device__ __forceinline__ double obj_load_f64(const float* q) {
    unsigned lo, hi;
    __builtin_memcpy(&lo, q, 4);
    __builtin_memcpy(&hi, q + 1, 4);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}
// sums of two quantities over the 256 threads, fixed tree; every thread calls it and gets both totals.  The barrier at the end lets the
// caller enter it again at once.
__device__ __forceinline__ void obj_block_sum2(double& a, double& b, double (&s_a)[256], double (&s_b)[256]) {
    s_a[threadIdx.x] = a, s_b[threadIdx.x] = b;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) s_a[threadIdx.x] += s_a[threadIdx.x + h], s_b[threadIdx.x] += s_b[threadIdx.x + h];
        __syncthreads();
    }
    a = s_a[0], b = s_b[0];
    __syncthreads();
}

// The split of a slice: a function of HW alone.
struct ObjSplit {
    int np;    // parts per slice
    int plen;  // elements per part, a multiple of 4 (the last part: what is left)
};
static ObjSplit obj_split(int HW) {
    int np = (int)(((long)HW + OBJ_PART_ELEMS - 1) / OBJ_PART_ELEMS);
    if (np > CFD_OBJ_MAX_PARTS) np = CFD_OBJ_MAX_PARTS;
    const long per = ((long)HW + np - 1) / np;
    return ObjSplit{np, (int)((per + 3) / 4 * 4)};
}

// Elements [lo, hi) of slice `slice` as 16-byte units u = 0 .. nunit - 1 (unit u: elements lo + 4 u .. lo + 4 u + 3, clipped at hi);
// thread t owns units t, t + 256, ...  VEC: HW % 4 == 0 and every pointer on the 16-byte grid, so every unit is whole and aligned.
struct ObjRange {
    size_t base;  // first element of the slice inside a (B, Co, HW) tensor
    size_t mbase; // first element of the sample's mask row
    int lo, hi, nunit;
    __device__ __forceinline__ ObjRange(int Co, int HW, int np, int plen) {
        const unsigned part = blockIdx.x % (unsigned)np, slice = blockIdx.x / (unsigned)np;
        base = (size_t)slice * (size_t)HW;
        mbase = (size_t)(slice / (unsigned)Co) * (size_t)HW;
        lo = (int)part * plen;
        hi = lo + plen < HW ? lo + plen : HW;
        nunit = hi > lo ? (hi - lo + 3) >> 2 : 0;
    }
};
template <bool VEC>
__device__ __forceinline__ f32x4 obj_load4(const float* p, size_t first, int left, float fill) {
    if constexpr (VEC) {
        return *reinterpret_cast<const f32x4*>(p + first);
    } else {
        f32x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = j < left ? p[first + j] : fill;
        return v;
    }
}

template <bool VEC, bool MASK>
__global__ __launch_bounds__(256) void k_obj_part(const float* __restrict__ preds, const float* __restrict__ label,
                                                  const float* __restrict__ mask, float* __restrict__ parts, int Co, int HW, int np,
                                                  int plen) {
    __shared__ double s_e[256], s_s[256];
    const ObjRange r(Co, HW, np, plen);
    double e = 0.0, s = 0.0;
    for (int u0 = threadIdx.x; u0 < r.nunit; u0 += OBJ_TRIPS * 256) {
        f32x4 pv[OBJ_TRIPS], lv[OBJ_TRIPS], mv[OBJ_TRIPS];
#pragma unroll
        for (int k = 0; k < OBJ_TRIPS; ++k) {
            const int u = u0 + k * 256;
            const bool in = u < r.nunit;
            const int i = r.lo + 4 * u, left = in ? r.hi - i : 0;
            // (a unit or an element outside the part reads as 0: it adds +0.0 to both sums, which changes no bit of them)
            pv[k] = in ? obj_load4<VEC>(preds, r.base + i, left, 0.f) : f32x4{0.f, 0.f, 0.f, 0.f};
            lv[k] = in ? obj_load4<VEC>(label, r.base + i, left, 0.f) : f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (MASK) mv[k] = in ? obj_load4<VEC>(mask, r.mbase + i, left, 0.f) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < OBJ_TRIPS; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // label * mask is rounded on its own (exact for a 0/1 mask), then ONE fp32 rounding makes d
                const float lm = MASK ? cfd_opaque_f(lv[k][j] * mv[k][j]) : lv[k][j];
                const float d = pv[k][j] - lm;
                e += (double)d * (double)d;
                s += (double)lm * (double)lm;
            }
        }
    }
    obj_block_sum2(e, s, s_e, s_s);
    if (threadIdx.x == 0) {
        obj_store_f64(parts + 4 * (size_t)blockIdx.x, e);
        obj_store_f64(parts + 4 * (size_t)blockIdx.x + 2, s);
    }
}

__device__ __forceinline__ double obj_term(int kind, double e, double s) { return kind == CFD_OBJ_REL_L2 ? sqrt(e) / sqrt(s) : e / s; }

// One workgroup.  rec + 8: the groups' (E_g, S_g); `parts`: the records of k_obj_part, record (b Co + c) np + part.
__global__ __launch_bounds__(256) void k_obj_final(float* __restrict__ rec, const float* __restrict__ parts, float* __restrict__ value,
                                                   int B, int Co, int np, int kind) {
    __shared__ double s_a[256], s_b[256];
    float* grp = rec + 8;
    double v = 0.0, ge = 0.0, gs = 0.0;
    if (kind != CFD_OBJ_NMSE_CHANNEL) {
        // a sample's records lie side by side: a thread adds them in index order, then the three sums over the samples go up the tree
        const int per = Co * np;
        for (int b = threadIdx.x; b < B; b += 256) {
            double e = 0.0, s = 0.0;
            for (int q = 0; q < per; ++q) {
                const float* p = parts + 4 * ((size_t)b * per + q);
                e += obj_load_f64(p), s += obj_load_f64(p + 2);
            }
            obj_store_f64(grp + 4 * (size_t)b, e);
            obj_store_f64(grp + 4 * (size_t)b + 2, s);
            v += obj_term(kind, e, s), ge += e, gs += s;
        }
        double zero = 0.0;
        obj_block_sum2(v, zero, s_a, s_b);
        obj_block_sum2(ge, gs, s_a, s_b);
    } else {
        // a channel's records are B * np strided ones: thread-strided over the samples, then the tree; every thread holds the totals
        for (int c = 0; c < Co; ++c) {
            double e = 0.0, s = 0.0;
            for (int b = threadIdx.x; b < B; b += 256)
                for (int q = 0; q < np; ++q) {
                    const float* p = parts + 4 * (((size_t)b * Co + c) * np + q);
                    e += obj_load_f64(p), s += obj_load_f64(p + 2);
                }
            obj_block_sum2(e, s, s_a, s_b);
            if (threadIdx.x == 0) {
                obj_store_f64(grp + 4 * (size_t)c, e);
                obj_store_f64(grp + 4 * (size_t)c + 2, s);
            }
            v += obj_term(kind, e, s), ge += e, gs += s;
        }
    }
    if (threadIdx.x == 0) {
        const double val = v / (double)(kind == CFD_OBJ_NMSE_CHANNEL ? Co : B);
        obj_store_f64(rec, ge);
        obj_store_f64(rec + 2, gs);
        obj_store_f64(rec + 4, val);
        value[0] = (float)val;  // (the one rounding)
    }
}

// gpreds = gadd + fp32(coef * d) on the split of k_obj_part.  gpreds may alias gadd: no __restrict__ on the two, and a thread has loaded
// every element it owns before it stores one of them.
template <bool VEC, bool MASK, bool GADD>
__global__ __launch_bounds__(256) void k_obj_bwd(const float* __restrict__ preds, const float* __restrict__ label,
                                                 const float* __restrict__ mask, const float* __restrict__ grp, const float* gadd,
                                                 const float* __restrict__ upstream_dev, float upstream, float* gpreds, int B, int Co,
                                                 int HW, int np, int plen, int kind) {
    const ObjRange r(Co, HW, np, plen);
    const unsigned slice = blockIdx.x / (unsigned)np;
    const unsigned g = kind == CFD_OBJ_NMSE_CHANNEL ? slice % (unsigned)Co : slice / (unsigned)Co;
    const double e = obj_load_f64(grp + 4 * (size_t)g), s = obj_load_f64(grp + 4 * (size_t)g + 2);
    double coef;
    if (kind == CFD_OBJ_REL_L2) coef = e == 0.0 ? 0.0 : 1.0 / ((double)B * sqrt(e) * sqrt(s));
    else coef = 2.0 / ((double)(kind == CFD_OBJ_NMSE_CHANNEL ? Co : B) * s);
    coef *= (double)upstream * (upstream_dev ? (double)upstream_dev[0] : 1.0);
    for (int u0 = threadIdx.x; u0 < r.nunit; u0 += OBJ_TRIPS * 256) {
        f32x4 pv[OBJ_TRIPS], lv[OBJ_TRIPS], mv[OBJ_TRIPS], av[OBJ_TRIPS];
#pragma unroll
        for (int k = 0; k < OBJ_TRIPS; ++k) {
            const int u = u0 + k * 256;
            if (u >= r.nunit) continue;
            const int i = r.lo + 4 * u, left = r.hi - i;
            pv[k] = obj_load4<VEC>(preds, r.base + i, left, 0.f);
            lv[k] = obj_load4<VEC>(label, r.base + i, left, 0.f);
            if constexpr (MASK) mv[k] = obj_load4<VEC>(mask, r.mbase + i, left, 0.f);
            if constexpr (GADD) av[k] = obj_load4<VEC>(gadd, r.base + i, left, 0.f);
        }
#pragma unroll
        for (int k = 0; k < OBJ_TRIPS; ++k) {
            const int u = u0 + k * 256;
            if (u >= r.nunit) continue;
            const int i = r.lo + 4 * u, left = r.hi - i;
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float lm = MASK ? cfd_opaque_f(lv[k][j] * mv[k][j]) : lv[k][j];
                const float d = pv[k][j] - lm;
                const float t = (float)(coef * (double)d);
                o[j] = GADD ? av[k][j] + t : t;
            }
            if constexpr (VEC) {
                *reinterpret_cast<f32x4*>(gpreds + r.base + i) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < left) gpreds[r.base + i + j] = o[j];
            }
        }
    }
}

// ---- host side ----
static bool obj_aligned16(std::initializer_list<const void*> bufs) {
    uintptr_t bits = 0;
    for (const void* b : bufs) bits |= (uintptr_t)b;  // (NULL adds nothing)
    return (bits & 15) == 0;
}
static int obj_check(const char* fn, int B, int Co, int HW, int kind) {
    CFD_REQUIRE(kind == CFD_OBJ_REL_L2 || kind == CFD_OBJ_NMSE_SAMPLE || kind == CFD_OBJ_NMSE_CHANNEL, CFD_ERR_INVALID_ARG,
                "%s: unknown kind %d", fn, kind);
    CFD_REQUIRE(B >= 1 && Co >= 1 && HW >= 1, CFD_ERR_INVALID_ARG, "%s: B = %d, Co = %d, HW = %d must all be >= 1", fn, B, Co, HW);
    // (one workgroup per part record: the grid's x dimension holds them, and a slice's element index stays an int)
    CFD_REQUIRE((size_t)B * (size_t)Co * CFD_OBJ_MAX_PARTS < (1ull << 31), CFD_ERR_UNSUPPORTED, "%s: B * Co = %zu slices are too many", fn,
                (size_t)B * (size_t)Co);
    CFD_REQUIRE(HW <= (1 << 30), CFD_ERR_UNSUPPORTED, "%s: HW = %d exceeds 2^30", fn, HW);
    return CFD_OK;
}

extern "C" int cfd_objective_fwd(const float* preds, const float* label, const float* mask, float* rec, float* value, int B, int Co,
                                 int HW, int kind, void* stream) {
    CFD_REQUIRE(preds && label && rec && value, CFD_ERR_INVALID_ARG, "cfd_objective_fwd: NULL pointer");
    CFD_TRY(obj_check("cfd_objective_fwd", B, Co, HW, kind));
    const ObjSplit sp = obj_split(HW);
    const unsigned nrec = (unsigned)((size_t)B * Co * sp.np);
    const size_t G = (size_t)(B > Co ? B : Co);
    float* parts = rec + 8 + 4 * G;
    const bool vec = HW % 4 == 0 && obj_aligned16({preds, label, mask});
    const double n = (double)B * Co * HW;
    {
        CFD_PROF_W("k_obj_part", (hipStream_t)stream, 8.0 * n + (mask ? 4.0 * B * HW : 0.0) + 16.0 * nrec, 4.0 * n);
        with_bools([&](auto V, auto M) {
            hipLaunchKernelGGL((k_obj_part<CFD_B(V), CFD_B(M)>), dim3(nrec), dim3(256), 0, (hipStream_t)stream, preds, label, mask, parts,
                               Co, HW, sp.np, sp.plen);
        }, vec, mask != nullptr);
        CFD_LAUNCH_CHECK("cfd_objective_fwd");
    }
    CFD_PROF_W("k_obj_final", (hipStream_t)stream, 16.0 * nrec + 16.0 * G + 28.0, 2.0 * nrec);
    hipLaunchKernelGGL(k_obj_final, dim3(1), dim3(256), 0, (hipStream_t)stream, rec, parts, value, B, Co, sp.np, kind);
    CFD_LAUNCH_CHECK("cfd_objective_fwd");
    return CFD_OK;
}

extern "C" int cfd_objective_bwd(const float* preds, const float* label, const float* mask, const float* rec, const float* gadd,
                                 const float* upstream_dev, float upstream, float* gpreds, int B, int Co, int HW, int kind,
                                 void* stream) {
    CFD_REQUIRE(preds && label && rec && gpreds, CFD_ERR_INVALID_ARG, "cfd_objective_bwd: NULL pointer");
    CFD_TRY(obj_check("cfd_objective_bwd", B, Co, HW, kind));
    const ObjSplit sp = obj_split(HW);
    const unsigned nrec = (unsigned)((size_t)B * Co * sp.np);
    const bool vec = HW % 4 == 0 && obj_aligned16({preds, label, mask, gadd, gpreds});
    const double n = (double)B * Co * HW;
    // read preds, label (and gadd), the mask row once per sample; write gpreds
    CFD_PROF_W("k_obj_bwd", (hipStream_t)stream, (gadd ? 16.0 : 12.0) * n + (mask ? 4.0 * B * HW : 0.0), 3.0 * n);
    with_bools([&](auto V, auto M, auto A) {
        hipLaunchKernelGGL((k_obj_bwd<CFD_B(V), CFD_B(M), CFD_B(A)>), dim3(nrec), dim3(256), 0, (hipStream_t)stream, preds, label, mask,
                           rec + 8, gadd, upstream_dev, upstream, gpreds, B, Co, HW, sp.np, sp.plen, kind);
    }, vec, mask != nullptr, gadd != nullptr);
    CFD_LAUNCH_CHECK("cfd_objective_bwd");
    return CFD_OK;
}
