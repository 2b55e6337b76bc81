// The optimiser launches: flat Adam / AdamW, gradient accumulation, the gradient norm of clipping, the multi-tensor step.
//   torch.optim.Adam          src/train_auto.py:213,256            -> k_adam / k_adam_f / k_adam_multi
// One walk over the flat buffer (flat_walk), one block that finishes a row of fc0's gradient (stem_row); what happens to an element is an
// operation struct: AdamOp, AccumOp, SumSqOp.
#include <initializer_list>

#include "cfd_common.h"
#include "cfd_launch.h"
#include "cfd_tail.h"

// ------------------------------------------------------------------------------------------------------
// Adam  (torch.optim.Adam defaults: amsgrad=False, maximize=False; train_auto.py:213)
// ------------------------------------------------------------------------------------------------------
// DW (CFD_STEP_DECOUPLED_WD of cfd_fno_adam_step; torch.optim.AdamW's single-tensor path): `wd` carries the factor 1 - lr * weight_decay
// (formed on the host in double, rounded to fp32) and the parameter is multiplied by it before the update; the gradient stays undecayed.
// The product and the scaled gradient are made opaque so that each is rounded on its own and what follows contracts exactly as it does
// without DW: a factor of 1 (weight_decay = 0) then gives the bits of plain Adam, with any gradient scale.
template <bool DW = false>
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd,
                                            float bc1, float rsqrt_bc2, float gscale) {
    float gi = g * gscale;
    if constexpr (DW) {
        gi = cfd_opaque_f(gi);  // (rounded on its own, as the select on wd below leaves it: not contracted into gi - m)
        p = cfd_opaque_f(p * wd);
    } else {
        if (wd != 0.f) gi = fmaf(wd, p, gi);
    }
    m = fmaf(1.f - b1, gi - m, m);                 // m.lerp_(g, 1-b1)
    v = fmaf(b2, v, (1.f - b2) * gi * gi);         // v.mul_(b2).addcmul_(g, g, 1-b2)
    const float denom = sqrtf(v) * rsqrt_bc2 + eps;  // sqrt(v)/sqrt(bc2) + eps
    p = p - (lr / bc1) * (m / denom);
}

// The flat walk.  A workgroup c < njob finishes row c of the lifting layer (stem_row); the others walk the flat buffer thread-strided and
// skip that layer's two ranges.  An operation has one(i, gv): element i, whose gradient is gv; and four(i): the 16-byte unit i, i.e.
// elements 4 i .. 4 i + 3 of every buffer it touches.
struct JobRanges {  // fc0.weight [jw0, jw1) and fc0.bias [jb0, jb1) inside the flat buffer; njob = 0 (no job, or an empty one): nothing to skip
    int njob, F;
    size_t jw0, jw1, jb0, jb1;
    __device__ __forceinline__ explicit JobRanges(const StemAdamJob& job = StemAdamJob{})
        : njob(job.part ? job.C : 0), F(job.in_chan + 3 + job.P), jw0((size_t)job.w_off), jw1(jw0 + (size_t)job.C * F),
          jb0((size_t)job.b_off), jb1(jb0 + job.C) {}
    __device__ __forceinline__ bool mine(size_t e) const { return !(njob && ((e >= jw0 && e < jw1) || (e >= jb0 && e < jb1))); }
    // a 16-byte unit that touches the lifting layer's ranges: it goes element by element
    __device__ __forceinline__ bool edge(size_t unit) const {
        const size_t jlo = jw0 < jb0 ? jw0 : jb0, jhi = jw1 > jb1 ? jw1 : jb1;
        return njob && 4 * unit < jhi && 4 * unit + 4 > jlo;
    }
    // this thread's first index and the stride, over the workgroups behind the job's.  bdim = blockDim.x as the KERNEL reads it: only a read
    // in the kernel's own body is folded into a scalar load of the launch's size
    __device__ __forceinline__ size_t t0(unsigned bdim) const { return (size_t)(blockIdx.x - njob) * bdim + threadIdx.x; }
    __device__ __forceinline__ size_t nt(unsigned bdim) const { return (size_t)(gridDim.x - njob) * bdim; }
};

// Workgroup blockIdx.x < r.njob: row c of the lifting layer's gradient from the sum records of k_block<.., STEMG>, stored into g (in the
// same, still unscaled units as every other gradient), then the operation on each of its F + 1 elements.
template <typename Op>
__device__ __forceinline__ void stem_row(float* __restrict__ g, const StemAdamJob& job, const JobRanges& r,
                                         float (&s_r)[CFD_STEMG_NA][256], Op& op) {
    const int c = blockIdx.x;
    stem_combine_channel(job.part, job.nrec, job.spl, job.cp, job.P, job.C, c, s_r);
    if ((int)threadIdx.x <= r.F) {
        const bool bias = (int)threadIdx.x == r.F;
        const float gv = bias ? s_r[0][0] : s_r[stem_feature_slot(threadIdx.x, job.in_chan)][0];
        const size_t i = bias ? (size_t)job.b_off + c : (size_t)job.w_off + (size_t)c * r.F + threadIdx.x;
        g[i] = gv;
        op.one(i, gv);
    }
}

// elements [first, n) one by one
template <typename Op>
__device__ __forceinline__ void flat_tail(const float* __restrict__ g, size_t first, size_t n, const JobRanges& r, unsigned bdim, Op& op) {
    const size_t nt = r.nt(bdim);
    for (size_t i = first + r.t0(bdim); i < n; i += nt)
        if (r.mine(i)) op.one(i, g[i]);
}
// VEC: every buffer is 16-byte aligned -- a thread owns four consecutive elements per trip (one 16-byte load per buffer: the flat buffer
// of the FNO engine, 926 k elements, is ONE trip of 905 workgroups instead of two trips of 2048); the last n % 4 elements go to the first
// threads of the grid one by one.
template <bool VEC, typename Op>
__device__ __forceinline__ void flat_walk(const float* __restrict__ g, size_t n, const JobRanges& r, unsigned bdim, Op& op) {
    if constexpr (VEC) {
        const size_t n4 = n >> 2, nt = r.nt(bdim);
        for (size_t i = r.t0(bdim); i < n4; i += nt) {
            if (r.edge(i)) {
                for (size_t e = 4 * i; e < 4 * i + 4; ++e)
                    if (r.mine(e)) op.one(e, g[e]);
                continue;
            }
            op.four(i);
        }
        flat_tail(g, 4 * n4, n, r, bdim, op);
    } else {
        flat_tail(g, 0, n, r, bdim, op);
    }
}

// EMA (cfd_fno_adam_step_ema): an exponential moving average of the parameters, updated while the new parameter is still in a register --
// ema[i] = fmaf(d, ema[i], (1 - d) * p_new), the ema.mul_(d).add_(p, alpha = 1 - d) of timm and diffusers.  The product is made opaque so
// that it is rounded on its own: d = 0 then gives ema[i] == p_new bit for bit for any finite ema[i] (but for the sign of a zero: 0 * e + -0 is +0).  8 more bytes per element, no launch.
template <bool EMA>
struct EmaPart {};
template <>
struct EmaPart<true> {
    float* __restrict__ ema;
    float decay;
};
template <bool EMA>
__device__ __forceinline__ float ema_update(const EmaPart<EMA>& a, float e, float p) {
    return fmaf(a.decay, e, cfd_opaque_f((1.f - a.decay) * p));
}

template <bool DW, bool EMA = false>
struct AdamOp {
    float* __restrict__ p;
    const float* __restrict__ g;
    float *__restrict__ m, *__restrict__ v;
    float lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale;
    EmaPart<EMA> a;  // (empty without EMA)
    template <typename I>  // (I: size_t on the flat buffer, unsigned in k_adam_multi)
    __device__ __forceinline__ void one(I i, float gv) const {
        adam_update<DW>(p[i], gv, m[i], v[i], lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale);
        if constexpr (EMA) a.ema[i] = ema_update(a, a.ema[i], p[i]);
    }
    template <typename I>
    __device__ __forceinline__ void four(I i) const {
        f32x4 pi = reinterpret_cast<const f32x4*>(p)[i], mi = reinterpret_cast<const f32x4*>(m)[i], vi = reinterpret_cast<const f32x4*>(v)[i];
        const f32x4 gi = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 ei;
        if constexpr (EMA) ei = reinterpret_cast<const f32x4*>(a.ema)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float pj = pi[j], mj = mi[j], vj = vi[j];
            adam_update<DW>(pj, gi[j], mj, vj, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale);
            pi[j] = pj, mi[j] = mj, vi[j] = vj;
            if constexpr (EMA) ei[j] = ema_update(a, ei[j], pj);
        }
        reinterpret_cast<f32x4*>(m)[i] = mi;
        reinterpret_cast<f32x4*>(v)[i] = vi;
        reinterpret_cast<f32x4*>(p)[i] = pi;
        if constexpr (EMA) reinterpret_cast<f32x4*>(a.ema)[i] = ei;
    }
};
// acc[i] = s * g[i] (INIT: the previous contents are never loaded) or fmaf(s, g[i], acc[i])
template <bool INIT>
struct AccumOp {
    float* __restrict__ acc;
    const float* __restrict__ g;
    float gscale;
    __device__ __forceinline__ float add(float a, float gv) const { return INIT ? gscale * gv : fmaf(gscale, gv, a); }
    __device__ __forceinline__ void one(size_t i, float gv) const { acc[i] = add(INIT ? 0.f : acc[i], gv); }
    __device__ __forceinline__ void four(size_t i) const {
        const f32x4 gi = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 ai = INIT ? f32x4{0.f, 0.f, 0.f, 0.f} : reinterpret_cast<const f32x4*>(acc)[i];
#pragma unroll
        for (int j = 0; j < 4; ++j) ai[j] = add(ai[j], gi[j]);
        reinterpret_cast<f32x4*>(acc)[i] = ai;
    }
};
struct SumSqOp {  // (k_gradsq walks its 16-byte units itself: no four)
    double acc = 0.0;
    __device__ __forceinline__ void one(size_t, float gv) { acc += (double)gv * gv; }
};

// the data-parallel step's optimiser call (cfd_adam_flat): the walk with no job -- no LDS, nothing in front of the first load
template <bool VEC>
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, size_t n, float lr, float b1, float b2, float eps,
                                              float wd, float bc1, float rsqrt_bc2, float gscale) {
    const AdamOp<false> op{p, g, m, v, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale};
    flat_walk<VEC>(g, n, JobRanges(), blockDim.x, op);
}

// ------------------------------------------------------------------------------------------------------
// Global gradient-norm clipping of the fused training step (cfd_fno_params.clip, ABI 604; torch.nn.utils.clip_grad_norm_, norm_type 2).
// The gradient is final only inside the optimiser launch (CFD_TRAIN_DEFER_*: the nMSE normaliser is a factor Adam applies, the fc0 rows
// are finished by Adam's workgroups), so the norm is taken there: k_gradsq carries the lifting layer's job instead of k_adam_f and sums
// squares in fp64, one record per workgroup; k_adam_f adds the records up (every workgroup the same few hundred doubles in the same
// order, so the same coefficient) and multiplies it into the gradient scale.  No atomics: two calls give the same bits.
// ------------------------------------------------------------------------------------------------------
// (a record is an fp64 stored as two 32-bit words: the clip buffer is a float buffer on any 4-byte boundary)
__device__ __forceinline__ void clip_store_f64(float* q, double d) {
    unsigned long long u;
    __builtin_memcpy(&u, &d, 8);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    __builtin_memcpy(q, &lo, 4);
    __builtin_memcpy(q + 1, &hi, 4);
}
__device__ __forceinline__ double clip_load_f64(const float* q) {
    unsigned lo, hi;
    __builtin_memcpy(&lo, q, 4);
    __builtin_memcpy(&hi, q + 1, 4);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}
// sum over the 256 threads of a workgroup, fixed tree; every thread calls it and gets the total
__device__ __forceinline__ double clip_block_sum(double a, double (&s_sq)[256]) {
    s_sq[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) s_sq[threadIdx.x] += s_sq[threadIdx.x + h];
        __syncthreads();
    }
    return s_sq[0];
}
__device__ __forceinline__ double clip_total_sq(const float* __restrict__ buf, int nrec, double (&s_sq)[256]) {
    double a = 0.0;
    for (int r = threadIdx.x; r < nrec; r += 256) a += clip_load_f64(buf + 2 + 2 * r);
    return clip_block_sum(a, s_sq);
}

// Workgroup c < job.C: row c of the lifting layer's gradient (what k_adam_f's workgroup c does without clipping, minus Adam) and the sum
// of its squares; the other workgroups: the squares of the flat gradient buffer outside the lifting layer's two ranges, thread-strided,
// four independent loads per thread and trip (its own loop over the 16-byte units: LABNOTES "Gradient clipping").  Record blockIdx.x of
// clip[2..] = this workgroup's sum.
template <bool VEC>
__global__ __launch_bounds__(256) void k_gradsq(float* __restrict__ g, size_t n, float* __restrict__ clip, const StemAdamJob job) {
    __shared__ float s_r[CFD_STEMG_NA][256];
    __shared__ double s_sq[256];
    const JobRanges r(job);
    SumSqOp op;
    if ((int)blockIdx.x < r.njob) {
        stem_row(g, job, r, s_r, op);
    } else if constexpr (VEC) {
        const size_t n4 = n >> 2, nt = r.nt(blockDim.x);
        for (size_t i0 = r.t0(blockDim.x); i0 < n4; i0 += 4 * nt) {
            f32x4 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t i = i0 + u * nt;
                x[u] = i < n4 ? reinterpret_cast<const f32x4*>(g)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t i = i0 + u * nt;
                const bool edge = r.edge(i);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (!edge || r.mine(4 * i + j)) op.one(4 * i + j, x[u][j]);
            }
        }
        flat_tail(g, 4 * n4, n, r, blockDim.x, op);
    } else {
        flat_walk<false>(g, n, r, blockDim.x, op);
    }
    const double tot = clip_block_sum(op.acc, s_sq);
    if (threadIdx.x == 0) clip_store_f64(clip + 2 + 2 * blockIdx.x, tot);
}

// Round 6, the fused training step's optimiser launch (cfd_fno_adam_step): the flat Adam above PLUS the work that used to be launches of
// its own in front of it -- (a) the nMSE normaliser: the head ran with the mse coefficient upstream / n, so every gradient still lacks the
// factor n / sum (label*mask)^2 = sums[3] / sums[2] (both left by the head's reduction; k_label_energy_part + _coef: two launches, 10 us);
// (b) the lifting layer's gradient: workgroup c < job.C finishes row c of fc0 from the sum records of k_block<.., STEMG>, stores it (in
// the same, still unscaled units as every other gradient) and applies Adam to it; the flat part skips those two ranges.
// DW: decoupled weight decay (adam_update<true>: the `wd` argument is the factor 1 - lr * weight_decay).
// GUARD (CFD_STEP_SKIP_NONFINITE; the launcher sets it only with clip.buf != NULL): a norm that is not finite -- a NaN or an inf in the
// gradient, an overflowing sum, an inf or NaN normaliser, a NaN grad_scale -- makes the launch a SKIPPED STEP.  Every workgroup has added
// up the same records in the same order, so the test is uniform across the grid and each returns before it has loaded an element of
// p, m or v.  The thread that stores clip[0..1] keeps the two counters at the buffer's end (plain load, add, store: no other thread of the
// launch and no record of k_gradsq reaches them).  n == 0 is no step at all: the counters stay.
// EMA (cfd_fno_adam_step_ema with ema != NULL): AdamOp<DW, true> on both paths, the flat walk and the job's rows; a skipped step has
// returned before any element is loaded, so the average keeps its bits with the parameters.  Without EMA `ea` is an empty struct.
template <bool VEC, bool DW = false, bool GUARD = false, bool EMA = false>
__global__ __launch_bounds__(256) void k_adam_f(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                size_t n, float lr, float b1, float b2, float eps, float wd, float bc1, float rsqrt_bc2,
                                                float gscale, const float* __restrict__ sums, const StemAdamJob job, const ClipArgs clip,
                                                const EmaPart<EMA> ea) {
    __shared__ float s_r[CFD_STEMG_NA][256];
    __shared__ double s_sq[256];
    if (sums) gscale *= sums[3] / sums[2];
    if (clip.buf) {  // (uniform; NULL = the launch of ABI 603: nothing is loaded before the first element)
        const double sq = clip_total_sq(clip.buf, clip.nrec, s_sq);
        const double norm = fabs((double)gscale) * sqrt(sq);
        const double coef = n ? fmin(1.0, (double)clip.max_norm / (norm + 1e-6)) : 1.0;
        if constexpr (GUARD) {
            const bool skip = n && !__builtin_isfinite(norm);  // (the build has no fast-math flag: the test is not folded away)
            if (blockIdx.x == 0 && threadIdx.x == 0) {
                clip.buf[0] = (float)norm, clip.buf[1] = skip ? 0.f : (float)coef;
                if (skip) {
                    clip.buf[CFD_CLIP_SKIPPED] += 1.f;
                    clip.buf[CFD_CLIP_CONSECUTIVE] += 1.f;
                } else if (n) {
                    clip.buf[CFD_CLIP_CONSECUTIVE] = 0.f;
                }
            }
            if (skip) return;
        } else {
            if (blockIdx.x == 0 && threadIdx.x == 0) clip.buf[0] = (float)norm, clip.buf[1] = (float)coef;
        }
        gscale *= (float)coef;  // (coef == 1: the same bits as without clipping)
    }
    const JobRanges r(job);
    const AdamOp<DW, EMA> op{p, g, m, v, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale, ea};
    if ((int)blockIdx.x < r.njob) stem_row(g, job, r, s_r, op);
    else flat_walk<VEC>(g, n, r, blockDim.x, op);
}

// Gradient accumulation over micro-batches (CFD_STEP_ACCUMULATE of cfd_fno_adam_step): the optimiser launch's place in a pass that is not
// the group's last.  It finishes the pass's gradient exactly as k_adam_f does -- the deferred normaliser in the scale, workgroup c < job.C
// the lifting layer's row c, stored into g in the pass's unscaled units -- and its update rule is AccumOp<INIT>.  One thread writes each
// element, no atomics: two calls give the same bits.  12 bytes per element, 8 with INIT; grid capped like Adam's.
template <bool VEC, bool INIT>
__global__ __launch_bounds__(256) void k_grad_accum(float* __restrict__ acc, float* __restrict__ g, size_t n, float gscale,
                                                    const float* __restrict__ sums, const StemAdamJob job) {
    __shared__ float s_r[CFD_STEMG_NA][256];
    if (sums) gscale *= sums[3] / sums[2];
    const JobRanges r(job);
    const AccumOp<INIT> op{acc, g, gscale};
    if ((int)blockIdx.x < r.njob) stem_row(g, job, r, s_r, op);
    else flat_walk<VEC>(g, n, r, blockDim.x, op);
}

// ---- host side ----
// VEC needs every buffer on a 16-byte boundary and one whole unit; ONE trip per thread up to 2048 workgroups (beyond: several trips)
#define CFD_FLAT_MAX_BLOCKS 2048u
struct FlatGrid { bool vec; unsigned blocks; };  // (blocks = 0 when n == 0)
static FlatGrid flat_grid(size_t n, std::initializer_list<const void*> bufs) {
    uintptr_t bits = 0;
    for (const void* b : bufs) bits |= (uintptr_t)b;
    const bool vec = (bits & 15) == 0 && n >= 4;
    const size_t blocks = ((vec ? n / 4 : n) + 255) / 256;
    return FlatGrid{vec, blocks > CFD_FLAT_MAX_BLOCKS ? CFD_FLAT_MAX_BLOCKS : (unsigned)blocks};
}
// the job by value (NULL: none), refused where stem_combine_channel / stem_row cannot run it
static int checked_job(const StemAdamJob* job, StemAdamJob& jb) {
    jb = job ? *job : StemAdamJob{};
    CFD_REQUIRE(!jb.part || (jb.P <= 8 && jb.in_chan + 3 + jb.P < 256), CFD_ERR_UNSUPPORTED, "cfd_fno_adam_step: lifting layer with %d case parameters", jb.P);
    return CFD_OK;
}

int cfd_int_adam_flat_f(float* param, float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr, float beta1, float beta2,
                        float eps, float weight_decay, int step, float grad_scale, const float* sums, const StemAdamJob* job, float* clip,
                        float max_grad_norm, int decoupled, int guard, float* ema, float ema_decay, void* stream) {
    CFD_REQUIRE(param && grad && exp_avg && exp_avg_sq, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: NULL pointer");
    CFD_REQUIRE(!guard || clip, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: CFD_STEP_SKIP_NONFINITE needs grads->clip");
    CFD_REQUIRE(step >= 1, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: step must be >= 1");
    CFD_REQUIRE(!clip || max_grad_norm > 0.f, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: max_grad_norm must be > 0 (+inf: measure only)");
    if (n == 0 && !clip) return CFD_OK;
    StemAdamJob jb;
    CFD_TRY(checked_job(job, jb));
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    // k_gradsq does not touch the average: its form and its records are those of the call without `ema` (fg0), so the clip buffer is that
    // call's bit for bit wherever the average lies; Adam's launch takes the average's pointer into its alignment test (fg)
    const FlatGrid fg0 = flat_grid(n, {param, grad, exp_avg, exp_avg_sq});
    const FlatGrid fg = ema ? flat_grid(n, {param, grad, exp_avg, exp_avg_sq, ema}) : fg0;
    unsigned blocks = fg.blocks;
    ClipArgs ca{};
    if (clip) {  // the norm needs the finished fc0 rows: k_gradsq takes the job, Adam's launch runs the flat update alone
        const int njob = jb.part ? jb.C : 0;
        // (with the guard the last two floats are its counters: the records must end in front of them)
        CFD_REQUIRE(2 + 2 * (njob + CFD_CLIP_MAX_WGS) <= CFD_CLIP_FLOATS - (guard ? 2 : 0), CFD_ERR_UNSUPPORTED,
                    "cfd_fno_adam_step: clipping with a lifting layer of %d channels", njob);
        const unsigned gsq = fg0.blocks < CFD_CLIP_MAX_WGS ? fg0.blocks : (unsigned)CFD_CLIP_MAX_WGS;  // (n == 0: none)
        ca = ClipArgs{clip, max_grad_norm, (int)gsq + njob};
        if (ca.nrec > 0) {
            CFD_PROF_W("k_gradsq", (hipStream_t)stream, 4.0 * n, 2.0 * n);
            with_bools([&](auto V) {
                hipLaunchKernelGGL(k_gradsq<CFD_B(V)>, dim3((unsigned)ca.nrec), dim3(256), 0, (hipStream_t)stream, grad, n, clip, jb);
            }, fg0.vec);
            CFD_LAUNCH_CHECK("cfd_fno_adam_step");
        }
        jb = StemAdamJob{};
        if (blocks == 0) blocks = 1;  // (n == 0: one workgroup stores clip[0] = 0, clip[1] = 1)
    }
    blocks += jb.part ? jb.C : 0;
    CFD_PROF_W("k_adam", (hipStream_t)stream, (ema ? 36.0 : 28.0) * n, (ema ? 14.0 : 12.0) * n);  // read p, g, m, v; write p, m, v; the average both ways
    const float rbc1 = (float)bc1, rbc2 = (float)(1.0 / sqrt(bc2));
    // AdamW: p *= 1 - lr * wd (the factor in double, rounded once, as torch forms it), then Adam on the undecayed gradient
    const float wdarg = decoupled ? (float)(1.0 - (double)lr * (double)weight_decay) : weight_decay;
    // (guard: the variants that can skip the step: clip != NULL was required above)
    with_bools([&](auto V, auto D, auto G, auto E) {
        EmaPart<CFD_B(E)> ea{};
        if constexpr (CFD_B(E)) ea = EmaPart<true>{ema, ema_decay};
        hipLaunchKernelGGL((k_adam_f<CFD_B(V), CFD_B(D), CFD_B(G), CFD_B(E)>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, param, grad,
                           exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, wdarg, rbc1, rbc2, grad_scale, sums, jb, ca, ea);
    }, fg.vec, decoupled != 0, guard != 0, ema != nullptr);
    CFD_LAUNCH_CHECK("cfd_fno_adam_step");
    return CFD_OK;
}

int cfd_int_grad_accum_f(float* acc, float* grad, size_t n, float grad_scale, const float* sums, const StemAdamJob* job, int init,
                         void* stream) {
    CFD_REQUIRE(acc && grad, CFD_ERR_INVALID_ARG, "cfd_fno_adam_step: NULL pointer");
    if (n == 0) return CFD_OK;
    StemAdamJob jb;
    CFD_TRY(checked_job(job, jb));
    const FlatGrid fg = flat_grid(n, {acc, grad});
    const unsigned blocks = fg.blocks + (jb.part ? jb.C : 0);
    CFD_PROF_W("k_grad_accum", (hipStream_t)stream, (init ? 8.0 : 12.0) * n, 2.0 * n);  // read g (and acc); write acc
    with_bools([&](auto V, auto I) {
        hipLaunchKernelGGL((k_grad_accum<CFD_B(V), CFD_B(I)>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, acc, grad, n, grad_scale,
                           sums, jb);
    }, fg.vec, init != 0);
    CFD_LAUNCH_CHECK("cfd_fno_adam_step");
    return CFD_OK;
}

extern "C" int cfd_adam_flat(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                             float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                             void* stream) {
    CFD_REQUIRE(param && grad && exp_avg && exp_avg_sq, CFD_ERR_INVALID_ARG, "cfd_adam_flat: NULL pointer");
    CFD_REQUIRE(step >= 1, CFD_ERR_INVALID_ARG, "cfd_adam_flat: step must be >= 1");
    if (n == 0) return CFD_OK;
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const FlatGrid fg = flat_grid(n, {param, grad, exp_avg, exp_avg_sq});
    CFD_PROF_W("k_adam", (hipStream_t)stream, 28.0 * n, 12.0 * n);  // read p, g, m, v; write p, m, v
    with_bools([&](auto V) {
        hipLaunchKernelGGL(k_adam<CFD_B(V)>, dim3(fg.blocks), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, lr,
                           beta1, beta2, eps, weight_decay, (float)bc1, (float)(1.0 / sqrt(bc2)), grad_scale);
    }, fg.vec);
    CFD_LAUNCH_CHECK("cfd_adam_flat");
    return CFD_OK;
}

// ------------------------------------------------------------------------------------------------------
// The same step for MANY parameter tensors in one launch (the autograd training paths of the U-Net / ResNet / DeepONet families keep
// torch's per-tensor parameters: 136 / 28 / 33 tensors).  torch's fused multi-tensor Adam took 3 x 31 us for the U-Net's 4.4 MB and
// 40 us for the Auto-DeepONet's 2.3 MB -- 7 % of that model's step.  The (p, g, m, v, n) table travels as the kernel argument;
// workgroups [blk0, blk0 + nblk) belong to item i.  Learning rate and step count come from device scalars when given (a captured
// HIP graph replays with the values of the moment), bias corrections are formed in fp32 like torch's capturable path.
// ------------------------------------------------------------------------------------------------------
#define CFD_ADAM_MAX 80
struct AdamItem { float* p; const float* g; float* m; float* v; unsigned n, blk0; };
struct AdamBatch { int n; AdamItem it[CFD_ADAM_MAX]; };
// this workgroup's item: the last one whose first workgroup is <= blockIdx.x.  Bisection -- seven dependent scalar loads of the
// kernel-argument table at most; the linear walk of rounds 3-4 cost the last items' workgroups up to 79 of them
template <typename Batch>
__device__ __forceinline__ int batch_item(const Batch& b) {
    int i = 0, hi = b.n;
    while (hi - i > 1) {
        const int mid = (i + hi) >> 1;
        if (blockIdx.x >= b.it[mid].blk0) i = mid;
        else hi = mid;
    }
    return i;
}

__global__ __launch_bounds__(256) void k_adam_multi(const AdamBatch b, const float* __restrict__ lr_dev, float lr,
                                                    const float* __restrict__ step_dev, float step, float b1, float b2, float eps,
                                                    float wd, float gscale) {
    const int i = batch_item(b);
    const AdamItem& e = b.it[i];
    const unsigned nblk = (i + 1 < b.n ? b.it[i + 1].blk0 : gridDim.x) - e.blk0;
    if (lr_dev) lr = lr_dev[0];
    if (step_dev) step = step_dev[0];
    // the bias corrections once per workgroup (wave 0), not once per wave: two powf are ~300 VALU instructions, and with one element per
    // thread they were most of the kernel's issue time
    __shared__ float s_bc[2];
    if (threadIdx.x < 64) {
        const float c1 = 1.f - powf(b1, step), c2 = 1.f / sqrtf(1.f - powf(b2, step));
        if (threadIdx.x == 0) s_bc[0] = c1, s_bc[1] = c2;
    }
    __syncthreads();
    const AdamOp<false> op{e.p, e.g, e.m, e.v, lr, b1, b2, eps, wd, s_bc[0], s_bc[1], gscale};
    // (bit 31 of n: the item's four buffers are 16-byte aligned -- a thread owns four consecutive elements per trip, the last n % 4
    // elements go one by one to the item's first threads)
    const unsigned n = e.n & 0x7fffffffu, t0 = (blockIdx.x - e.blk0) * blockDim.x + threadIdx.x, nt = nblk * blockDim.x;
    unsigned first = 0;
    if (e.n >> 31) {
        const unsigned n4 = n >> 2;
        for (unsigned k = t0; k < n4; k += nt) op.four(k);
        first = 4 * n4;
    }
    for (unsigned k = first + t0; k < n; k += nt) op.one(k, e.g[k]);
}

extern "C" int cfd_adam_multi(int n, float* const* param, const float* const* grad, float* const* exp_avg, float* const* exp_avg_sq,
                              const size_t* numel, const float* lr_dev, float lr, const float* step_dev, float step, float beta1,
                              float beta2, float eps, float weight_decay, float grad_scale, void* stream) {
    CFD_REQUIRE(n >= 0, CFD_ERR_INVALID_ARG, "cfd_adam_multi: negative count");
    if (n == 0) return CFD_OK;
    CFD_REQUIRE(param && grad && exp_avg && exp_avg_sq && numel, CFD_ERR_INVALID_ARG, "cfd_adam_multi: NULL table");
    CFD_REQUIRE(step_dev || step >= 1.f, CFD_ERR_INVALID_ARG, "cfd_adam_multi: step must be >= 1");
    for (int base = 0; base < n; base += CFD_ADAM_MAX) {
        AdamBatch b{};
        b.n = n - base < CFD_ADAM_MAX ? n - base : CFD_ADAM_MAX;
        unsigned blocks = 0;
        double total = 0.0;
        for (int i = 0; i < b.n; ++i) {
            const int k = base + i;
            CFD_REQUIRE(param[k] && grad[k] && exp_avg[k] && exp_avg_sq[k], CFD_ERR_INVALID_ARG, "cfd_adam_multi: NULL pointer in item %d", k);
            CFD_REQUIRE(numel[k] < (1ull << 31), CFD_ERR_UNSUPPORTED, "cfd_adam_multi: item %d has 2^31 or more elements", k);
            AdamItem& e = b.it[i];
            e.p = param[k], e.g = grad[k], e.m = exp_avg[k], e.v = exp_avg_sq[k], e.n = (unsigned)numel[k], e.blk0 = blocks;
            // ONE trip per thread up to 2048 workgroups per tensor, four elements in 16-byte units where the buffers allow: a thread that
            // walks several trips pays one memory latency per trip (the Auto-DeepONet's 430 k-element first-layer weight: 7 trips on 256
            // workgroups), and one element per thread takes more workgroups than the chip holds at once (2300 for that model: two
            // rounds of the whole latency chain -- table lookup, step / rate scalars, bias corrections, loads)
            const FlatGrid fg = flat_grid(e.n, {e.p, e.g, e.m, e.v});
            if (fg.vec) e.n |= 0x80000000u;
            blocks += fg.blocks < 1 ? 1 : fg.blocks;
            total += (double)(e.n & 0x7fffffffu);
        }
        CFD_PROF_W("k_adam", (hipStream_t)stream, 28.0 * total, 12.0 * total);
        hipLaunchKernelGGL(k_adam_multi, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b, lr_dev, lr, step_dev, step, beta1, beta2,
                           eps, weight_decay, grad_scale);
        CFD_LAUNCH_CHECK("cfd_adam_multi");
    }
    return CFD_OK;
}

// dst[k][i] = scale * src[k][i] for n tensors in one launch per 80 (the data-parallel path of the graph-replayed models packs every
// parameter gradient, pre-scaled by 1 / world, into ONE flat buffer behind the captured backward pass: graph.GraphedTrainStep;
// torch.cat + mul_ + ~136 copy_ launches per U-Net step before).  Same table walk as k_adam_multi.
struct CopyItem { const float* s; float* d; unsigned n, blk0; };
struct CopyBatch { int n; CopyItem it[CFD_ADAM_MAX]; };
__global__ __launch_bounds__(256) void k_scale_copy_multi(const CopyBatch b, float scale) {
    const int i = batch_item(b);
    const CopyItem& e = b.it[i];
    const unsigned nblk = (i + 1 < b.n ? b.it[i + 1].blk0 : gridDim.x) - e.blk0;
    for (unsigned k = (blockIdx.x - e.blk0) * blockDim.x + threadIdx.x; k < e.n; k += nblk * blockDim.x) e.d[k] = e.s[k] * scale;
}

extern "C" int cfd_scale_copy_multi(int n, const float* const* src, float* const* dst, const size_t* numel, float scale, void* stream) {
    CFD_REQUIRE(n >= 0, CFD_ERR_INVALID_ARG, "cfd_scale_copy_multi: negative count");
    if (n == 0) return CFD_OK;
    CFD_REQUIRE(src && dst && numel, CFD_ERR_INVALID_ARG, "cfd_scale_copy_multi: NULL table");
    for (int base = 0; base < n; base += CFD_ADAM_MAX) {
        CopyBatch b{};
        b.n = n - base < CFD_ADAM_MAX ? n - base : CFD_ADAM_MAX;
        unsigned blocks = 0;
        double total = 0.0;
        for (int i = 0; i < b.n; ++i) {
            const int k = base + i;
            CFD_REQUIRE(src[k] && dst[k], CFD_ERR_INVALID_ARG, "cfd_scale_copy_multi: NULL pointer in item %d", k);
            CFD_REQUIRE(numel[k] < (1ull << 31), CFD_ERR_UNSUPPORTED, "cfd_scale_copy_multi: item %d has 2^31 or more elements", k);
            CopyItem& e = b.it[i];
            e.s = src[k], e.d = dst[k], e.n = (unsigned)numel[k], e.blk0 = blocks;
            unsigned nb = (e.n + 255) / 256;  // (as cfd_adam_multi: one element per thread up to CFD_FLAT_MAX_BLOCKS workgroups per tensor)
            if (nb < 1) nb = 1;
            if (nb > CFD_FLAT_MAX_BLOCKS) nb = CFD_FLAT_MAX_BLOCKS;
            blocks += nb;
            total += (double)e.n;
        }
        CFD_PROF_W("k_scale_copy_multi", (hipStream_t)stream, 8.0 * total, total);
        hipLaunchKernelGGL(k_scale_copy_multi, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b, scale);
        CFD_LAUNCH_CHECK("cfd_scale_copy_multi");
    }
    return CFD_OK;
}
