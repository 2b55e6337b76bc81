// Sobolev (H^s) training objective of the FNO: the relative norm of the 2-D spectrum weighted by 1 + a1^2 |k|^2 + a2^2 |k|^4.
//   HsLoss     src/models/fno/utilities3.py     -> k_hs_fwd + k_hs_final (value), k_hs_bwd (d value / d preds)
// The gradient on the predictions enters the FNO's backward pass as gpreds_ext, like the objectives of objective.hip.
// Definitions, the layout of `rec` and the rounding order: include/cfdbench_amd.h, "Sobolev objective".
//
// One 256-thread workgroup per (sample, channel) image.  The half spectrum Dh[r][l], l <= W/2, of a real image is two real GEMM stages on
// the exact-fp32 matrix pipe (v_mfma_f32_16x16x4_f32; per output element segments of eight terms in k order, added in fp64: HsSum):
//   stage W   P = X (H x W) . [cos | -sin] (W x 2 Wf)                          Wf = W/2 + 1 kept columns, Re at column l, Im at Wf + l
//   stage H   Dh = (C - i S) (H x H) . (P_re + i P_im)
// and the adjoint, Re F^H of a weighted half spectrum Z, is the same two stages backwards:
//   stage H'  U = (C + i S) (H x H) . Z                 stage W'  out = [U_re | U_im] (H x 2 Wf4) . [cos ; -sin]
// A column l of the half spectrum stands for itself and -- unless l == 0 or 2 l == W -- for its mirror image (-r, W - l), whose |Dh| is the
// same: its weight is w(r, l) + w(-r, W - l), which also covers the reference's wave numbers of odd sizes (not symmetric under i -> N - i).
// Twiddles: a 1-D table of N entries per axis in LDS, formed by every workgroup ((i k) mod N in integers, sin / cos in double, one
// rounding); a lane walks it with an integer stride.  The image, P, the spectrum and U live in LDS (the spectrum overwrites the image, U
// overwrites P): nothing of the transform goes to HBM.  The weighted sums are fp64: per lane in tile order, then a fixed tree through LDS.
// No atomics; the 16-byte loads fill the same LDS image as the scalar ones, so both forms and any two calls give the same bits.
#include <initializer_list>

#include "cfd_common.h"
#include "cfd_launch.h"

#define HS_LDS_CAP 163840  // the 160 KB of a CU: static + dynamic LDS of a workgroup
#define HS_TWO_PI 6.283185307179586476925286766559

__device__ __forceinline__ void hs_store_f64(float* q, double d) {
    unsigned long long u;
    __builtin_memcpy(&u, &d, 8);
    const unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32);
    __builtin_memcpy(q, &lo, 4);
    __builtin_memcpy(q + 1, &hi, 4);
}
__device__ __forceinline__ double hs_load_f64(const float* q) {
    unsigned lo, hi;
    __builtin_memcpy(&lo, q, 4);
    __builtin_memcpy(&hi, q + 1, 4);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    double d;
    __builtin_memcpy(&d, &u, 8);
    return d;
}

// LDS pitches as in dft_many.hip: an A-operand plane reads conflict-free when pitch / 4 is odd, a B-operand plane when pitch / 16 is odd
__host__ __device__ static inline int hs_pitch_a(int n) { return (n / 4) % 2 ? n : n + 4; }
__host__ __device__ static inline int hs_pitch_b(int n) { return (n / 16) % 2 ? n : n + 16; }

struct HsDims {
    int Hp, Hk, Wk, Wq;  // H to 16 (rows of tiles), H to 4 (k of the H stages), W to 4 (k of stage W), W to 16 (columns of stage W')
    int Wf, NC;          // kept columns; 2 Wf to 16: columns of P and of the spectrum
    int Wf4, K2;         // Wf to 4; 2 Wf4: k of stage W' ([Re | pad | Im | pad])
    int LX, LT, LU;      // pitches of the image, of P / the spectrum, of U
    int tabs;            // floats of the four 1-D tables
    int regA, regB;      // floats of the two regions: image, then spectrum; P, then U
};
__host__ __device__ static inline HsDims hs_dims(int H, int W) {
    HsDims d;
    d.Hp = (H + 15) / 16 * 16, d.Hk = (H + 3) / 4 * 4, d.Wk = (W + 3) / 4 * 4, d.Wq = (W + 15) / 16 * 16;
    d.Wf = W / 2 + 1, d.NC = (2 * d.Wf + 15) / 16 * 16;
    d.Wf4 = (d.Wf + 3) / 4 * 4, d.K2 = 2 * d.Wf4;
    d.LX = hs_pitch_a(d.Wk), d.LT = hs_pitch_b(d.NC), d.LU = hs_pitch_a(d.K2);
    d.tabs = 2 * d.Wk + 2 * d.Hk;
    d.regA = d.Hp * (d.LX > d.LT ? d.LX : d.LT);
    d.regB = d.Hp * (d.LT > d.LU ? d.LT : d.LU);
    return d;
}
static size_t hs_lds_bytes(int H, int W) {
    const HsDims d = hs_dims(H, W);
    return ((size_t)d.tabs + (size_t)d.regA + (size_t)d.regB) * sizeof(float);
}
#define HS_STATIC_LDS (3 * 256 * 8)  // the reduction tree of k_hs_fwd

// the reference's wave number of index i on an axis of n points (not symmetric under i -> n - i when n is odd)
__device__ __forceinline__ int hs_wave(int i, int n) { return i < n / 2 ? i : n - i; }

// What element (row, col) of the half spectrum stands for: r = kx^2 + ky^2 of itself and, where it has a mirror image, of that.
struct HsMode {
    double n, r1, r2, q1, q2;  // multiplicity; r and r^2 of the element; r and r^2 of the mirror image (0 without one)
};
__device__ __forceinline__ HsMode hs_mode(int row, int col, int H, int W) {
    HsMode m;
    const int kx = hs_wave(row, H), ky = hs_wave(col, W);
    const int r = kx * kx + ky * ky;
    m.r1 = (double)r, m.r2 = (double)r * (double)r;
    const bool paired = !(col == 0 || 2 * col == W);
    m.n = paired ? 2.0 : 1.0, m.q1 = 0.0, m.q2 = 0.0;
    if (paired) {
        const int kxm = hs_wave(row ? H - row : 0, H), kym = hs_wave(W - col, W);
        const int q = kxm * kxm + kym * kym;
        m.q1 = (double)q, m.q2 = (double)q * (double)q;
    }
    return m;
}

struct HsLds {
    float *tcw, *tsw, *tch, *tsh;  // cos, sin (2 pi i / W), i < W; the same for H
    float *ra, *rb;
};
__device__ __forceinline__ HsLds hs_carve(float* smem, const HsDims& d) {
    HsLds s;
    s.tcw = smem, s.tsw = s.tcw + d.Wk, s.tch = s.tsw + d.Wk, s.tsh = s.tch + d.Hk;
    s.ra = smem + d.tabs, s.rb = s.ra + d.regA;
    return s;
}
__device__ __forceinline__ void hs_tables(const HsLds& s, int H, int W) {
    for (int i = threadIdx.x; i < W; i += 256) {
        const double a = HS_TWO_PI * (double)i / (double)W;
        s.tcw[i] = (float)cos(a), s.tsw[i] = (float)sin(a);
    }
    for (int i = threadIdx.x; i < H; i += 256) {
        const double a = HS_TWO_PI * (double)i / (double)H;
        s.tch[i] = (float)cos(a), s.tsh[i] = (float)sin(a);
    }
}

// The image into LDS, zero outside H x W.  WHICH 0: d = preds - label * mask (label * mask rounded on its own, then ONE fp32 rounding);
// WHICH 1: label * mask.  VEC: W % 4 == 0 and every pointer on the 16-byte grid.
template <bool VEC, bool MASK, int WHICH>
__device__ __forceinline__ void hs_stage_image(float* xs, const float* __restrict__ preds, const float* __restrict__ label,
                                               const float* __restrict__ mask, size_t base, size_t mbase, int H, int W, const HsDims& d) {
    if constexpr (VEC) {
        const int nu = d.Wk / 4;  // (= W / 4)
        for (int u = threadIdx.x; u < d.Hp * nu; u += 256) {
            const int r = u / nu, c = (u - r * nu) * 4;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (r < H) {
                const size_t at = (size_t)r * W + c;
                const f32x4 lv = *reinterpret_cast<const f32x4*>(label + base + at);
                f32x4 mv = {1.f, 1.f, 1.f, 1.f}, pv = {0.f, 0.f, 0.f, 0.f};
                if constexpr (MASK) mv = *reinterpret_cast<const f32x4*>(mask + mbase + at);
                if constexpr (WHICH == 0) pv = *reinterpret_cast<const f32x4*>(preds + base + at);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float lm = MASK ? cfd_opaque_f(lv[j] * mv[j]) : lv[j];
                    v[j] = WHICH == 0 ? pv[j] - lm : lm;
                }
            }
            *reinterpret_cast<f32x4*>(xs + r * d.LX + c) = v;
        }
    } else {
        for (int i = threadIdx.x; i < d.Hp * d.Wk; i += 256) {
            const int r = i / d.Wk, c = i - r * d.Wk;
            float v = 0.f;
            if (r < H && c < W) {
                const size_t at = (size_t)r * W + c;
                const float lm = MASK ? cfd_opaque_f(label[base + at] * mask[mbase + at]) : label[base + at];
                v = WHICH == 0 ? preds[base + at] - lm : lm;
            }
            xs[r * d.LX + c] = v;
        }
    }
}

// An output element of a stage: the matrix instruction's fp32 accumulator takes a SEGMENT of eight terms from zero (two instructions, k
// ascending), the segments are added in fp64 in k order, and the element is rounded to fp32 once.  A single fp32 chain over the whole k
// range (up to 128 terms, 256 in the complex stages) loses sqrt(k) roundings of the growing accumulator; the gradient of the head's bias,
// a cancelling sum over every pixel, then misses the fused step's tolerance.  Fixed order: the same bits on every call.
struct HsSum {
    double s[4];
    __device__ __forceinline__ HsSum() : s{0.0, 0.0, 0.0, 0.0} {}
    __device__ __forceinline__ void flush(f32x4& acc) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] += (double)acc[r];
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ f32x4 result(f32x4& acc) {
        flush(acc);
        return f32x4{(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
    }
};

// stage W: ps[x][c] = sum_y xs[x][y] T[y][c], T = [cos | -sin](2 pi l y / W); columns >= 2 Wf get a zero operand
__device__ __forceinline__ void hs_stage_w(const float* xs, float* ps, const HsLds& s, int W, const HsDims& d) {
    const int tid = threadIdx.x, wave = tid >> 6, i16 = tid & 15, k4 = (tid >> 4) & 3;
    const int nc1 = d.NC / 16, nt = (d.Hp / 16) * nc1;
    for (int t = wave; t < nt; t += 4) {
        const int x0 = (t / nc1) * 16, c0 = (t % nc1) * 16;
        const int c = c0 + i16;
        const bool imag = c >= d.Wf;
        const int l = imag ? c - d.Wf : c;
        const float* tb = imag ? s.tsw : s.tcw;
        const float sgn = c < 2 * d.Wf ? (imag ? -1.f : 1.f) : 0.f;
        const int step = (4 * l) % W;
        int idx = (k4 * l) % W;
        const float* a = xs + (x0 + i16) * d.LX + k4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        HsSum sum;
        for (int y = 0; y < d.Wk; y += 4) {
            acc = cfd_mfma16x16x4(a[y], sgn * tb[idx], acc);
            idx += step;
            idx -= idx >= W ? W : 0;
            if (y & 4) sum.flush(acc);
        }
        acc = sum.result(acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) ps[(x0 + 4 * k4 + r) * d.LT + c] = acc[r];
    }
}

// stage H, one 16 x 16 tile: Dh[r][l] = sum_x (cos - i sin)(2 pi r x / H) (P[x][l] + i P[x][Wf + l]).  Lanes of columns >= Wf read column
// Wf - 1 and lanes of rows >= H walk row 0 of the table: their results are not used.
__device__ __forceinline__ void hs_stage_h_tile(const float* ps, const HsLds& s, int H, const HsDims& d, int r0, int l0, f32x4& re, f32x4& im) {
    const int tid = threadIdx.x, i16 = tid & 15, k4 = (tid >> 4) & 3;
    const int row = r0 + i16 < H ? r0 + i16 : 0;
    const int l = l0 + i16 < d.Wf ? l0 + i16 : d.Wf - 1;
    const int step = (4 * row) % H;
    int idx = (k4 * row) % H;
    const float* br = ps + k4 * d.LT + l;
    const float* bi = br + d.Wf;
    re = f32x4{0.f, 0.f, 0.f, 0.f}, im = f32x4{0.f, 0.f, 0.f, 0.f};
    HsSum sre, sim;
    for (int x = 0; x < d.Hk; x += 4) {
        const float c = s.tch[idx], sn = s.tsh[idx], pr = br[x * d.LT], pi = bi[x * d.LT];
        re = cfd_mfma16x16x4(c, pr, re);
        re = cfd_mfma16x16x4(sn, pi, re);
        im = cfd_mfma16x16x4(c, pi, im);
        im = cfd_mfma16x16x4(-sn, pr, im);
        idx += step;
        idx -= idx >= H ? H : 0;
        sre.flush(re), sim.flush(im);  // (eight terms each: four of cos, four of sin)
    }
    re = sre.result(re), im = sim.result(im);
}

// sums of three quantities over the 256 threads on a fixed tree; every thread gets the totals
__device__ __forceinline__ void hs_block_sum3(double (&v)[3], double (&red)[3][256]) {
#pragma unroll
    for (int t = 0; t < 3; ++t) red[t][threadIdx.x] = v[t];
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) {
#pragma unroll
            for (int t = 0; t < 3; ++t) red[t][threadIdx.x] += red[t][threadIdx.x + h];
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 3; ++t) v[t] = red[t][0];
    __syncthreads();
}

// One workgroup per image: the record (E_0, E_1, E_2, S_0, S_1, S_2) of the image, fp64.
template <bool VEC, bool MASK>
__global__ __launch_bounds__(256) void k_hs_fwd(const float* __restrict__ preds, const float* __restrict__ label, const float* __restrict__ mask,
                                                float* __restrict__ recs, int Co, int H, int W) {
    CFD_DYN_SHARED(float, smem);
    __shared__ double red[3][256];
    const HsDims d = hs_dims(H, W);
    const HsLds s = hs_carve(smem, d);
    const size_t img = blockIdx.x, base = img * (size_t)H * W, mbase = (img / (unsigned)Co) * (size_t)H * W;
    const int tid = threadIdx.x, wave = tid >> 6, i16 = tid & 15, k4 = (tid >> 4) & 3;
    const int nlt = (d.Wf + 15) / 16, nt = (d.Hp / 16) * nlt;
    hs_tables(s, H, W);
    double out[6];
    for (int which = 0; which < 2; ++which) {
        if (which == 0) hs_stage_image<VEC, MASK, 0>(s.ra, preds, label, mask, base, mbase, H, W, d);
        else hs_stage_image<VEC, MASK, 1>(s.ra, preds, label, mask, base, mbase, H, W, d);
        __syncthreads();
        hs_stage_w(s.ra, s.rb, s, W, d);
        __syncthreads();
        double e[3] = {0.0, 0.0, 0.0};
        for (int t = wave; t < nt; t += 4) {
            const int r0 = (t / nlt) * 16, l0 = (t % nlt) * 16;
            f32x4 re, im;
            hs_stage_h_tile(s.rb, s, H, d, r0, l0, re, im);
            const int col = l0 + i16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 4 * k4 + r;
                if (row < H && col < d.Wf) {
                    const HsMode m = hs_mode(row, col, H, W);
                    const double p = (double)re[r] * (double)re[r] + (double)im[r] * (double)im[r];
                    e[0] += m.n * p, e[1] += (m.r1 + m.q1) * p, e[2] += (m.r2 + m.q2) * p;
                }
            }
        }
        hs_block_sum3(e, red);  // (its barriers also separate this pass's readers of P from the next pass)
        out[3 * which] = e[0], out[3 * which + 1] = e[1], out[3 * which + 2] = e[2];
    }
    if (tid == 0) {
#pragma unroll
        for (int t = 0; t < 6; ++t) hs_store_f64(recs + 12 * img + 2 * t, out[t]);
    }
}

struct HsArgs {
    int k, balanced;
    double A1, A2;  // a1^2, a2^2
};

// One workgroup.  rec: the value (fp64), then the samples' (E_0..2, S_0..2); recs: the images' records, image b Co + c.
__global__ __launch_bounds__(256) void k_hs_final(float* __restrict__ rec, const float* __restrict__ recs, float* __restrict__ value, int B,
                                                  int Co, HsArgs a) {
    __shared__ double red[3][256];
    double v[3] = {0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < B; b += 256) {
        double q[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int c = 0; c < Co; ++c) {
#pragma unroll
            for (int t = 0; t < 6; ++t) q[t] += hs_load_f64(recs + 12 * ((size_t)b * Co + c) + 2 * t);
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) hs_store_f64(rec + 2 + 12 * (size_t)b + 2 * t, q[t]);
        const double A[3] = {1.0, a.A1, a.A2};
        if (a.balanced) {
            double term = 0.0;
            for (int t = 0; t <= a.k; ++t) term += sqrt(A[t] * q[t]) / sqrt(A[t] * q[3 + t]);
            v[0] += term / (double)(a.k + 1);
        } else {
            double e = 0.0, sden = 0.0;
            for (int t = 0; t <= a.k; ++t) e += A[t] * q[t], sden += A[t] * q[3 + t];
            v[0] += sqrt(e) / sqrt(sden);
        }
    }
    hs_block_sum3(v, red);
    if (threadIdx.x == 0) {
        const double val = v[0] / (double)B;
        hs_store_f64(rec, val);
        value[0] = (float)val;  // (the one rounding)
    }
}

// One workgroup per image: gpreds = gadd + fp32(scale * Re F^H (w Dh)), w = g0 + g1 r + g2 r^2 on the element and its mirror image.
// gpreds may alias gadd: no __restrict__ on the two, and a lane reads the element it writes.
template <bool VEC, bool MASK, bool GADD>
__global__ __launch_bounds__(256) void k_hs_bwd(const float* __restrict__ preds, const float* __restrict__ label, const float* __restrict__ mask,
                                                const float* __restrict__ rec, const float* gadd, const float* __restrict__ upstream_dev,
                                                float upstream, float* gpreds, int B, int Co, int H, int W, HsArgs a) {
    CFD_DYN_SHARED(float, smem);
    const HsDims d = hs_dims(H, W);
    const HsLds s = hs_carve(smem, d);
    const size_t img = blockIdx.x, base = img * (size_t)H * W, mbase = (img / (unsigned)Co) * (size_t)H * W;
    const int tid = threadIdx.x, wave = tid >> 6, i16 = tid & 15, k4 = (tid >> 4) & 3;
    const int nlt = (d.Wf + 15) / 16, nt = (d.Hp / 16) * nlt;

    // the sample's coefficients, fp64: the filter is scale * (g[0] + g[1] r + g[2] r^2)
    // (scalars, no indexed array: the compiler keeps them in registers)
    double g1 = 0.0, g2 = 0.0, scale;
    {
        const float* sb = rec + 2 + 12 * (img / (unsigned)Co);
        const double e0 = hs_load_f64(sb), e1 = hs_load_f64(sb + 2), e2 = hs_load_f64(sb + 4);
        const double s0 = hs_load_f64(sb + 6), s1 = hs_load_f64(sb + 8), s2 = hs_load_f64(sb + 10);
        if (a.balanced) {
            const double den = (double)B * (double)(a.k + 1);
            scale = e0 == 0.0 ? 0.0 : 1.0 / (den * sqrt(e0) * sqrt(s0));
            g1 = (e1 == 0.0 || scale == 0.0) ? 0.0 : (1.0 / (den * sqrt(e1) * sqrt(s1))) / scale;
            if (a.k >= 2) g2 = (e2 == 0.0 || scale == 0.0) ? 0.0 : (1.0 / (den * sqrt(e2) * sqrt(s2))) / scale;
        } else {
            double e = e0 + a.A1 * e1, sden = s0 + a.A1 * s1;
            g1 = a.A1;
            if (a.k >= 2) e += a.A2 * e2, sden += a.A2 * s2, g2 = a.A2;
            scale = e == 0.0 ? 0.0 : 1.0 / ((double)B * sqrt(e) * sqrt(sden));
        }
        scale *= (double)upstream * (upstream_dev ? (double)upstream_dev[0] : 1.0);
    }

    hs_tables(s, H, W);
    hs_stage_image<VEC, MASK, 0>(s.ra, preds, label, mask, base, mbase, H, W, d);
    __syncthreads();
    hs_stage_w(s.ra, s.rb, s, W, d);
    __syncthreads();
    // stage H into the image's region: Z = fp32(w Dh), zero in the rows >= H (the k padding of stage H')
    float* zs = s.ra;
    for (int t = wave; t < nt; t += 4) {
        const int r0 = (t / nlt) * 16, l0 = (t % nlt) * 16;
        f32x4 re, im;
        hs_stage_h_tile(s.rb, s, H, d, r0, l0, re, im);
        const int col = l0 + i16;
        if (col < d.Wf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = r0 + 4 * k4 + r;
                float zr = 0.f, zi = 0.f;
                if (row < H) {
                    const HsMode m = hs_mode(row, col, H, W);
                    const double w = (1.0 + g1 * m.r1 + g2 * m.r2) + (m.n == 2.0 ? 1.0 + g1 * m.q1 + g2 * m.q2 : 0.0);
                    zr = (float)(w * (double)re[r]), zi = (float)(w * (double)im[r]);
                }
                zs[row * d.LT + col] = zr;
                zs[row * d.LT + d.Wf + col] = zi;
            }
        }
    }
    __syncthreads();
    // stage H': U[x][l] = sum_r (cos + i sin)(2 pi r x / H) Z[r][l]; Re at column l, Im at Wf4 + l, zero in the padding columns
    float* us = s.rb;
    for (int i = tid; i < d.Hp * 2 * (d.Wf4 - d.Wf); i += 256) {
        const int np = d.Wf4 - d.Wf, x = i / (2 * np), j = i - x * 2 * np;
        us[x * d.LU + (j < np ? d.Wf + j : d.Wf4 + d.Wf + j - np)] = 0.f;
    }
    for (int t = wave; t < nt; t += 4) {
        const int x0 = (t / nlt) * 16, l0 = (t % nlt) * 16;
        const int x = x0 + i16 < H ? x0 + i16 : 0;
        const int l = l0 + i16 < d.Wf ? l0 + i16 : d.Wf - 1;
        const int step = (4 * x) % H;
        int idx = (k4 * x) % H;
        const float* bzr = zs + k4 * d.LT + l;
        const float* bzi = bzr + d.Wf;
        f32x4 ur = {0.f, 0.f, 0.f, 0.f}, ui = {0.f, 0.f, 0.f, 0.f};
        HsSum sur, sui;
        for (int r = 0; r < d.Hk; r += 4) {
            const float c = s.tch[idx], sn = s.tsh[idx], zr = bzr[r * d.LT], zi = bzi[r * d.LT];
            ur = cfd_mfma16x16x4(c, zr, ur);
            ur = cfd_mfma16x16x4(-sn, zi, ur);
            ui = cfd_mfma16x16x4(c, zi, ui);
            ui = cfd_mfma16x16x4(sn, zr, ui);
            idx += step;
            idx -= idx >= H ? H : 0;
            sur.flush(ur), sui.flush(ui);
        }
        ur = sur.result(ur), ui = sui.result(ui);
        const int col = l0 + i16;
        if (col < d.Wf) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                us[(x0 + 4 * k4 + r) * d.LU + col] = ur[r];
                us[(x0 + 4 * k4 + r) * d.LU + d.Wf4 + col] = ui[r];
            }
        }
    }
    __syncthreads();
    // stage W': out[x][y] = sum_l cos(2 pi l y / W) U_re[x][l] - sin(2 pi l y / W) U_im[x][l]
    const int ny = d.Wq / 16, ntw = (d.Hp / 16) * ny;
    for (int t = wave; t < ntw; t += 4) {
        const int x0 = (t / ny) * 16, y0 = (t % ny) * 16;
        const int y = y0 + i16, ym = y < W ? y : 0;
        const int step = (4 * ym) % W;
        const float* ua = us + (x0 + i16) * d.LU + k4;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        HsSum sum;
        int idx = (k4 * ym) % W;
        for (int c = 0; c < d.Wf4; c += 4) {
            acc = cfd_mfma16x16x4(ua[c], s.tcw[idx], acc);
            idx += step;
            idx -= idx >= W ? W : 0;
            if (c & 4) sum.flush(acc);
        }
        sum.flush(acc);
        idx = (k4 * ym) % W;
        for (int c = 0; c < d.Wf4; c += 4) {
            acc = cfd_mfma16x16x4(ua[d.Wf4 + c], -s.tsw[idx], acc);
            idx += step;
            idx -= idx >= W ? W : 0;
            if (c & 4) sum.flush(acc);
        }
        acc = sum.result(acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int xr = x0 + 4 * k4 + r;
            if (xr < H && y < W) {
                const size_t at = base + (size_t)xr * W + y;
                const float term = (float)(scale * (double)acc[r]);  // (the one rounding of the term)
                gpreds[at] = GADD ? gadd[at] + term : term;
            }
        }
    }
}

// ---- host side ----
static bool hs_aligned16(std::initializer_list<const void*> bufs) {
    uintptr_t bits = 0;
    for (const void* b : bufs) bits |= (uintptr_t)b;  // (NULL adds nothing)
    return (bits & 15) == 0;
}
static int hs_check(const char* fn, int B, int Co, int H, int W, int k, int balanced) {
    CFD_REQUIRE(k == 1 || k == 2, CFD_ERR_INVALID_ARG, "%s: k = %d must be 1 or 2", fn, k);
    CFD_REQUIRE(balanced == 0 || balanced == 1, CFD_ERR_INVALID_ARG, "%s: balanced = %d must be 0 or 1", fn, balanced);
    CFD_REQUIRE(B >= 1 && Co >= 1, CFD_ERR_INVALID_ARG, "%s: B = %d, Co = %d must both be >= 1", fn, B, Co);
    CFD_REQUIRE(H >= 2 && H <= 128 && W >= 2 && W <= 128, CFD_ERR_UNSUPPORTED, "%s: grid %d x %d is outside 2 .. 128", fn, H, W);
    // (one workgroup per image: the grid's x dimension holds them)
    CFD_REQUIRE((size_t)B * (size_t)Co < (1ull << 31), CFD_ERR_UNSUPPORTED, "%s: B * Co = %zu images are too many", fn, (size_t)B * (size_t)Co);
    CFD_REQUIRE(hs_lds_bytes(H, W) + HS_STATIC_LDS <= HS_LDS_CAP, CFD_ERR_UNSUPPORTED, "%s: grid %d x %d needs %zu bytes of LDS, more than %d", fn, H,
                W, hs_lds_bytes(H, W) + HS_STATIC_LDS, HS_LDS_CAP);
    return CFD_OK;
}
static HsArgs hs_args(int k, float a1, float a2, int balanced) {
    return HsArgs{k, balanced, (double)a1 * (double)a1, k >= 2 ? (double)a2 * (double)a2 : 0.0};
}
// multiply-adds of one half-spectrum transform (stage W + stage H), times 2 for flops
static double hs_transform_flops(int H, int W) { return 2.0 * ((double)H * W * (W + 2) + 2.0 * H * H * (W + 2)); }

extern "C" int cfd_sobolev_fwd(const float* preds, const float* label, const float* mask, float* rec, float* value, int B, int Co, int H,
                               int W, int k, float a1, float a2, int balanced, void* stream) {
    CFD_REQUIRE(preds && label && rec && value, CFD_ERR_INVALID_ARG, "cfd_sobolev_fwd: NULL pointer");
    CFD_TRY(hs_check("cfd_sobolev_fwd", B, Co, H, W, k, balanced));
    const size_t lds = hs_lds_bytes(H, W);
    const unsigned nimg = (unsigned)((size_t)B * Co);
    float* recs = rec + 2 + 12 * (size_t)B;
    const bool vec = W % 4 == 0 && hs_aligned16({preds, label, mask});
    const double n = (double)nimg * H * W;
    {
        CFD_PROF_W("k_hs_fwd", (hipStream_t)stream, 8.0 * n + (mask ? 4.0 * B * H * W : 0.0) + 48.0 * nimg, 2.0 * nimg * hs_transform_flops(H, W));
        int rc = CFD_OK;
        with_bools([&](auto V, auto M) {
            rc = cfd_allow_lds<k_hs_fwd<CFD_B(V), CFD_B(M)>>(lds, "cfd_sobolev_fwd");
            if (rc != CFD_OK) return;
            hipLaunchKernelGGL((k_hs_fwd<CFD_B(V), CFD_B(M)>), dim3(nimg), dim3(256), lds, (hipStream_t)stream, preds, label, mask, recs, Co, H, W);
        }, vec, mask != nullptr);
        CFD_TRY(rc);
        CFD_LAUNCH_CHECK("cfd_sobolev_fwd");
    }
    CFD_PROF_W("k_hs_final", (hipStream_t)stream, 48.0 * nimg + 48.0 * B + 12.0, 12.0 * nimg);
    hipLaunchKernelGGL(k_hs_final, dim3(1), dim3(256), 0, (hipStream_t)stream, rec, recs, value, B, Co, hs_args(k, a1, a2, balanced));
    CFD_LAUNCH_CHECK("cfd_sobolev_fwd");
    return CFD_OK;
}

extern "C" int cfd_sobolev_bwd(const float* preds, const float* label, const float* mask, const float* rec, const float* gadd,
                               const float* upstream_dev, float upstream, float* gpreds, int B, int Co, int H, int W, int k, float a1,
                               float a2, int balanced, void* stream) {
    CFD_REQUIRE(preds && label && rec && gpreds, CFD_ERR_INVALID_ARG, "cfd_sobolev_bwd: NULL pointer");
    CFD_TRY(hs_check("cfd_sobolev_bwd", B, Co, H, W, k, balanced));
    const size_t lds = hs_lds_bytes(H, W);
    const unsigned nimg = (unsigned)((size_t)B * Co);
    const bool vec = W % 4 == 0 && hs_aligned16({preds, label, mask});
    const double n = (double)nimg * H * W;
    // read preds, label (and gadd), the mask row once per sample; write gpreds
    CFD_PROF_W("k_hs_bwd", (hipStream_t)stream, (gadd ? 16.0 : 12.0) * n + (mask ? 4.0 * B * H * W : 0.0) + 48.0 * B, 2.0 * nimg * hs_transform_flops(H, W));
    int rc = CFD_OK;
    with_bools([&](auto V, auto M, auto A) {
        rc = cfd_allow_lds<k_hs_bwd<CFD_B(V), CFD_B(M), CFD_B(A)>>(lds, "cfd_sobolev_bwd");
        if (rc != CFD_OK) return;
        hipLaunchKernelGGL((k_hs_bwd<CFD_B(V), CFD_B(M), CFD_B(A)>), dim3(nimg), dim3(256), lds, (hipStream_t)stream, preds, label, mask, rec,
                           gadd, upstream_dev, upstream, gpreds, B, Co, H, W, hs_args(k, a1, a2, balanced));
    }, vec, mask != nullptr, gadd != nullptr);
    CFD_TRY(rc);
    CFD_LAUNCH_CHECK("cfd_sobolev_bwd");
    return CFD_OK;
}
