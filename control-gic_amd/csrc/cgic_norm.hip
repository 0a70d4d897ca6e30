// cgic_norm.hip -- the decoder's SpatialNorm (decoder.py:34-53) as one pass over the features, on fp32, fp16 and bf16:
//     zq    = interpolate(zq, size=f.shape[-2:], mode="nearest")
//     new_f = GroupNorm(groups, eps, affine)(f) * conv_y(zq) + conv_b(zq)          conv_y, conv_b: 1x1, 4 -> C
// and, on request, the swish that ResnetBlock puts directly behind it (decoder.py:29-31).  torch runs this as six element-wise
// passes over [B,C,H,W] (two conv outputs written in full from a 4-channel input, GroupNorm, a multiply, an add, the swish); here
// the features are read once or twice and written once, and zq (4 channels, at most a few KB per image row) comes out of the caches.
//
// Values.  A group (b, g) is one contiguous span of (C / groups) * H * W elements.  Its mean and biased variance are accumulated in
// float64 as sums of x - K and (x - K)^2, K the span's first element (so the variance does not cancel), rstd = 1 / sqrt(var + eps);
// mean and rstd are each rounded once to fp32.  Per element, in fp32 and without contraction (-ffp-contract=off):
//     n = ((x - mean) * rstd) * gamma[c] + beta[c]
//     y = by[c] + sum_k wy[c,k] * zq[b,k,sy,sx]    (k = 0..3 in order; b likewise from wb, bb)
//     v = n * y + b;    with swish  v / (1 + exp(-v))
// Half features are upcast exactly; a half output is the fp32 value rounded once to nearest-even.
//
// Two forms, chosen by cgic_norm_plan.h (which also holds every check of the call); no workgroup ever waits for another:
//   norm_one_kernel                       one workgroup per span: the span goes to LDS in the feature type while it is summed, then
//                                         the waves apply from LDS, each wave one channel (or a piece of one) at a time;
//   norm_stats_kernel + norm_apply_kernel ordered by the stream: a (span, chunk) grid writes one (sum, sum of squares) pair of
//                                         doubles per chunk (and K per span) to the caller's workspace; the apply workgroups add
//                                         their span's partials in chunk order, so the result does not depend on scheduling.
// A workgroup's (the one-launch form: a wave's) channel is uniform: its twelve parameters are scalar loads.  A thread takes U
// consecutive elements of a row: 16 bytes of the feature type where the plan allows, else fewer.  Where x is at ratio 1 it reads
// its pixels of each zq channel as 16-byte vectors, all issued before the first is used; otherwise the four zq values of a pixel
// are loaded once and serve every x of the thread that falls on that pixel.  The index divisions (by the row width and the two ratios) are multiplications by the plan's magic numbers.
// Every element is read before it is written in both forms, so out may be f.
//
// The encoder's plain GroupNorm (vqvae_blocks.py:34, and the swish of ResnetBlock / the norm_out heads behind it) is the same kernel
// family instantiated with MOD = false (cgic_group_norm, _train, _backward): the same statistics, per element
//     v = ((x - mean) * rstd) * gamma[c] + beta[c];    with swish  v / (1 + exp(-v))
// No zq pointer reaches those instantiations and no y / b value is loaded or multiplied; norm_stats_kernel never saw zq and is
// shared.  On finite inputs the result is bit for bit the modulated one at wy = wb = 0, by = 1, bb = 0 (n * 1 + 0 is exact).
#include "cgic_common.h"
#include "cgic_norm_bwd_plan.h"
#include "cgic_norm_plan.h"

namespace cgic {
namespace norm {

// a feature type: its raw element, the exact upcast and, for a half, the rounding of a fp32 value to it
struct F32 {
    using raw = uint32_t;
    static __device__ __forceinline__ float up(uint32_t v) { return __uint_as_float(v); }
};
struct F16 {
    using raw = uint16_t;
    static __device__ __forceinline__ float up(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
    static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
};
struct BF16 {
    using raw = uint16_t;
    static __device__ __forceinline__ float up(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
    static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
};

template <int BYTES> struct RawOf;
template <> struct RawOf<2> { using type = uint16_t; };
template <> struct RawOf<4> { using type = uint32_t; };
template <> struct RawOf<8> { using type = uint2; };
template <> struct RawOf<16> { using type = uint4; };

// N consecutive elements as ONE access of their size
template <class E, int N>
__device__ __forceinline__ void load_n(const E *p, E (&v)[N])
{
    using R = typename RawOf<sizeof(E) * N>::type;
    const R r = *reinterpret_cast<const R *>(p);
    __builtin_memcpy(v, &r, sizeof(R));
}
template <class E, int N>
__device__ __forceinline__ void store_n(E *p, const E (&v)[N])
{
    using R = typename RawOf<sizeof(E) * N>::type;
    R r;
    __builtin_memcpy(&r, v, sizeof(R));
    *reinterpret_cast<R *>(p) = r;
}
// N results to out[idx ...]: rounded to T's half type (HOUT), or as they are (8 floats: two 16-byte stores)
template <class T, bool HOUT, int N>
__device__ __forceinline__ void store_out(void *out, int64_t idx, const float (&o)[N])
{
    if constexpr (HOUT) {
        typename T::raw v[N];
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = T::down(o[i]);
        store_n<typename T::raw, N>(reinterpret_cast<typename T::raw *>(out) + idx, v);
    } else if constexpr (N == 8) {
        float4 *dst = reinterpret_cast<float4 *>(reinterpret_cast<float *>(out) + idx);
        dst[0] = make_float4(o[0], o[1], o[2], o[3]);
        dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    } else {
        store_n<float, N>(reinterpret_cast<float *>(out) + idx, o);
    }
}

// U consecutive floats of zq as one access (8: two)
template <int U>
__device__ __forceinline__ void load_zq(const float *p, float (&z)[U])
{
    if constexpr (U == 8) {
        float lo[4], hi[4];
        load_n<float, 4>(p, lo);
        load_n<float, 4>(p + 4, hi);
#pragma unroll
        for (int j = 0; j < 4; ++j) { z[j] = lo[j]; z[4 + j] = hi[j]; }
    } else {
        load_n<float, U>(p, z);
    }
}

// n / d by the plan's magic multiplier (exact for the plan's dividends), or plainly where the plan has none
__device__ __forceinline__ unsigned fdiv(unsigned n, unsigned m, unsigned d) { return m ? __umulhi(n, m) : d == 1 ? n : n / d; }

// what the kernels know of a call besides the features
struct Geom {
    int C, cpg, groups;             // channels, channels per group, groups
    int H, W, hq, wq;
    int ymul, ydiv, xmul, xdiv;     // the nearest index: src = dst * mul / div (one of the two is 1)
    unsigned mg_w, mg_y, mg_x;      // magic multipliers of the divisions by W, ydiv, xdiv (0: divide)
    int zq_vec;                     // x at ratio 1 and zq aligned: a thread's pixels of a channel are one access
    int swish;
    double eps;
    const float *zq, *gamma, *beta, *wy, *by, *wb, *bb;
};

// the twelve parameters of a channel; c is uniform where this is called, so these are scalar loads
struct Chan {
    float gamma, beta, by, bb, wy[kNormZq], wb[kNormZq];
};
__device__ __forceinline__ Chan load_chan(const Geom &g, int c)
{
    Chan w;
    w.gamma = g.gamma[c]; w.beta = g.beta[c]; w.by = g.by[c]; w.bb = g.bb[c];
#pragma unroll
    for (int k = 0; k < kNormZq; ++k) { w.wy[k] = g.wy[c * kNormZq + k]; w.wb[k] = g.wb[c * kNormZq + k]; }
    return w;
}

// mean and rstd of a span from its two sums about K, each rounded once to fp32.  A NaN or an Inf in the span makes both sums
// non-finite and the variance a NaN: the whole span comes out NaN, as in the reference.
__device__ __forceinline__ void finish_stats(double K, double s1, double s2, double n, double eps, float *mean, float *rstd)
{
    const double m = s1 / n;
    double var = s2 / n - m * m;
    if (var < 0.0) var = 0.0;                       // (a NaN stays a NaN)
    *mean = (float)(K + m);
    *rstd = (float)(1.0 / sqrt(var + eps));
}

// the two sums of a thread's elements about K
template <class T, int U>
__device__ __forceinline__ void accumulate(const typename T::raw (&v)[U], double K, double *s1, double *s2)
{
#pragma unroll
    for (int j = 0; j < U; ++j) {
        const double d = (double)T::up(v[j]) - K;
        *s1 += d;
        *s2 += d * d;
    }
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;                                       // (lane 0 holds the wave's sum)
}

// units [first, end) of one channel's plane, `step` apart: src is the plane (in global memory or in LDS), out_plane the index of
// its first element in out, zq_b the image's zq
template <class T, bool HOUT, int U>
__device__ __forceinline__ void apply_units(const typename T::raw *src, void *out, int64_t out_plane, unsigned first, unsigned end,
                                            unsigned step, const Geom &g, const float *zq_b, const Chan &w, float mean, float rstd)
{
    const unsigned W = (unsigned)g.W, plane_q = (unsigned)g.hq * (unsigned)g.wq;
    for (unsigned i = first; i < end; i += step) {
        const unsigned e = i * U;
        const unsigned y = fdiv(e, g.mg_w, W), x = e - y * W;
        const unsigned sy = fdiv(y * (unsigned)g.ymul, g.mg_y, (unsigned)g.ydiv);
        typename T::raw v[U];
        load_n<typename T::raw, U>(src + e, v);
        const float *zrow = zq_b + (size_t)sy * (unsigned)g.wq;
        float o[U];
        const auto element = [&](int j, float yv, float bv) {
            const float n = ((T::up(v[j]) - mean) * rstd) * w.gamma + w.beta;
            float val = n * yv + bv;
            if (g.swish) val = val / (1.0f + expf(-val));
            o[j] = val;
        };
        if (g.zq_vec) {
            // x at ratio 1: the thread's U consecutive pixels of each zq channel as one access, all issued before the first is used
            float z[kNormZq][U];
#pragma unroll
            for (int k = 0; k < kNormZq; ++k) load_zq<U>(zrow + (size_t)k * plane_q + x, z[k]);
#pragma unroll
            for (int j = 0; j < U; ++j) {
                float yv = w.by, bv = w.bb;
#pragma unroll
                for (int k = 0; k < kNormZq; ++k) {
                    yv = yv + w.wy[k] * z[k][j];
                    bv = bv + w.wb[k] * z[k][j];
                }
                element(j, yv, bv);
            }
        } else {
            const unsigned acc = x * (unsigned)g.xmul;
            unsigned sx = fdiv(acc, g.mg_x, (unsigned)g.xdiv), rem = acc - sx * (unsigned)g.xdiv;
            float yv = 0.f, bv = 0.f;
#pragma unroll
            for (int j = 0; j < U; ++j) {
                if (j == 0 || rem == 0) {           // a new zq pixel: its four values once, for every x that falls on it
                    yv = w.by;
                    bv = w.bb;
#pragma unroll
                    for (int k = 0; k < kNormZq; ++k) {
                        const float z = zrow[(size_t)k * plane_q + sx];
                        yv = yv + w.wy[k] * z;
                        bv = bv + w.wb[k] * z;
                    }
                }
                element(j, yv, bv);
                // the next x: sub-sampling (xdiv == 1) moves on by xmul pixels, up-sampling by one pixel every xdiv steps
                if (g.xdiv == 1) {
                    sx += (unsigned)g.xmul;
                } else if (++rem == (unsigned)g.xdiv) {
                    rem = 0;
                    ++sx;
                }
            }
        }
        store_out<T, HOUT, U>(out, out_plane + e, o);
    }
}

// the same units of the plain GroupNorm: no zq, v = n
template <class T, bool HOUT, int U>
__device__ __forceinline__ void apply_units_plain(const typename T::raw *src, void *out, int64_t out_plane, unsigned first, unsigned end,
                                                  unsigned step, int swish, float gamma, float beta, float mean, float rstd)
{
    for (unsigned i = first; i < end; i += step) {
        const unsigned e = i * U;
        typename T::raw v[U];
        load_n<typename T::raw, U>(src + e, v);
        float o[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            float val = ((T::up(v[j]) - mean) * rstd) * gamma + beta;
            if (swish) val = val / (1.0f + expf(-val));
            o[j] = val;
        }
        store_out<T, HOUT, U>(out, out_plane + e, o);
    }
}
// channel c of image b: MOD the modulated layer (the twelve parameters, zq), else the plain one (gamma and beta alone)
template <class T, bool HOUT, int U, bool MOD>
__device__ __forceinline__ void apply_channel(const typename T::raw *src, void *out, int64_t out_plane, unsigned first, unsigned end, unsigned step,
                                              const Geom &g, int64_t b, int c, float mean, float rstd)
{
    if constexpr (MOD) {
        const Chan w = load_chan(g, c);
        apply_units<T, HOUT, U>(src, out, out_plane, first, end, step, g, g.zq + (size_t)b * kNormZq * (unsigned)g.hq * (unsigned)g.wq, w, mean, rstd);
    } else {
        apply_units_plain<T, HOUT, U>(src, out, out_plane, first, end, step, g.swish, g.gamma[c], g.beta[c], mean, rstd);
    }
}

// ---- one launch: one workgroup per span
template <class T, bool HOUT, int U, bool MOD>
__global__ __launch_bounds__(kNormOneThreads) void norm_one_kernel(const typename T::raw *f, Geom g, unsigned span_bytes16, void *out, float *stats)
{
    using E = typename T::raw;
    extern __shared__ __attribute__((aligned(16))) unsigned char norm_lds[];
    E *sp = reinterpret_cast<E *>(norm_lds);
    double *part = reinterpret_cast<double *>(norm_lds + span_bytes16);
    const int64_t spn = blockIdx.x;
    const unsigned plane = (unsigned)g.H * (unsigned)g.W, span = (unsigned)g.cpg * plane, units = span / U;
    const E *src = f + spn * (int64_t)span;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = lane_id(), nw = (int)(blockDim.x >> 6);
    // the span to LDS, summed on the way
    const double K = (double)T::up(src[0]);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (unsigned i = threadIdx.x; i < units; i += blockDim.x) {
        E v[U];
        load_n<E, U>(src + (size_t)i * U, v);
        store_n<E, U>(sp + (size_t)i * U, v);
        accumulate<T, U>(v, K, &s1, &s2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (lane == 0) { part[2 * wave] = s1; part[2 * wave + 1] = s2; }
    __syncthreads();                                // (the span and the waves' sums are in LDS; global f is not read again)
    double t1 = 0.0, t2 = 0.0;
    for (int k = 0; k < nw; ++k) { t1 += part[2 * k]; t2 += part[2 * k + 1]; }
    float mean, rstd;
    finish_stats(K, t1, t2, (double)span, g.eps, &mean, &rstd);
    if (stats && threadIdx.x == 0) { stats[2 * spn] = mean; stats[2 * spn + 1] = rstd; }       // (the training forward)
    // apply from LDS: a wave takes one channel, or 256 units of one, at a time
    const int64_t b = spn / g.groups;
    const int grp = (int)(spn - b * g.groups);
    const unsigned plane_units = plane / U, seg_units = 4 * kWave;
    const unsigned segs = (plane_units + seg_units - 1) / seg_units, items = (unsigned)g.cpg * segs;
    for (unsigned it = (unsigned)wave; it < items; it += (unsigned)nw) {
        const unsigned cl = it / segs, sg = it - cl * segs;
        const unsigned first = sg * seg_units, last = first + seg_units < plane_units ? first + seg_units : plane_units;
        apply_channel<T, HOUT, U, MOD>(sp + (size_t)cl * plane, out, spn * (int64_t)span + (int64_t)cl * plane, first + (unsigned)lane, last, kWave,
                                       g, b, grp * g.cpg + (int)cl, mean, rstd);
    }
}

// ---- two launches.  The workspace: spans * chunks pairs (sum, sum of squares), then one K per span
template <class T, int U>
__global__ __launch_bounds__(kNormThreads) void norm_stats_kernel(const typename T::raw *f, unsigned units, int chunks, unsigned chunk_units,
                                                                  int64_t spans, double *ws)
{
    using E = typename T::raw;
    __shared__ double part[2 * (kNormThreads / kWave)];
    const int64_t spn = blockIdx.x / (unsigned)chunks;
    const unsigned ch = (unsigned)(blockIdx.x - spn * chunks);
    const E *src = f + spn * (int64_t)units * U;
    const double K = (double)T::up(src[0]);
    const unsigned first = ch * chunk_units;
    const unsigned last = first + chunk_units < units ? first + chunk_units : units;
    double s1 = 0.0, s2 = 0.0;
    for (unsigned i = first + threadIdx.x; i < last; i += blockDim.x) {
        E v[U];
        load_n<E, U>(src + (size_t)i * U, v);
        accumulate<T, U>(v, K, &s1, &s2);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const int wave = (int)(threadIdx.x >> 6);
    if (lane_id() == 0) { part[2 * wave] = s1; part[2 * wave + 1] = s2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < kNormThreads / kWave; ++k) { t1 += part[2 * k]; t2 += part[2 * k + 1]; }
        double *dst = ws + ((int64_t)blockIdx.x) * 2;
        dst[0] = t1;
        dst[1] = t2;
        if (ch == 0) ws[spans * chunks * 2 + spn] = K;
    }
}

template <class T, bool HOUT, int U, bool MOD>
__global__ __launch_bounds__(kNormThreads) void norm_apply_kernel(const typename T::raw *f, Geom g, const double *ws, int chunks, int64_t spans,
                                                                  int64_t items, unsigned parts, void *out, float *stats)
{
    const unsigned plane = (unsigned)g.H * (unsigned)g.W, plane_units = plane / U;
    const double n = (double)g.cpg * (double)plane;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t bc = it / parts;
        const unsigned part = (unsigned)(it - bc * parts);
        const int64_t b = bc / g.C;
        const int c = (int)(bc - b * g.C);
        const int64_t spn = b * g.groups + c / g.cpg;
        // the span's partials in chunk order (uniform: every thread adds the same numbers in the same order)
        const double *p = ws + spn * chunks * 2;
        double t1 = 0.0, t2 = 0.0;
        for (int k = 0; k < chunks; ++k) { t1 += p[2 * k]; t2 += p[2 * k + 1]; }
        float mean, rstd;
        finish_stats(ws[spans * chunks * 2 + spn], t1, t2, n, g.eps, &mean, &rstd);
        if (stats && part == 0 && c % g.cpg == 0 && threadIdx.x == 0) { stats[2 * spn] = mean; stats[2 * spn + 1] = rstd; }
        const unsigned first = part * (unsigned)kNormPartUnits;
        const unsigned last = first + (unsigned)kNormPartUnits < plane_units ? first + (unsigned)kNormPartUnits : plane_units;
        apply_channel<T, HOUT, U, MOD>(f + bc * (int64_t)plane, out, bc * (int64_t)plane, first + threadIdx.x, last, blockDim.x, g, b, c, mean, rstd);
    }
}

// ---- the launches: the plan's form and unit and the call's type pair pick the instantiation
template <class T, bool HOUT, int U, bool MOD>
static int launch_unit(const NormCall &c, const NormPlan &p, const Geom &g, float *stats, hipStream_t s)
{
    using E = const typename T::raw *;
    if (p.form == 1) {
        const auto kernel = norm_one_kernel<T, HOUT, U, MOD>;
        const int rc = ensure_lds_above_48k((const void *)kernel, p.lds_bytes);
        if (rc) return rc;
        const unsigned span_bytes16 = (unsigned)(p.lds_bytes - 2 * sizeof(double) * (size_t)(kNormOneThreads / kWave));
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid_one), dim3(p.threads_one), p.lds_bytes, s, (E)c.f, g, span_bytes16, (void *)c.out, stats);
        return launch_check("norm_one_kernel");
    }
    const unsigned units = (unsigned)(p.span / U);
    hipLaunchKernelGGL((norm_stats_kernel<T, U>), dim3((unsigned)p.grid_stats), dim3(p.threads), 0, s, (E)c.f, units, p.chunks,
                       (unsigned)p.chunk_units, p.spans, (double *)c.workspace);
    int rc = launch_check("norm_stats_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL((norm_apply_kernel<T, HOUT, U, MOD>), dim3((unsigned)p.grid_apply), dim3(p.threads), 0, s, (E)c.f, g,
                       (const double *)c.workspace, p.chunks, p.spans, c.B * c.C * p.parts, (unsigned)p.parts, (void *)c.out, stats);
    return launch_check("norm_apply_kernel");
}

template <class T, bool HOUT, bool MOD>
static int launch_typed(const NormCall &c, const NormPlan &p, const Geom &g, float *stats, hipStream_t s)
{
    if constexpr (sizeof(typename T::raw) == 2)
        if (p.unit == 8) return launch_unit<T, HOUT, 8, MOD>(c, p, g, stats, s);
    switch (p.unit) {
    case 4: return launch_unit<T, HOUT, 4, MOD>(c, p, g, stats, s);
    case 2: return launch_unit<T, HOUT, 2, MOD>(c, p, g, stats, s);
    default: return launch_unit<T, HOUT, 1, MOD>(c, p, g, stats, s);
    }
}

// the call's type pair
template <bool MOD>
static int launch_call(const NormCall &c, const NormPlan &p, const Geom &g, float *stats, hipStream_t s)
{
    const bool hout = c.out_dtype != CGIC_DT_F32;
    if (c.in_dtype == CGIC_DT_F32) return launch_typed<F32, false, MOD>(c, p, g, stats, s);
    if (c.in_dtype == CGIC_DT_F16) return hout ? launch_typed<F16, true, MOD>(c, p, g, stats, s) : launch_typed<F16, false, MOD>(c, p, g, stats, s);
    return hout ? launch_typed<BF16, true, MOD>(c, p, g, stats, s) : launch_typed<BF16, false, MOD>(c, p, g, stats, s);
}

// ================================================================================================================ the backward
// With go the incoming gradient and mean, rstd the training forward's (stats), per element in fp32, v recomputed as the forward does:
//     xhat = (x - mean) * rstd;  n = xhat * gamma[c] + beta[c];  y, b as above;  v = n * y + b
//     gv = go, with swish go * (s * (1 + v * (1 - s))), s = 1 / (1 + exp(-v));     gn = gv * y;  gy = gv * n
//     df = rstd * ((gamma[c] * gn - S1 / N) - xhat * (S2 / N)),   S1 = sum_c gamma[c] sum_p gn,  S2 = sum_c gamma[c] sum_p gn * xhat
//     dbeta = sum gn, dgamma = sum gn * xhat, dby = sum gy, dbb = sum gv, dwy[k] = sum gy * z_k, dwb[k] = sum gv * z_k   (over b, p)
//     dz_k(b, p) = sum_c wy[c,k] * gy + wb[c,k] * gv, folded through the nearest index into dzq
// Every sum is accumulated in float64 in an order that cgic_norm_bwd_plan.h fixes (three launches ordered by the stream: reduce,
// finish, apply; no atomics), so two calls give the same bits and an image's df and dzq do not depend on its batch.  A NaN in f
// reaches every gradient it reaches in the reference: nothing here selects, clamps or skips by value.
struct BwdGeom {
    Geom g;
    const float *stats;             // [B * groups][2] = (mean, rstd)
    int chan_block, chan_blocks, tiles, need_dz, need_conv, need_df;
    double *sums;                   // workspace: [B][C][tiles][12]
    double *span;                   //            [B][C][2] = gamma_c * (sum gn, sum gn * xhat) of the plane
    float *dz;                      //            [B][chan_blocks][4][H * W]
};

// U consecutive elements of go: one access, or two of 16 bytes (8 floats)
template <class E, int U>
__device__ __forceinline__ void load_go(const E *p, E (&v)[U])
{
    if constexpr (sizeof(E) * U == 32) {
        E lo[U / 2], hi[U / 2];
        load_n<E, U / 2>(p, lo);
        load_n<E, U / 2>(p + U / 2, hi);
#pragma unroll
        for (int j = 0; j < U / 2; ++j) { v[j] = lo[j]; v[U / 2 + j] = hi[j]; }
    } else {
        load_n<E, U>(p, v);
    }
}

// zq's four values at each of the U pixels of the unit at (y, x)
template <int U>
__device__ __forceinline__ void load_z(const Geom &g, const float *zq_b, unsigned y, unsigned x, float (&z)[kNormZq][U])
{
    const unsigned plane_q = (unsigned)g.hq * (unsigned)g.wq;
    const unsigned sy = fdiv(y * (unsigned)g.ymul, g.mg_y, (unsigned)g.ydiv);
    const float *zrow = zq_b + (size_t)sy * (unsigned)g.wq;
    if (g.zq_vec) {
#pragma unroll
        for (int k = 0; k < kNormZq; ++k) {
            float row[U];                           // (element by element into z: a block copy into a row of it would keep z in scratch)
            load_zq<U>(zrow + (size_t)k * plane_q + x, row);
#pragma unroll
            for (int j = 0; j < U; ++j) z[k][j] = row[j];
        }
    } else {
        const unsigned acc = x * (unsigned)g.xmul;
        unsigned sx = fdiv(acc, g.mg_x, (unsigned)g.xdiv), rem = acc - sx * (unsigned)g.xdiv;
#pragma unroll
        for (int j = 0; j < U; ++j) {
#pragma unroll
            for (int k = 0; k < kNormZq; ++k) z[k][j] = (j == 0 || rem == 0) ? zrow[(size_t)k * plane_q + sx] : z[k][j > 0 ? j - 1 : 0];
            if (g.xdiv == 1) {
                sx += (unsigned)g.xmul;
            } else if (++rem == (unsigned)g.xdiv) {
                rem = 0;
                ++sx;
            }
        }
    }
}

// the terms of one element
struct Terms {
    float xhat, n, y, gv;
};
__device__ __forceinline__ Terms bwd_terms(const Chan &w, int swish, float x, float mean, float rstd, float go, float z0, float z1, float z2, float z3)
{
    const float z[kNormZq] = {z0, z1, z2, z3};
    float yv = w.by, bv = w.bb;
#pragma unroll
    for (int k = 0; k < kNormZq; ++k) {
        yv = yv + w.wy[k] * z[k];
        bv = bv + w.wb[k] * z[k];
    }
    Terms t;
    t.xhat = (x - mean) * rstd;
    t.n = t.xhat * w.gamma + w.beta;
    t.y = yv;
    t.gv = go;
    if (swish) {
        const float v = t.n * yv + bv;
        const float sg = 1.0f / (1.0f + expf(-v));
        t.gv = go * (sg * (1.0f + v * (1.0f - sg)));
    }
    return t;
}

// the plain GroupNorm's: v = n, so y = 1 and gn = gv (one multiplication less, the same bits as the modulated terms at y = 1, b = 0)
__device__ __forceinline__ Terms bwd_terms_plain(float gamma, float beta, int swish, float x, float mean, float rstd, float go)
{
    Terms t;
    t.xhat = (x - mean) * rstd;
    t.n = t.xhat * gamma + beta;
    t.y = 1.0f;
    t.gv = go;
    if (swish) {
        const float v = t.n;
        const float sg = 1.0f / (1.0f + expf(-v));
        t.gv = go * (sg * (1.0f + v * (1.0f - sg)));
    }
    return t;
}

// ---- reduce: workgroup (b, channel block, pixel tile); a thread keeps one unit of pixels and walks the block's channels.
// MOD: the modulated layer.  Without it (the plain GroupNorm) a channel has two plane sums, nothing of zq is read and no dz written
template <class T, class G, int U, bool MOD>
__global__ __launch_bounds__(kNormBwdThreads) void norm_bwd_reduce_kernel(const typename T::raw *f, const typename G::raw *go, BwdGeom a)
{
    constexpr int NS = MOD ? kNormBwdSums : 2;      // sums per (channel, tile) in the workspace
    __shared__ double part[kNormBwdChanBlock][kNormBwdThreads / kWave][NS];
    const Geom &g = a.g;
    const unsigned plane = (unsigned)g.H * (unsigned)g.W, plane_units = plane / U;
    const unsigned tile = blockIdx.x % (unsigned)a.tiles, rest = blockIdx.x / (unsigned)a.tiles;
    const unsigned cb = rest % (unsigned)a.chan_blocks;
    const int64_t b = rest / (unsigned)a.chan_blocks;
    const unsigned u = tile * blockDim.x + threadIdx.x;
    const bool live = u < plane_units;
    const unsigned e = live ? u * U : 0u;
    const unsigned y = fdiv(e, g.mg_w, (unsigned)g.W), x = e - y * (unsigned)g.W;
    const int wave = (int)(threadIdx.x >> 6), lane = lane_id(), nw = (int)(blockDim.x >> 6);
    float z[kNormZq][U];
    double dz[kNormZq][U];
    if constexpr (MOD) {
        load_z<U>(g, g.zq + (size_t)b * kNormZq * (unsigned)g.hq * (unsigned)g.wq, y, x, z);      // (a thread without a unit: the plane's first)
#pragma unroll
        for (int k = 0; k < kNormZq; ++k)
#pragma unroll
            for (int j = 0; j < U; ++j) dz[k][j] = 0.0;
    }
    const int c0 = (int)cb * a.chan_block, c1 = c0 + a.chan_block < g.C ? c0 + a.chan_block : g.C;
    const unsigned nsum = MOD && a.need_conv ? (unsigned)kNormBwdSums : 2u;       // sums per channel that are added, written and later read
    for (int c = c0; c < c1; ++c) {
        const int64_t spn = b * g.groups + c / g.cpg;
        const float mean = a.stats[2 * spn], rstd = a.stats[2 * spn + 1];
        double s[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) s[i] = 0.0;
        if constexpr (!MOD) {
            const float gamma = g.gamma[c], beta = g.beta[c];
            if (live) {
                const int64_t at = (b * g.C + c) * (int64_t)plane + e;
                typename T::raw fv[U];
                typename G::raw gov[U];
                load_n<typename T::raw, U>(f + at, fv);
                load_go<typename G::raw, U>(go + at, gov);
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const Terms t = bwd_terms_plain(gamma, beta, g.swish, T::up(fv[j]), mean, rstd, G::up(gov[j]));
                    s[0] += (double)t.gv;
                    s[1] += (double)(t.gv * t.xhat);
                }
            }
        } else {
            const Chan w = load_chan(g, c);
            if (live) {
                const int64_t at = (b * g.C + c) * (int64_t)plane + e;
                typename T::raw fv[U];
                typename G::raw gov[U];
                load_n<typename T::raw, U>(f + at, fv);
                load_go<typename G::raw, U>(go + at, gov);
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const Terms t = bwd_terms(w, g.swish, T::up(fv[j]), mean, rstd, G::up(gov[j]), z[0][j], z[1][j], z[2][j], z[3][j]);
                    const float gn = t.gv * t.y, gy = t.gv * t.n;
                    s[0] += (double)gn;
                    s[1] += (double)(gn * t.xhat);
                    if (a.need_conv) {
                        s[2] += (double)gy;
                        s[3] += (double)t.gv;
                    }
#pragma unroll
                    for (int k = 0; k < kNormZq; ++k) {
                        if (a.need_conv) {
                            s[4 + k] += (double)(gy * z[k][j]);
                            s[8 + k] += (double)(t.gv * z[k][j]);
                        }
                        if (a.need_dz) dz[k][j] += (double)(w.wy[k] * gy + w.wb[k] * t.gv);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            if ((unsigned)i >= nsum) break;                   // (no conv gradient is wanted: the first two sums only)
            const double t = wave_sum(s[i]);
            if (lane == 0) part[c - c0][wave][i] = t;
        }
    }
    __syncthreads();
    // the waves in wave order: one thread per (channel, sum)
    for (unsigned i = threadIdx.x; i < (unsigned)(c1 - c0) * nsum; i += blockDim.x) {
        const unsigned cl = i / nsum, j = i - cl * nsum;
        double t = 0.0;
        for (int wv = 0; wv < nw; ++wv) t += part[cl][wv][j];
        a.sums[(((b * g.C + c0 + (int)cl) * a.tiles + tile) * NS) + j] = t;
    }
    if constexpr (MOD) {
        if (a.need_dz && live) {
#pragma unroll
            for (int k = 0; k < kNormZq; ++k) {
                float o[U];
#pragma unroll
                for (int j = 0; j < U; ++j) o[j] = (float)dz[k][j];
                store_out<F32, false, U>(a.dz, ((b * a.chan_blocks + cb) * kNormZq + k) * (int64_t)plane + e, o);
            }
        }
    }
}

// ---- finish: the first `grid_sums` workgroups hold a thread per (channel, sum), the others a thread per element of dzq
template <bool MOD>
__global__ __launch_bounds__(kNormBwdThreads) void norm_bwd_finish_kernel(BwdGeom a, int64_t B, unsigned grid_sums, float *dgamma, float *dbeta,
                                                                          float *dwy, float *dby, float *dwb, float *dbb, float *dzq)
{
    constexpr unsigned NS = MOD ? kNormBwdSums : 2;
    const Geom &g = a.g;
    if (!MOD || blockIdx.x < grid_sums) {           // (the plain GroupNorm has no dzq: every workgroup is one of these)
        const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= (unsigned)g.C * NS) return;
        const unsigned c = i / NS, j = i - c * NS;
        if (j >= 2 && !a.need_conv) return;         // (reduce did not write these)
        const double gamma = (double)g.gamma[c];
        double total = 0.0;
        for (int64_t b = 0; b < B; ++b) {
            const double *src = a.sums + (b * g.C + c) * a.tiles * NS + j;
            double s = 0.0;
            for (int t = 0; t < a.tiles; ++t) s += src[(int64_t)t * NS];
            if (j < 2 && a.need_df) a.span[(b * g.C + c) * 2 + j] = gamma * s;
            total += s;
        }
        float *dst = j == 0 ? dbeta : j == 1 ? dgamma : j == 2 ? dby : j == 3 ? dbb : j < 4 + kNormZq ? dwy : dwb;
        if (dst) dst[j < 4 ? c : c * kNormZq + ((j - 4) & (kNormZq - 1))] = (float)total;
        return;
    }
    if constexpr (!MOD) return;
    const unsigned plane = (unsigned)g.H * (unsigned)g.W, plane_q = (unsigned)g.hq * (unsigned)g.wq;
    const int64_t i = (int64_t)(blockIdx.x - grid_sums) * blockDim.x + threadIdx.x;
    if (i >= B * kNormZq * (int64_t)plane_q) return;
    const int64_t bk = i / plane_q;
    const unsigned pix = (unsigned)(i - bk * plane_q), k = (unsigned)(bk & (kNormZq - 1));
    const int64_t b = bk / kNormZq;
    const unsigned sy = pix / (unsigned)g.wq, sx = pix - sy * (unsigned)g.wq;
    // the feature pixels that read this element: a ydiv x xdiv block where the axis is up-sampled; one or none where it is sub-sampled
    const bool hit = sy % (unsigned)g.ymul == 0 && sx % (unsigned)g.xmul == 0;
    const unsigned y0 = g.ymul > 1 ? sy / (unsigned)g.ymul : sy * (unsigned)g.ydiv, x0 = g.xmul > 1 ? sx / (unsigned)g.xmul : sx * (unsigned)g.xdiv;
    double t = 0.0;
    if (hit)
        for (int cb = 0; cb < a.chan_blocks; ++cb) {
            const float *src = a.dz + ((b * a.chan_blocks + cb) * kNormZq + k) * (int64_t)plane;
            for (unsigned dy = 0; dy < (unsigned)g.ydiv; ++dy)
                for (unsigned dx = 0; dx < (unsigned)g.xdiv; ++dx) t += (double)src[(size_t)(y0 + dy) * (unsigned)g.W + x0 + dx];
        }
    dzq[i] = (float)t;
}

// ---- apply: the forward's grid; df of a unit is written after go's unit was read, so df may be go
template <class T, class G, bool HOUT, int U, bool MOD>
__global__ __launch_bounds__(kNormThreads) void norm_bwd_apply_kernel(const typename T::raw *f, const typename G::raw *go, BwdGeom a, int64_t items,
                                                                      unsigned parts, void *df)
{
    const Geom &g = a.g;
    const unsigned plane = (unsigned)g.H * (unsigned)g.W, plane_units = plane / U;
    const double n = (double)g.cpg * (double)plane;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const int64_t bc = it / parts;
        const unsigned part = (unsigned)(it - bc * parts);
        const int64_t b = bc / g.C;
        const int c = (int)(bc - b * g.C), grp = c / g.cpg;
        const int64_t spn = b * g.groups + grp;
        // S1, S2: the group's channels in channel order (uniform)
        const double *sp = a.span + (b * g.C + (int64_t)grp * g.cpg) * 2;
        double s1 = 0.0, s2 = 0.0;
        for (int cl = 0; cl < g.cpg; ++cl) { s1 += sp[2 * cl]; s2 += sp[2 * cl + 1]; }
        const float m1 = (float)(s1 / n), m2 = (float)(s2 / n);
        const float mean = a.stats[2 * spn], rstd = a.stats[2 * spn + 1];
        const unsigned first = part * (unsigned)kNormPartUnits;
        const unsigned last = first + (unsigned)kNormPartUnits < plane_units ? first + (unsigned)kNormPartUnits : plane_units;
        if constexpr (!MOD) {
            const float gamma = g.gamma[c], beta = g.beta[c];
            for (unsigned i = first + threadIdx.x; i < last; i += blockDim.x) {
                const unsigned e = i * U;
                typename T::raw fv[U];
                typename G::raw gov[U];
                load_n<typename T::raw, U>(f + bc * (int64_t)plane + e, fv);
                load_go<typename G::raw, U>(go + bc * (int64_t)plane + e, gov);
                float o[U];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const Terms t = bwd_terms_plain(gamma, beta, g.swish, T::up(fv[j]), mean, rstd, G::up(gov[j]));
                    o[j] = rstd * ((gamma * t.gv - m1) - t.xhat * m2);
                    if constexpr (HOUT) asm volatile("" : "+v"(o[j]));          // (as below: the fp32 product has to exist)
                }
                store_out<T, HOUT, U>(df, bc * (int64_t)plane + e, o);
            }
        } else {
            const Chan w = load_chan(g, c);
            const float *zq_b = g.zq + (size_t)b * kNormZq * (unsigned)g.hq * (unsigned)g.wq;
            for (unsigned i = first + threadIdx.x; i < last; i += blockDim.x) {
                const unsigned e = i * U;
                const unsigned y = fdiv(e, g.mg_w, (unsigned)g.W), x = e - y * (unsigned)g.W;
                float z[kNormZq][U];
                load_z<U>(g, zq_b, y, x, z);
                typename T::raw fv[U];
                typename G::raw gov[U];
                load_n<typename T::raw, U>(f + bc * (int64_t)plane + e, fv);
                load_go<typename G::raw, U>(go + bc * (int64_t)plane + e, gov);
                float o[U];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const Terms t = bwd_terms(w, g.swish, T::up(fv[j]), mean, rstd, G::up(gov[j]), z[0][j], z[1][j], z[2][j], z[3][j]);
                    const float gn = t.gv * t.y;
                    o[j] = rstd * ((w.gamma * gn - m1) - t.xhat * m2);
                    // a half df is the fp32 value rounded once more: the fp32 product has to exist.  Left to itself the compiler folds the
                    // multiplication into the conversion (v_fma_mixlo_f16: one rounding of the exact product), and where the fp32 value
                    // lies halfway between two halves the result is no longer .to(half) of the fp32 df
                    if constexpr (HOUT) asm volatile("" : "+v"(o[j]));
                }
                store_out<T, HOUT, U>(df, bc * (int64_t)plane + e, o);
            }
        }
    }
}

template <class T, class G, int U, bool MOD>
static int bwd_launch_unit(const NormBwdCall &c, const NormBwdPlan &p, const BwdGeom &a, hipStream_t s)
{
    using E = const typename T::raw *;
    using EG = const typename G::raw *;
    hipLaunchKernelGGL((norm_bwd_reduce_kernel<T, G, U, MOD>), dim3((unsigned)p.grid_reduce), dim3(p.threads_reduce), 0, s, (E)c.f, (EG)c.go, a);
    int rc = launch_check("norm_bwd_reduce_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(norm_bwd_finish_kernel<MOD>, dim3((unsigned)(p.grid_sums + p.grid_dzq)), dim3(kNormBwdThreads), 0, s, a, c.B, (unsigned)p.grid_sums,
                       (float *)c.dgn_weight, (float *)c.dgn_bias, (float *)c.dwy, (float *)c.dby, (float *)c.dwb, (float *)c.dbb, (float *)c.dzq);
    rc = launch_check("norm_bwd_finish_kernel");
    if (rc || !p.grid_apply) return rc;
    const int64_t items = c.B * c.C * p.parts;
    if constexpr (sizeof(typename T::raw) == 2) {
        if (c.df_dtype != CGIC_DT_F32) {
            hipLaunchKernelGGL((norm_bwd_apply_kernel<T, G, true, U, MOD>), dim3((unsigned)p.grid_apply), dim3(kNormThreads), 0, s, (E)c.f, (EG)c.go, a, items,
                               (unsigned)p.parts, (void *)c.df);
            return launch_check("norm_bwd_apply_kernel");
        }
    }
    hipLaunchKernelGGL((norm_bwd_apply_kernel<T, G, false, U, MOD>), dim3((unsigned)p.grid_apply), dim3(kNormThreads), 0, s, (E)c.f, (EG)c.go, a, items,
                       (unsigned)p.parts, (void *)c.df);
    return launch_check("norm_bwd_apply_kernel");
}

template <class T, class G, bool MOD>
static int bwd_launch_typed(const NormBwdCall &c, const NormBwdPlan &p, const BwdGeom &a, hipStream_t s)
{
    if constexpr (sizeof(typename T::raw) == 2)
        if (p.unit == 8) return bwd_launch_unit<T, G, 8, MOD>(c, p, a, s);
    switch (p.unit) {
    case 4: return bwd_launch_unit<T, G, 4, MOD>(c, p, a, s);
    case 2: return bwd_launch_unit<T, G, 2, MOD>(c, p, a, s);
    default: return bwd_launch_unit<T, G, 1, MOD>(c, p, a, s);
    }
}

// the call's types of f and go
template <bool MOD>
static int bwd_launch_call(const NormBwdCall &c, const NormBwdPlan &p, const BwdGeom &a, hipStream_t s)
{
    const bool hgo = c.go_dtype != CGIC_DT_F32;
    if (c.in_dtype == CGIC_DT_F32) return bwd_launch_typed<F32, F32, MOD>(c, p, a, s);
    if (c.in_dtype == CGIC_DT_F16) return hgo ? bwd_launch_typed<F16, F16, MOD>(c, p, a, s) : bwd_launch_typed<F16, F32, MOD>(c, p, a, s);
    return hgo ? bwd_launch_typed<BF16, BF16, MOD>(c, p, a, s) : bwd_launch_typed<BF16, F32, MOD>(c, p, a, s);
}

}  // namespace norm
}  // namespace cgic

using namespace cgic;

// the forward and the training forward (stats != NULL also writes the groups' mean and rstd): the same plan, the same kernels
static int norm_forward(const char *name, bool plain, bool train, const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, const float *zq,
                        int64_t hq, int64_t wq, int groups, double eps, const float *gn_weight, const float *gn_bias, const float *wy,
                        const float *by, const float *wb, const float *bb, int swish, void *out, int out_dtype, float *stats, void *workspace,
                        size_t workspace_bytes, cgic_stream_t stream)
{
    NormCall c{};
    c.in_dtype = in_dtype; c.out_dtype = out_dtype; c.B = B; c.C = C; c.H = H; c.W = W; c.hq = hq; c.wq = wq; c.groups = groups;
    c.f = (uintptr_t)f; c.zq = (uintptr_t)zq; c.gn_weight = (uintptr_t)gn_weight; c.gn_bias = (uintptr_t)gn_bias;
    c.wy = (uintptr_t)wy; c.by = (uintptr_t)by; c.wb = (uintptr_t)wb; c.bb = (uintptr_t)bb; c.out = (uintptr_t)out;
    c.workspace = (uintptr_t)workspace; c.workspace_bytes = workspace_bytes; c.plain = plain;
    NormPlan p;
    const char *why = "";
    const int rc = train ? norm_train_plan(c, (uintptr_t)stats, &p, &why) : norm_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    CGIC_REQUIRE(eps >= 0.0, CGIC_ERR_INVALID, "%s: eps %g", name, eps);
    if (p.form == 0) return CGIC_OK;
    norm::Geom g{};
    g.C = C; g.groups = groups; g.cpg = C / groups; g.H = (int)H; g.W = (int)W; g.hq = (int)hq; g.wq = (int)wq;
    g.ymul = p.ymul; g.ydiv = p.ydiv; g.xmul = p.xmul; g.xdiv = p.xdiv; g.mg_w = p.mg_w; g.mg_y = p.mg_y; g.mg_x = p.mg_x; g.zq_vec = p.zq_vec ? 1 : 0;
    g.swish = swish ? 1 : 0; g.eps = eps;
    g.zq = zq; g.gamma = gn_weight; g.beta = gn_bias; g.wy = wy; g.by = by; g.wb = wb; g.bb = bb;
    const hipStream_t s = (hipStream_t)stream;
    return plain ? norm::launch_call<false>(c, p, g, stats, s) : norm::launch_call<true>(c, p, g, stats, s);
}

extern "C" int cgic_spatial_norm(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, const float *zq, int64_t hq, int64_t wq,
                                 int groups, double eps, const float *gn_weight, const float *gn_bias, const float *wy, const float *by,
                                 const float *wb, const float *bb, int swish, void *out, int out_dtype, void *workspace,
                                 size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_spatial_norm");
    return norm_forward("spatial_norm", false, false, f, in_dtype, B, C, H, W, zq, hq, wq, groups, eps, gn_weight, gn_bias, wy, by, wb, bb, swish, out,
                        out_dtype, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int cgic_spatial_norm_train(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, const float *zq, int64_t hq,
                                       int64_t wq, int groups, double eps, const float *gn_weight, const float *gn_bias, const float *wy,
                                       const float *by, const float *wb, const float *bb, int swish, void *out, int out_dtype, float *stats,
                                       void *workspace, size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_spatial_norm_train");
    return norm_forward("spatial_norm_train", false, true, f, in_dtype, B, C, H, W, zq, hq, wq, groups, eps, gn_weight, gn_bias, wy, by, wb, bb, swish,
                        out, out_dtype, stats, workspace, workspace_bytes, stream);
}

// the plain GroupNorm's calls: no zq, no conv_y / conv_b -- the same plans with the flag set, the kernels' other instantiation
extern "C" int cgic_group_norm(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups, double eps, const float *gn_weight,
                               const float *gn_bias, int swish, void *out, int out_dtype, void *workspace, size_t workspace_bytes,
                               cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_group_norm");
    return norm_forward("group_norm", true, false, f, in_dtype, B, C, H, W, nullptr, 0, 0, groups, eps, gn_weight, gn_bias, nullptr, nullptr, nullptr,
                        nullptr, swish, out, out_dtype, nullptr, workspace, workspace_bytes, stream);
}

extern "C" int cgic_group_norm_train(const void *f, int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups, double eps,
                                     const float *gn_weight, const float *gn_bias, int swish, void *out, int out_dtype, float *stats,
                                     void *workspace, size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_group_norm_train");
    return norm_forward("group_norm_train", true, true, f, in_dtype, B, C, H, W, nullptr, 0, 0, groups, eps, gn_weight, gn_bias, nullptr, nullptr,
                        nullptr, nullptr, swish, out, out_dtype, stats, workspace, workspace_bytes, stream);
}

static int norm_backward(bool plain, const void *f, int in_dtype, const void *go, int go_dtype, int64_t B, int C, int64_t H, int64_t W,
                         const float *zq, int64_t hq, int64_t wq, int groups, const float *stats, const float *gn_weight,
                         const float *gn_bias, const float *wy, const float *by, const float *wb, const float *bb, int swish,
                         void *df, int df_dtype, float *dzq, float *dgn_weight, float *dgn_bias, float *dwy, float *dby,
                         float *dwb, float *dbb, void *workspace, size_t workspace_bytes, cgic_stream_t stream)
{
    NormBwdCall c{};
    c.in_dtype = in_dtype; c.go_dtype = go_dtype; c.df_dtype = df_dtype;
    c.B = B; c.C = C; c.H = H; c.W = W; c.hq = hq; c.wq = wq; c.groups = groups;
    c.f = (uintptr_t)f; c.go = (uintptr_t)go; c.zq = (uintptr_t)zq; c.stats = (uintptr_t)stats; c.gn_weight = (uintptr_t)gn_weight;
    c.gn_bias = (uintptr_t)gn_bias; c.wy = (uintptr_t)wy; c.by = (uintptr_t)by; c.wb = (uintptr_t)wb; c.bb = (uintptr_t)bb;
    c.df = (uintptr_t)df; c.dzq = (uintptr_t)dzq; c.dgn_weight = (uintptr_t)dgn_weight; c.dgn_bias = (uintptr_t)dgn_bias;
    c.dwy = (uintptr_t)dwy; c.dby = (uintptr_t)dby; c.dwb = (uintptr_t)dwb; c.dbb = (uintptr_t)dbb;
    c.workspace = (uintptr_t)workspace; c.workspace_bytes = workspace_bytes; c.plain = plain;
    NormBwdPlan p;
    const char *why = "";
    const int rc = norm_bwd_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    norm::BwdGeom a{};
    norm::Geom &g = a.g;
    g.C = C; g.groups = groups; g.cpg = C / groups; g.H = (int)H; g.W = (int)W; g.hq = (int)hq; g.wq = (int)wq;
    g.ymul = p.ymul; g.ydiv = p.ydiv; g.xmul = p.xmul; g.xdiv = p.xdiv; g.mg_w = p.mg_w; g.mg_y = p.mg_y; g.mg_x = p.mg_x; g.zq_vec = p.zq_vec ? 1 : 0;
    g.swish = swish ? 1 : 0;
    g.zq = zq; g.gamma = gn_weight; g.beta = gn_bias; g.wy = wy; g.by = by; g.wb = wb; g.bb = bb;
    a.stats = stats; a.chan_block = p.chan_block; a.chan_blocks = (int)p.chan_blocks; a.tiles = (int)p.tiles; a.need_dz = p.need_dz ? 1 : 0;
    a.need_conv = p.need_conv ? 1 : 0; a.need_df = p.need_df ? 1 : 0;
    unsigned char *ws = (unsigned char *)workspace;
    a.sums = (double *)(ws + p.off_sums); a.span = (double *)(ws + p.off_span); a.dz = (float *)(ws + p.off_dz);
    const hipStream_t s = (hipStream_t)stream;
    return plain ? norm::bwd_launch_call<false>(c, p, a, s) : norm::bwd_launch_call<true>(c, p, a, s);
}

extern "C" int cgic_spatial_norm_backward(const void *f, int in_dtype, const void *go, int go_dtype, int64_t B, int C, int64_t H, int64_t W,
                                          const float *zq, int64_t hq, int64_t wq, int groups, const float *stats, const float *gn_weight,
                                          const float *gn_bias, const float *wy, const float *by, const float *wb, const float *bb, int swish,
                                          void *df, int df_dtype, float *dzq, float *dgn_weight, float *dgn_bias, float *dwy, float *dby,
                                          float *dwb, float *dbb, void *workspace, size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_spatial_norm_backward");
    return norm_backward(false, f, in_dtype, go, go_dtype, B, C, H, W, zq, hq, wq, groups, stats, gn_weight, gn_bias, wy, by, wb, bb, swish, df, df_dtype,
                         dzq, dgn_weight, dgn_bias, dwy, dby, dwb, dbb, workspace, workspace_bytes, stream);
}

extern "C" int cgic_group_norm_backward(const void *f, int in_dtype, const void *go, int go_dtype, int64_t B, int C, int64_t H, int64_t W, int groups,
                                        const float *stats, const float *gn_weight, const float *gn_bias, int swish, void *df, int df_dtype,
                                        float *dgn_weight, float *dgn_bias, void *workspace, size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_group_norm_backward");
    return norm_backward(true, f, in_dtype, go, go_dtype, B, C, H, W, nullptr, 0, 0, groups, stats, gn_weight, gn_bias, nullptr, nullptr, nullptr, nullptr,
                         swish, df, df_dtype, nullptr, dgn_weight, dgn_bias, nullptr, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

extern "C" size_t cgic_spatial_norm_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormBwdPlan p;
    const char *why = "";
    return norm_bwd_shape(in_dtype, B, C, H, W, groups, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" size_t cgic_group_norm_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormBwdPlan p;
    const char *why = "";
    return norm_bwd_shape(in_dtype, B, C, H, W, groups, &p, &why, true) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" size_t cgic_spatial_norm_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormPlan p;
    const char *why = "";
    return norm_form(in_dtype, B, C, H, W, groups, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" int cgic_spatial_norm_one_launch(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormPlan p;
    const char *why = "";
    const int rc = norm_form(in_dtype, B, C, H, W, groups, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    return p.form == 1 ? 1 : 0;
}
