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
#include "cgic_norm_bwd_plan.h"
#include "cgic_norm_dev.h"

namespace cgic {
namespace norm {

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

// units [first, end) of one channel's plane, `step` apart: src is the plane (in global memory or in LDS), out_plane the index of
// its first element in out, zq_b the image's zq.  Without MOD the element is n, and nothing of zq is indexed or read
template <class T, bool HOUT, int U, bool MOD>
__device__ __forceinline__ void apply_units(const typename T::raw *src, void *out, int64_t out_plane, unsigned first, unsigned end,
                                            unsigned step, const Geom &g, const float *zq_b, const Chan &w, float mean, float rstd)
{
    const unsigned W = (unsigned)g.W, plane_q = (unsigned)g.hq * (unsigned)g.wq;
    for (unsigned i = first; i < end; i += step) {
        const unsigned e = i * U;
        [[maybe_unused]] unsigned x = 0, sy = 0;      // (MOD: the unit's place in its row, the row of zq under it)
        if constexpr (MOD) {
            const unsigned y = fdiv(e, g.mg_w, W);
            x = e - y * W;
            sy = fdiv(y * (unsigned)g.ymul, g.mg_y, (unsigned)g.ydiv);
        }
        typename T::raw v[U];
        load_n<typename T::raw, U>(src + e, v);
        float o[U];
        const auto element = [&](int j, float yv, float bv) {
            float val = ((T::up(v[j]) - mean) * rstd) * w.gamma + w.beta;
            if constexpr (MOD) val = val * yv + bv;
            if (g.swish) val = val / (1.0f + expf(-val));
            o[j] = val;
        };
        if constexpr (!MOD) {
#pragma unroll
            for (int j = 0; j < U; ++j) element(j, 0.f, 0.f);
        } else {
            const float *zrow = zq_b + (size_t)sy * (unsigned)g.wq;
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
                    if (j == 0 || rem == 0) {       // a new zq pixel: its four values once, for every x that falls on it
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
        }
        store_out<T, HOUT, U>(out, out_plane + e, o);
    }
}

// channel c of image b: its parameters, the image's zq
template <class T, bool HOUT, int U, bool MOD>
__device__ __forceinline__ void apply_channel(const typename T::raw *src, void *out, int64_t out_plane, unsigned first, unsigned end, unsigned step,
                                              const Geom &g, int64_t b, int c, float mean, float rstd)
{
    const Chan w = load_chan<MOD>(g, c);
    apply_units<T, HOUT, U, MOD>(src, out, out_plane, first, end, step, g, g.zq + (size_t)b * kNormZq * (unsigned)g.hq * (unsigned)g.wq, w, mean, rstd);
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
    const norm::Geom g = norm::make_geom(c, p, swish, eps);
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

extern "C" size_t cgic_spatial_norm_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormPlan p;
    const char *why = "";
    return norm_form("spatial_norm", in_dtype, B, C, H, W, groups, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" int cgic_spatial_norm_one_launch(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormPlan p;
    const char *why = "";
    const int rc = norm_form("spatial_norm", in_dtype, B, C, H, W, groups, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    return p.form == 1 ? 1 : 0;
}
