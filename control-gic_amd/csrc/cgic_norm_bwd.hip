// cgic_norm_bwd.hip -- the backward of the norm kernels of cgic_norm.hip: cgic_spatial_norm_backward (the decoder's SpatialNorm) and,
// instantiated with MOD = false, cgic_group_norm_backward (the encoder's plain GroupNorm: y = 1, b = 0, no zq).  The device-side
// pieces that both directions use are in cgic_norm_dev.h, every check of a call and its launch plan in cgic_norm_bwd_plan.h.
//
// With go the incoming gradient and mean, rstd the training forward's (stats), per element in fp32, v recomputed as the forward does:
//     xhat = (x - mean) * rstd;  n = xhat * gamma[c] + beta[c];  y, b as above;  v = n * y + b
//     gv = go, with swish go * (s * (1 + v * (1 - s))), s = 1 / (1 + exp(-v));     gn = gv * y;  gy = gv * n
//     df = rstd * ((gamma[c] * gn - S1 / N) - xhat * (S2 / N)),   S1 = sum_c gamma[c] sum_p gn,  S2 = sum_c gamma[c] sum_p gn * xhat
//     dbeta = sum gn, dgamma = sum gn * xhat, dby = sum gy, dbb = sum gv, dwy[k] = sum gy * z_k, dwb[k] = sum gv * z_k   (over b, p)
//     dz_k(b, p) = sum_c wy[c,k] * gy + wb[c,k] * gv, folded through the nearest index into dzq
// Every sum is accumulated in float64 in an order that cgic_norm_bwd_plan.h fixes (three launches ordered by the stream: reduce,
// finish, apply; no atomics), so two calls give the same bits and an image's df and dzq do not depend on its batch.  A NaN in f
// reaches every gradient it reaches in the reference: nothing here selects, clamps or skips by value.
// The plain GroupNorm's terms are these with v = n and gn = gv: on finite inputs the bits of the modulated ones at wy = wb = 0,
// by = 1, bb = 0 (tests/test_group_norm_bwd.py), with no multiplication by that 1 and no addition of that 0.
#include "cgic_norm_bwd_plan.h"
#include "cgic_norm_dev.h"

namespace cgic {
namespace norm {

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

// the terms of element j of a unit; z its zq values (MOD only)
struct Terms {
    float xhat, n, y, gv;           // (y: MOD only)
};
template <bool MOD, int U>
__device__ __forceinline__ Terms bwd_terms(const Chan &w, int swish, float x, float mean, float rstd, float go, const float (&z)[kNormZq][U], int j)
{
    Terms t;
    float bv = 0.f;
    if constexpr (MOD) {
        t.y = w.by;
        bv = w.bb;
#pragma unroll
        for (int k = 0; k < kNormZq; ++k) {
            t.y = t.y + w.wy[k] * z[k][j];
            bv = bv + w.wb[k] * z[k][j];
        }
    }
    t.xhat = (x - mean) * rstd;
    t.n = t.xhat * w.gamma + w.beta;
    t.gv = go;
    if (swish) {
        float v = t.n;
        if constexpr (MOD) v = t.n * t.y + bv;
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
        const Chan w = load_chan<MOD>(g, c);
        if (live) {
            const int64_t at = (b * g.C + c) * (int64_t)plane + e;
            typename T::raw fv[U];
            typename G::raw gov[U];
            load_n<typename T::raw, U>(f + at, fv);
            load_go<typename G::raw, U>(go + at, gov);
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const Terms t = bwd_terms<MOD, U>(w, g.swish, T::up(fv[j]), mean, rstd, G::up(gov[j]), z, j);
                float gn = t.gv;
                [[maybe_unused]] float gy = 0.f;
                if constexpr (MOD) {
                    gn = t.gv * t.y;
                    gy = t.gv * t.n;
                }
                s[0] += (double)gn;
                s[1] += (double)(gn * t.xhat);
                if constexpr (MOD) {
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
        const Chan w = load_chan<MOD>(g, c);
        const float *zq_b = nullptr;
        if constexpr (MOD) zq_b = g.zq + (size_t)b * kNormZq * (unsigned)g.hq * (unsigned)g.wq;
        for (unsigned i = first + threadIdx.x; i < last; i += blockDim.x) {
            const unsigned e = i * U;
            float z[kNormZq][U];
            if constexpr (MOD) {
                const unsigned y = fdiv(e, g.mg_w, (unsigned)g.W), x = e - y * (unsigned)g.W;
                load_z<U>(g, zq_b, y, x, z);
            }
            typename T::raw fv[U];
            typename G::raw gov[U];
            load_n<typename T::raw, U>(f + bc * (int64_t)plane + e, fv);
            load_go<typename G::raw, U>(go + bc * (int64_t)plane + e, gov);
            float o[U];
#pragma unroll
            for (int j = 0; j < U; ++j) {
                const Terms t = bwd_terms<MOD, U>(w, g.swish, T::up(fv[j]), mean, rstd, G::up(gov[j]), z, j);
                float gn = t.gv;
                if constexpr (MOD) gn = t.gv * t.y;
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
    a.g = norm::make_geom(c, p, swish, 0.0);
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
    return norm_bwd_shape("spatial_norm", false, in_dtype, B, C, H, W, groups, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" size_t cgic_group_norm_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t H, int64_t W, int groups)
{
    NormBwdPlan p;
    const char *why = "";
    return norm_bwd_shape("group_norm", true, in_dtype, B, C, H, W, groups, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}
