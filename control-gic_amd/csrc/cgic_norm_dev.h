// cgic_norm_dev.h -- the device-side pieces that the norm kernels share (cgic_norm.hip: the forward and the training forward;
// cgic_norm_bwd.hip: the backward): the feature types, the accesses of N consecutive elements, the division by a magic multiplier,
// what a kernel knows of a call (Geom, filled by make_geom from the plan's geometry and the call's pointers) and of a channel (Chan).
// MOD is the modulated layer (SpatialNorm); without it (the plain GroupNorm) nothing of zq, conv_y or conv_b is loaded or computed.
#pragma once
#include "cgic_common.h"
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

// the Geom of a call (a NormCall or a NormBwdCall; the plain one's hq, wq and five pointers are 0) from its plan's zq geometry
template <class Call>
inline Geom make_geom(const Call &c, const NormZqGeom &q, int swish, double eps)
{
    Geom g{};
    g.C = (int)c.C; g.groups = (int)c.groups; g.cpg = (int)(c.C / c.groups); g.H = (int)c.H; g.W = (int)c.W; g.hq = (int)c.hq; g.wq = (int)c.wq;
    g.ymul = q.ymul; g.ydiv = q.ydiv; g.xmul = q.xmul; g.xdiv = q.xdiv; g.mg_w = q.mg_w; g.mg_y = q.mg_y; g.mg_x = q.mg_x; g.zq_vec = q.zq_vec ? 1 : 0;
    g.swish = swish ? 1 : 0; g.eps = eps;
    g.zq = (const float *)c.zq; g.gamma = (const float *)c.gn_weight; g.beta = (const float *)c.gn_bias;
    g.wy = (const float *)c.wy; g.by = (const float *)c.by; g.wb = (const float *)c.wb; g.bb = (const float *)c.bb;
    return g;
}

// the parameters of a channel -- gamma and beta, and the ten of conv_y and conv_b with MOD; c is uniform where this is called, so
// these are scalar loads
struct Chan {
    float gamma, beta, by, bb, wy[kNormZq], wb[kNormZq];
};
template <bool MOD>
__device__ __forceinline__ Chan load_chan(const Geom &g, int c)
{
    Chan w;
    w.gamma = g.gamma[c]; w.beta = g.beta[c];
    if constexpr (MOD) {
        w.by = g.by[c]; w.bb = g.bb[c];
#pragma unroll
        for (int k = 0; k < kNormZq; ++k) { w.wy[k] = g.wy[c * kNormZq + k]; w.wb[k] = g.wb[c * kNormZq + k]; }
    }
    return w;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;                                       // (lane 0 holds the wave's sum)
}

}  // namespace norm
}  // namespace cgic
