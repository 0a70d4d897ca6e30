// cgic_merge.hip -- the mask-weighted streams either side of the quantiser, on fp32, fp16 and bf16 features: the encoder's
// three-grain merge (vqvae_blocks.py:361-366), the decoder's two average pools (decoder.py:304-305,366-367) and its two masked blends
// (decoder.py:372-378; 512 channels at the reference's config: 0.5 GB per fp32 tensor at B=64 -- pure HBM streams).  The reference
// materialises the upsampled temporaries; each of these is one pass: read every tensor at its own resolution, write the result
// once.  Under torch.autocast the reference's blend expressions promote to fp32 (the masks are .float()) and AvgPool2d keeps the
// half type; a cast in front of fp32 kernels would read 2 and write 4 bytes per element and operand before the kernel reads them
// again, so the kernels read the halves themselves.  One kernel family for the three feature types:
//   - the upcast is exact (fp32: the bits; bf16: a 16-bit shift; fp16: v_cvt_f32_f16, subnormals kept);
//   - the products, the left-to-right sums and the pool's row-major running sum / (float)(k*k) (the order of ATen's CPU kernel) are
//     the reference's fp32 operations in the reference's order (-ffp-contract=off: no fused multiply-add): bit-identical;
//   - a half output is that fp32 value rounded once to nearest-even (fp16 overflow: +-Inf), a fp32 output is the value itself.
// One thread takes U consecutive x of a row: 16 bytes of the feature type (8 halves, 4 floats) where the width and every pointer's
// alignment allow, else half of that down to 1 -- cgic_merge_plan.h decides, with every check of the eight entry points -- and
// reads everything before it stores, so a blend may run in place.  No LDS, no atomics, grid-stride.
#include "cgic_common.h"
#include "cgic_merge_plan.h"

namespace cgic {

// a feature type: its raw element, the exact upcast and, for a half, the rounding of a fp32 value to it (F32: fp32 out only)
struct F32 {
    using raw = uint32_t;
    static constexpr int widest = 4;                // elements in 16 bytes: the largest unit
    static __device__ __forceinline__ float up(uint32_t v) { return __uint_as_float(v); }
};
struct F16 {
    using raw = uint16_t;
    static constexpr int widest = 8;
    static __device__ __forceinline__ float up(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
    static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
};
struct BF16 {
    using raw = uint16_t;
    static constexpr int widest = 8;
    static __device__ __forceinline__ float up(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
    static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
};

// N consecutive elements as ONE access of their size (two for 32 bytes)
template <int BYTES> struct RawOf;
template <> struct RawOf<2> { using type = uint16_t; };
template <> struct RawOf<4> { using type = uint32_t; };
template <> struct RawOf<8> { using type = uint2; };
template <> struct RawOf<16> { using type = uint4; };

template <class E, int N>
__device__ __forceinline__ void load_f(const E *p, E (&v)[N])
{
    using R = typename RawOf<sizeof(E) * N>::type;
    const R r = *reinterpret_cast<const R *>(p);
    __builtin_memcpy(v, &r, sizeof(R));
}
template <int N>
__device__ __forceinline__ void load_i(const int32_t *p, int32_t (&v)[N])
{
    if constexpr (N == 8) {
        const uint4 lo = *reinterpret_cast<const uint4 *>(p), hi = *reinterpret_cast<const uint4 *>(p + 4);
        __builtin_memcpy(v, &lo, 16);
        __builtin_memcpy(v + 4, &hi, 16);
    } else {
        using R = typename RawOf<4 * N>::type;
        const R r = *reinterpret_cast<const R *>(p);
        __builtin_memcpy(v, &r, sizeof(R));
    }
}
// N results to out[idx ...]: rounded to T's half type (HOUT), or as they are.  PLUS_ZERO: a half result of -0 is stored as +0 (the pool)
template <class T, bool HOUT, int N, bool PLUS_ZERO = false>
__device__ __forceinline__ void store_out(void *out, int64_t idx, const float (&o)[N])
{
    if constexpr (HOUT) {
        using E = typename T::raw;
        using R = typename RawOf<sizeof(E) * N>::type;
        E v[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            v[i] = T::down(o[i]);
            if (PLUS_ZERO && v[i] == 0x8000u) v[i] = 0;
        }
        R r;
        __builtin_memcpy(&r, v, sizeof(R));
        *reinterpret_cast<R *>(reinterpret_cast<E *>(out) + idx) = r;
    } else if constexpr (N == 8) {
        float4 *dst = reinterpret_cast<float4 *>(reinterpret_cast<float *>(out) + idx);
        dst[0] = make_float4(o[0], o[1], o[2], o[3]);
        dst[1] = make_float4(o[4], o[5], o[6], o[7]);
    } else {
        using R = typename RawOf<4 * N>::type;
        R r;
        __builtin_memcpy(&r, o, sizeof(R));
        *reinterpret_cast<R *>(reinterpret_cast<float *>(out) + idx) = r;
    }
}

constexpr int at_least_one(int v) { return v < 1 ? 1 : v; }

// h = up4(hc) * up4(mc) + up2(hm) * up2(mm) + hf * mf on the fine grid [B,C,h,w]; one thread = U consecutive x
template <class T, bool HOUT, int U>
__global__ __launch_bounds__(256) void grain_merge_kernel(
    const typename T::raw *__restrict__ hc, const typename T::raw *__restrict__ hm, const typename T::raw *__restrict__ hf,
    const int32_t *__restrict__ mc, const int32_t *__restrict__ mm, const int32_t *__restrict__ mf, int64_t B, int C, int64_t h,
    int64_t w, void *__restrict__ out)
{
    constexpr int NC = at_least_one(U / 4), NM = at_least_one(U / 2);
    const int64_t w4 = w >> 2, h4 = h >> 2, w2 = w >> 1, h2 = h >> 1, wu = w / U;
    const int64_t total = B * C * h * wu;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xu = t % wu, r = t / wu;
        const int64_t y = r % h, bc = r / h;
        const int64_t b = bc / C;
        const int64_t x = xu * U;
        typename T::raw a[NC], m[NM], f[U];
        int32_t q0[NC], q1[NM], q2[U];
        load_f<typename T::raw, NC>(&hc[(bc * h4 + (y >> 2)) * w4 + (x >> 2)], a);
        load_i<NC>(&mc[(b * h4 + (y >> 2)) * w4 + (x >> 2)], q0);
        load_f<typename T::raw, NM>(&hm[(bc * h2 + (y >> 1)) * w2 + (x >> 1)], m);
        load_i<NM>(&mm[(b * h2 + (y >> 1)) * w2 + (x >> 1)], q1);
        load_f<typename T::raw, U>(&hf[(bc * h + y) * w + x], f);
        load_i<U>(&mf[(b * h + y) * w + x], q2);
        float o[U];
#pragma unroll
        for (int i = 0; i < U; ++i) {
            const int ic = U >= 4 ? i >> 2 : 0, im = U >= 2 ? i >> 1 : 0;
            const float am = T::up(a[ic]) * (float)q0[ic];
            const float pm = T::up(m[im]) * (float)q1[im];
            o[i] = (am + pm) + T::up(f[i]) * (float)q2[i];
        }
        store_out<T, HOUT, U>(out, (bc * h + y) * w + x, o);
    }
}

// x [planes,H,W] -> out [planes,H/K,W/K]: one thread = N adjacent outputs (fp32: 1) = K rows of N * K elements, one access per row (ROWWISE) or
// -- for a pointer that allows no such access -- N = 1 and the window's elements one by one.
// A half result that rounds to -0 (a negative average below half the type's smallest subnormal) is stored as +0: ATen's CPU
// kernel never returns -0 on a half tensor (it adds the rounded average onto a zeroed output element, and 0 + -0 is +0;
// tests/test_merge_half_host.py holds torch to that).  A fp32 result is the value as it is, a -0 included.
template <class T, bool HOUT, int K, int N, bool ROWWISE>
__global__ __launch_bounds__(256) void avgpool_kernel(const typename T::raw *__restrict__ x, int64_t planes, int64_t H, int64_t W,
                                                        void *__restrict__ out)
{
    const int64_t Ho = H / K, Wo = W / K, Wn = Wo / N;
    const int64_t total = planes * Ho * Wn;
    const float div = (float)(K * K);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xn = t % Wn, r = t / Wn;
        const int64_t yo = r % Ho, pl = r / Ho;
        const typename T::raw *src = x + (pl * H + yo * K) * W + xn * (N * K);
        float sum[N];
#pragma unroll
        for (int j = 0; j < N; ++j) sum[j] = 0.f;
#pragma unroll
        for (int dy = 0; dy < K; ++dy) {
            typename T::raw v[N * K];
            if constexpr (ROWWISE) {
                load_f<typename T::raw, N * K>(src + dy * W, v);
            } else {
#pragma unroll
                for (int dx = 0; dx < K; ++dx) v[dx] = src[dy * W + dx];
            }
#pragma unroll
            for (int j = 0; j < N; ++j)
#pragma unroll
                for (int dx = 0; dx < K; ++dx) sum[j] += T::up(v[j * K + dx]);
        }
        float o[N];
#pragma unroll
        for (int j = 0; j < N; ++j) o[j] = sum[j] / div;
        store_out<T, HOUT, N, true>(out, (pl * Ho + yo) * Wo + xn * N, o);
    }
}

// FINE = false: medium grid [B,C,h,w], masks m0 [B,h/2,w/2], m1 [B,h,w]:                  h * up2(m0) + own * m1
// FINE = true : fine grid   [B,C,h,w], masks m0 [B,h/4,w/4], m1 [B,h/2,w/2], m2 [B,h,w]:  h * up4(m0) + h * up2(m1) + own * m2
// out may be hin (no __restrict__ on the two): a thread has read its U elements before it stores them
template <class T, bool HOUT, int U, bool FINE>
__global__ __launch_bounds__(256) void decoder_blend_kernel(
    const typename T::raw *hin, const typename T::raw *__restrict__ own, const int32_t *__restrict__ m0, const int32_t *__restrict__ m1,
    const int32_t *__restrict__ m2, int64_t B, int C, int64_t h, int64_t w, void *out)
{
    constexpr int N4 = at_least_one(U / 4), N2 = at_least_one(U / 2);
    const int64_t wu = w / U;
    const int64_t total = B * C * h * wu;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xu = t % wu, r = t / wu;
        const int64_t y = r % h, bc = r / h;
        const int64_t b = bc / C;
        const int64_t x = xu * U;
        typename T::raw hv[U], ov[U];
        load_f<typename T::raw, U>(&hin[(bc * h + y) * w + x], hv);
        load_f<typename T::raw, U>(&own[(bc * h + y) * w + x], ov);
        float o[U];
        if constexpr (FINE) {
            int32_t q0[N4], q1[N2], q2[U];
            load_i<N4>(&m0[(b * (h >> 2) + (y >> 2)) * (w >> 2) + (x >> 2)], q0);
            load_i<N2>(&m1[(b * (h >> 1) + (y >> 1)) * (w >> 1) + (x >> 1)], q1);
            load_i<U>(&m2[(b * h + y) * w + x], q2);
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int i4 = U >= 4 ? i >> 2 : 0, i2 = U >= 2 ? i >> 1 : 0;
                const float hf = T::up(hv[i]);
                o[i] = (hf * (float)q0[i4] + hf * (float)q1[i2]) + T::up(ov[i]) * (float)q2[i];
            }
        } else {
            int32_t q0[N2], q1[U];
            load_i<N2>(&m0[(b * (h >> 1) + (y >> 1)) * (w >> 1) + (x >> 1)], q0);
            load_i<U>(&m1[(b * h + y) * w + x], q1);
#pragma unroll
            for (int i = 0; i < U; ++i) {
                const int i2 = U >= 2 ? i >> 1 : 0;
                o[i] = T::up(hv[i]) * (float)q0[i2] + T::up(ov[i]) * (float)q1[i];
            }
        }
        store_out<T, HOUT, U>(out, (bc * h + y) * w + x, o);
    }
}

// ---- the launches: the plan's unit and the call's type pair pick the instantiation
template <class T, bool HOUT, int U>
static void launch_one(const MergeCall &c, const MergePlan &p, hipStream_t s)
{
    using E = const typename T::raw *;
    using M = const int32_t *;
    const dim3 grid(p.grid), block(p.threads);
    if (c.op == MH_MERGE)
        hipLaunchKernelGGL((grain_merge_kernel<T, HOUT, U>), grid, block, 0, s, (E)c.feat[0], (E)c.feat[1], (E)c.feat[2], (M)c.mask[0],
                           (M)c.mask[1], (M)c.mask[2], c.B, c.C, c.h, c.w, (void *)c.out);
    else if (c.op == MH_BLEND_FINE)
        hipLaunchKernelGGL((decoder_blend_kernel<T, HOUT, U, true>), grid, block, 0, s, (E)c.feat[0], (E)c.feat[1], (M)c.mask[0],
                           (M)c.mask[1], (M)c.mask[2], c.B, c.C, c.h, c.w, (void *)c.out);
    else
        hipLaunchKernelGGL((decoder_blend_kernel<T, HOUT, U, false>), grid, block, 0, s, (E)c.feat[0], (E)c.feat[1], (M)c.mask[0],
                           (M)c.mask[1], (M) nullptr, c.B, c.C, c.h, c.w, (void *)c.out);
}

template <class T, bool HOUT, int K>
static void launch_pool(const MergeCall &c, const MergePlan &p, hipStream_t s)
{
    const dim3 grid(p.grid), block(p.threads);
#define CGIC_POOL(N, ROWWISE) \
    hipLaunchKernelGGL((avgpool_kernel<T, HOUT, K, N, ROWWISE>), grid, block, 0, s, (const typename T::raw *)c.feat[0], c.B, c.h, c.w, (void *)c.out)
    if (p.unit == 0) CGIC_POOL(1, false);
    else if (p.unit == K) CGIC_POOL(1, true);
    else if constexpr (T::widest == 8) {            // (several outputs per thread: the halves only)
        if (p.unit == 2 * K) CGIC_POOL(2, true);
        else if constexpr (K == 2) CGIC_POOL(4, true);
    }
#undef CGIC_POOL
}

template <class T, bool HOUT>
static void launch_typed(const MergeCall &c, const MergePlan &p, hipStream_t s)
{
    if (c.op == MH_POOL) {
        if (c.k == 4) launch_pool<T, HOUT, 4>(c, p, s);
        else launch_pool<T, HOUT, 2>(c, p, s);
        return;
    }
    if constexpr (T::widest == 8)
        if (p.unit == 8) return launch_one<T, HOUT, 8>(c, p, s);
    switch (p.unit) {
    case 4: launch_one<T, HOUT, 4>(c, p, s); break;
    case 2: launch_one<T, HOUT, 2>(c, p, s); break;
    default: launch_one<T, HOUT, 1>(c, p, s); break;
    }
}

// every entry point: check (the plan), then launch once; a refused call enqueues nothing
static int run(int entry, int op, int in_dtype, int out_dtype, int64_t B, int C, int64_t h, int64_t w, int k, const void *f0, const void *f1,
               const void *f2, const void *m0, const void *m1, const void *m2, void *out, const char *kernel, cgic_stream_t stream)
{
    MergeCall c{};
    c.op = op; c.entry = entry; c.in_dtype = in_dtype; c.out_dtype = out_dtype; c.B = B; c.C = C; c.h = h; c.w = w; c.k = k;
    c.feat[0] = (uintptr_t)f0; c.feat[1] = (uintptr_t)f1; c.feat[2] = (uintptr_t)f2;
    c.mask[0] = (uintptr_t)m0; c.mask[1] = (uintptr_t)m1; c.mask[2] = (uintptr_t)m2;
    c.out = (uintptr_t)out;
    MergePlan p;
    const char *why = "";
    const int rc = merge_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    if (p.grid == 0) return CGIC_OK;
    const hipStream_t s = (hipStream_t)stream;
    const bool hout = out_dtype != CGIC_DT_F32;
    if (in_dtype == CGIC_DT_F32) launch_typed<F32, false>(c, p, s);
    else if (in_dtype == CGIC_DT_F16) hout ? launch_typed<F16, true>(c, p, s) : launch_typed<F16, false>(c, p, s);
    else hout ? launch_typed<BF16, true>(c, p, s) : launch_typed<BF16, false>(c, p, s);
    return launch_check(kernel);
}

}  // namespace cgic

using namespace cgic;

extern "C" int cgic_grain_merge_f32(const float *h_coarse, const float *h_medium, const float *h_fine, const int32_t *mask_c,
                                    const int32_t *mask_m, const int32_t *mask_f, int64_t B, int C, int64_t h, int64_t w, float *out,
                                    cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_grain_merge_f32");
    return run(ME_F32, MH_MERGE, CGIC_DT_F32, CGIC_DT_F32, B, C, h, w, 0, h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f, out,
               "grain_merge_kernel", stream);
}

extern "C" int cgic_grain_merge_h(const void *h_coarse, const void *h_medium, const void *h_fine, int in_dtype, const int32_t *mask_c,
                                  const int32_t *mask_m, const int32_t *mask_f, int64_t B, int C, int64_t h, int64_t w, void *out,
                                  int out_dtype, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_grain_merge_h");
    return run(ME_H, MH_MERGE, in_dtype, out_dtype, B, C, h, w, 0, h_coarse, h_medium, h_fine, mask_c, mask_m, mask_f, out,
               "grain_merge_kernel", stream);
}

extern "C" int cgic_avgpool_f32(const float *x, int64_t planes, int64_t H, int64_t W, int k, float *out, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_avgpool_f32");
    return run(ME_F32, MH_POOL, CGIC_DT_F32, CGIC_DT_F32, planes, 1, H, W, k, x, nullptr, nullptr, nullptr, nullptr, nullptr, out,
               "avgpool_kernel", stream);
}

extern "C" int cgic_avgpool_h(const void *x, int in_dtype, int64_t planes, int64_t H, int64_t W, int k, void *out, int out_dtype,
                              cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_avgpool_h");
    return run(ME_H, MH_POOL, in_dtype, out_dtype, planes, 1, H, W, k, x, nullptr, nullptr, nullptr, nullptr, nullptr, out,
               "avgpool_kernel", stream);
}

extern "C" int cgic_decoder_blend_medium_f32(const float *h, const float *h_medium, const int32_t *mask_c, const int32_t *mask_m,
                                             int64_t B, int C, int64_t hh, int64_t ww, float *out, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_decoder_blend_medium_f32");
    return run(ME_F32, MH_BLEND_MEDIUM, CGIC_DT_F32, CGIC_DT_F32, B, C, hh, ww, 0, h, h_medium, nullptr, mask_c, mask_m, nullptr, out,
               "decoder_blend_kernel<medium>", stream);
}

extern "C" int cgic_decoder_blend_medium_h(const void *h, const void *h_medium, int in_dtype, const int32_t *mask_c,
                                           const int32_t *mask_m, int64_t B, int C, int64_t hh, int64_t ww, void *out, int out_dtype,
                                           cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_decoder_blend_medium_h");
    return run(ME_H, MH_BLEND_MEDIUM, in_dtype, out_dtype, B, C, hh, ww, 0, h, h_medium, nullptr, mask_c, mask_m, nullptr, out,
               "decoder_blend_kernel<medium>", stream);
}

extern "C" int cgic_decoder_blend_fine_f32(const float *h, const float *h_fine, const int32_t *mask_c, const int32_t *mask_m,
                                           const int32_t *mask_f, int64_t B, int C, int64_t hh, int64_t ww, float *out,
                                           cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_decoder_blend_fine_f32");
    return run(ME_F32, MH_BLEND_FINE, CGIC_DT_F32, CGIC_DT_F32, B, C, hh, ww, 0, h, h_fine, nullptr, mask_c, mask_m, mask_f, out,
               "decoder_blend_kernel<fine>", stream);
}

extern "C" int cgic_decoder_blend_fine_h(const void *h, const void *h_fine, int in_dtype, const int32_t *mask_c, const int32_t *mask_m,
                                         const int32_t *mask_f, int64_t B, int C, int64_t hh, int64_t ww, void *out, int out_dtype,
                                         cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_decoder_blend_fine_h");
    return run(ME_H, MH_BLEND_FINE, in_dtype, out_dtype, B, C, hh, ww, 0, h, h_fine, nullptr, mask_c, mask_m, mask_f, out,
               "decoder_blend_kernel<fine>", stream);
}
