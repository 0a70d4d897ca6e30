// cgic_attn_bwd.hip -- the backward pass of cgic_attn.hip's attention, again without a tokens x tokens matrix.  With
//     s_ij = scale * sum_c q[c,i] k[c,j],   P_ij = exp(s_ij - lse_i),   delta_i = sum_c go[c,i] out[c,i],   dP_ij = sum_c go[c,i] v[c,j],
//     dS_ij = P_ij (dP_ij - delta_i):
//     dv[c,j] = sum_i go[c,i] P_ij      dq[c,i] = scale sum_j dS_ij k[c,j]      dk[c,j] = scale sum_i dS_ij q[c,i]
// q, k, v, go, out are [C, N] per image with the tokens contiguous, lse is the forward's fp32 [B, N].  cgic_attn_bwd_plan.h holds every
// check and the geometry of the launches; this file is the kernels.  P and dS are recomputed per tile on the chip; all sums are in
// registers; the workspace holds delta alone.
//
//   pre    one thread per token: delta as four interleaved fp32 sums over the channels, added pairwise.
//   dq     the forward's structure: a workgroup of four waves owns 32 queries (q and go transposed in LDS) and walks the keys in
//          tiles of 128.  Per tile, wave w computes S^T and dP^T [its 32 keys][32 queries] over all C channels (A = k resp. v from
//          memory, B = q resp. go from LDS), so the query is the lane and lse_i, delta_i are per-lane scalars; dS goes, rounded once
//          to the operand type, to the LDS tile [query][key]; then wave w owns C / 4 channels of dq^T[channel][query] += K dS^T
//          (A = k's rows straight from memory, B = dS from LDS).
//   dkdv   the roles swapped: a workgroup owns 32 keys (k and v transposed in LDS) and walks the queries in tiles of 128.  Per tile,
//          wave w computes S^T and dP^T [32 keys][its 32 queries] (A = k resp. v from LDS, B = q resp. go from memory: the query is
//          again the lane); P goes to the LDS tile [key][query], wave w adds its C / 4 channels of dv^T[channel][key] += GO P
//          (A = go's rows from memory, B = P from LDS); then dS takes P's place in the same tile and dk^T[channel][key] += Q dS.
// The precision model (tests/attention_bwd_ref.py: grads_model): scores and dP in fp32 from the exactly upcast inputs,
// P = exp2((s * scale - lse) * log2 e) in fp32 and exactly 0 below 2^kNegligible, tail keys and queries 0 by a select, P and dS
// rounded once to the operand type in front of the second products, delta fp32, scale applied once to the finished fp32 sums, a half
// result the fp32 one rounded once.  No atomics, no workgroup waits for another, every sum in a fixed order: two calls give the same
// bits and an image's bits do not depend on B.
#include "cgic_attn_dev.h"
#include "cgic_attn_bwd_plan.h"

namespace cgic {
namespace attn {

constexpr float kLog2e = 1.4426950408889634f;

template <class T>
__device__ __forceinline__ float up(typename T::raw x);
template <>
__device__ __forceinline__ float up<F32>(float x) { return x; }
template <>
__device__ __forceinline__ float up<F16>(uint16_t x) { return (float)__builtin_bit_cast(_Float16, x); }
template <>
__device__ __forceinline__ float up<BF16>(uint16_t x) { return __builtin_bit_cast(float, (uint32_t)x << 16); }

// ---- pre: delta
template <class T>
__global__ __launch_bounds__(kAttnBwdPreThreads) void attn_bwd_delta_kernel(const typename T::raw *__restrict__ go, const typename T::raw *__restrict__ out,
                                                                          int64_t go_stride, int C, int64_t N, unsigned tiles,
                                                                          float *__restrict__ delta)
{
    const unsigned b = blockIdx.x / tiles, t = blockIdx.x - b * tiles;
    const int64_t i = (int64_t)t * kAttnBwdPreThreads + threadIdx.x;
    if (i >= N) return;
    const typename T::raw *g = go + (int64_t)b * go_stride + i, *o = out + (int64_t)b * C * N + i;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    for (int c = 0; c < C; c += 4) {                // (C is 256 or 512)
        s0 = fmaf(up<T>(g[(int64_t)c * N]), up<T>(o[(int64_t)c * N]), s0);
        s1 = fmaf(up<T>(g[(int64_t)(c + 1) * N]), up<T>(o[(int64_t)(c + 1) * N]), s1);
        s2 = fmaf(up<T>(g[(int64_t)(c + 2) * N]), up<T>(o[(int64_t)(c + 2) * N]), s2);
        s3 = fmaf(up<T>(g[(int64_t)(c + 3) * N]), up<T>(o[(int64_t)(c + 3) * N]), s3);
    }
    delta[(int64_t)b * N + i] = (s0 + s1) + (s2 + s3);
}

// [32][32] = sum over all C channels of one operand read from memory (`mem`: this lane's token, its first channel; channels N
// apart; zeros when the token is past the end) and one read from a transposed LDS image (`lds`: this lane's row, its first channel).
// MEM_IS_A: the memory operand's token is the row of the result, else its column (the lane).  fp32: four chains as in the forward.
template <class T, int C, bool MEM_IS_A>
__device__ __forceinline__ f32x16 over_channels(const typename T::raw *mem, int64_t N, bool ok, const typename T::raw *lds)
{
    using frag = typename T::frag;
    f32x16 sc[T::CHAINS];
#pragma unroll
    for (int ch = 0; ch < T::CHAINS; ++ch)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[ch][r] = 0.f;
    static_assert((C / T::KS) % (8 * T::CHAINS) == 0 || T::CHAINS == 1, "whole rounds of the chains");
    // (two rounds in flight: a half fragment from memory is 8 element loads, and eight rounds of them spilled)
#pragma unroll 2
    for (int st = 0; st < C / T::KS; st += T::CHAINS) {
#pragma unroll
        for (int ch = 0; ch < T::CHAINS; ++ch) {
            const frag m = load_strided<T>(mem + (int64_t)((st + ch) * T::KS) * N, N, ok);
            const frag s = lds_frag<T>(lds + (st + ch) * T::KS);
            if constexpr (MEM_IS_A) sc[ch] = T::mma(m, s, sc[ch]);
            else sc[ch] = T::mma(s, m, sc[ch]);
        }
    }
    static_assert(T::CHAINS == 1 || T::CHAINS == 4, "the pairwise sum below");
    if constexpr (T::CHAINS == 4) return (sc[0] + sc[1]) + (sc[2] + sc[3]);
    else return sc[0];
}

// acc[t] (this wave's channels 32 t .. 32 t + 31 of its quarter, by this lane's column) += rows of `mem` (a [C, N] image: channel
// rows, the tile's tokens from t0 on) times the LDS tile `tile` (this lane's row: its column's weights along the tile's tokens)
template <class T, int C, bool VEC>
__device__ __forceinline__ void over_tile(f32x16 (&acc)[C / (32 * kAttnWaves)], const typename T::raw *mem, int64_t N, int64_t t0, int w, int j, int h,
                                          const typename T::raw *tile)
{
    using frag = typename T::frag;
    constexpr int CT = C / (32 * kAttnWaves);
    const typename T::raw *pp = tile + T::EL * h;
#pragma unroll T::EL == 1 ? 4 : 2
    for (int st = 0; st < kAttnBK / T::KS; ++st) {
        const int64_t tt = t0 + st * T::KS;
        if (tt >= N) break;                                     // (uniform over the workgroup: the remaining weights are zeros)
        const int64_t left = N - (tt + T::EL * h);
        const int valid = left >= T::EL ? T::EL : left > 0 ? (int)left : 0;
        const frag bp = lds_frag<T>(pp + st * T::KS);
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const int ch = w * (C / kAttnWaves) + 32 * t + j;
            const frag a = load_row<T, VEC>(mem + (int64_t)ch * N + tt + T::EL * h, valid);
            acc[t] = T::mma(a, bp, acc[t]);
        }
    }
}

// this wave's channels of a [C, N] gradient image, `mul` times the accumulators (the scale; 1 for dv: exact), at the token of this lane
template <class T, int C>
__device__ __forceinline__ void store_grad(const f32x16 (&acc)[C / (32 * kAttnWaves)], float mul, void *__restrict__ dst, bool half_out,
                                           int64_t image, int64_t N, int64_t token, int w, int h)
{
    using raw = typename T::raw;
    constexpr int CT = C / (32 * kAttnWaves);
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = w * (C / kAttnWaves) + 32 * t + tile_row(r, h);
            const int64_t at = (image * C + ch) * N + token;
            float o = acc[t][r] * mul;
            if (half_out) {
                // a half gradient is the fp32 value rounded once more: the fp32 product has to exist (left to itself the compiler
                // folds the multiply into the conversion)
                asm volatile("" : "+v"(o));
                reinterpret_cast<raw *>(dst)[at] = T::down(o);
            } else {
                reinterpret_cast<float *>(dst)[at] = o;
            }
        }
}

template <class T, int C>
__device__ __forceinline__ void zero(f32x16 (&acc)[C / (32 * kAttnWaves)])
{
#pragma unroll
    for (int t = 0; t < C / (32 * kAttnWaves); ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// P of one score: exactly 0 below 2^kNegligible; a NaN exponent compares false and goes through exp2
__device__ __forceinline__ float weight(float s, float scale, float lse)
{
    const float x = (s * scale - lse) * kLog2e;
    return !(x < kNegligible) ? exp2_above_negligible(x) : 0.f;
}

// ---- dq
template <class T, int C, bool VEC>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dq_kernel(const typename T::raw *__restrict__ go, const typename T::raw *__restrict__ q,
                                                                  const typename T::raw *__restrict__ k, const typename T::raw *__restrict__ v,
                                                                  const float *__restrict__ lse, const float *__restrict__ delta, int64_t go_stride,
                                                                  int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t N, unsigned tiles,
                                                                  float scale, void *__restrict__ dq, int half_out)
{
    using raw = typename T::raw;
    constexpr int ROW = C + T::PAD, TROW = kAttnBK + T::PAD, CT = C / (32 * kAttnWaves);
    static_assert(C % (32 * kAttnWaves) == 0 && C % T::KS == 0 && kAttnBK % T::KS == 0, "whole MFMA tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_bwd_smem[];
    raw *Qs = reinterpret_cast<raw *>(attn_bwd_smem);       // [32 queries][ROW]: q transposed, channels along the row
    raw *Gs = Qs + kAttnBQ * ROW;                           // [32 queries][ROW]: go transposed
    raw *Ds = Gs + kAttnBQ * ROW;                           // [32 queries][TROW]: the tile's dS, keys along the row

    const unsigned b = blockIdx.x / tiles, qt = blockIdx.x - b * tiles;
    const int64_t q0 = (int64_t)qt * kAttnBQ;
    const int tid = (int)threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 31, h = l >> 5;
    const raw *qi = q + (int64_t)b * q_stride, *gi = go + (int64_t)b * go_stride, *ki = k + (int64_t)b * k_stride, *vi = v + (int64_t)b * v_stride;
    const bool q_ok = q0 + j < N;

    for (int i = tid; i < C * kAttnBQ; i += kAttnThreads) {     // (a tail query reads as zeros and is never stored)
        const int c = i >> 5, jj = i & 31;
        const bool ok = q0 + jj < N;
        Qs[jj * ROW + c] = ok ? qi[(int64_t)c * N + q0 + jj] : (raw)0;
        Gs[jj * ROW + c] = ok ? gi[(int64_t)c * N + q0 + jj] : (raw)0;
    }
    const float lse_i = q_ok ? lse[(int64_t)b * N + q0 + j] : 0.f;
    const float delta_i = q_ok ? delta[(int64_t)b * N + q0 + j] : 0.f;
    __syncthreads();

    f32x16 acc[CT];
    zero<T, C>(acc);
    const int64_t k_tiles = (N + kAttnBK - 1) / kAttnBK;
    for (int64_t kt = 0; kt < k_tiles; ++kt) {
        const int64_t k0 = kt * kAttnBK, kw = k0 + 32 * w;      // the tile's and this wave's first key
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
        if (kw < N) {                                           // (wave-uniform; a quarter that is all tail is masked below anyway)
            const int64_t key = kw + j;
            s = over_channels<T, C, true>(ki + (int64_t)(T::EL * h) * N + key, N, key < N, Qs + j * ROW + T::EL * h);
            dp = over_channels<T, C, true>(vi + (int64_t)(T::EL * h) * N + key, N, key < N, Gs + j * ROW + T::EL * h);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile_row(r, h);
            const float ds = weight(s[r], scale, lse_i) * (dp[r] - delta_i);
            Ds[j * TROW + 32 * w + row] = T::down(q_ok && kw + row < N ? ds : 0.f);
        }
        __syncthreads();
        over_tile<T, C, VEC>(acc, ki, N, k0, w, j, h, Ds + j * TROW);
        __syncthreads();                                        // (the next tile's dS follows these reads)
    }
    if (q_ok) store_grad<T, C>(acc, scale, dq, half_out != 0, (int64_t)b, N, q0 + j, w, h);
}

// ---- dk, dv
template <class T, int C, bool VEC>
__global__ __launch_bounds__(kAttnThreads) void attn_bwd_dkdv_kernel(const typename T::raw *__restrict__ go, const typename T::raw *__restrict__ q,
                                                                    const typename T::raw *__restrict__ k, const typename T::raw *__restrict__ v,
                                                                    const float *__restrict__ lse, const float *__restrict__ delta, int64_t go_stride,
                                                                    int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t N, unsigned tiles,
                                                                    float scale, void *__restrict__ dk, void *__restrict__ dv, int half_out)
{
    using raw = typename T::raw;
    constexpr int ROW = C + T::PAD, TROW = kAttnBwdBQT + T::PAD, CT = C / (32 * kAttnWaves);
    static_assert(kAttnBwdBQT == kAttnBK, "over_tile walks a tile of kAttnBK tokens");
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_bwd_smem[];
    raw *Ks = reinterpret_cast<raw *>(attn_bwd_smem);       // [32 keys][ROW]: k transposed, channels along the row
    raw *Vs = Ks + kAttnBwdBK * ROW;                        // [32 keys][ROW]: v transposed
    raw *Ts = Vs + kAttnBwdBK * ROW;                        // [32 keys][TROW]: the tile's P, then its dS, queries along the row

    const unsigned b = blockIdx.x / tiles, kt = blockIdx.x - b * tiles;
    const int64_t key0 = (int64_t)kt * kAttnBwdBK;
    const int tid = (int)threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 31, h = l >> 5;
    const raw *qi = q + (int64_t)b * q_stride, *gi = go + (int64_t)b * go_stride, *ki = k + (int64_t)b * k_stride, *vi = v + (int64_t)b * v_stride;
    const bool want_dk = dk != nullptr, want_dv = dv != nullptr;

    for (int i = tid; i < C * kAttnBwdBK; i += kAttnThreads) {  // (a tail key reads as zeros and is never stored)
        const int c = i >> 5, jj = i & 31;
        const bool ok = key0 + jj < N;
        Ks[jj * ROW + c] = ok ? ki[(int64_t)c * N + key0 + jj] : (raw)0;
        Vs[jj * ROW + c] = ok ? vi[(int64_t)c * N + key0 + jj] : (raw)0;
    }
    __syncthreads();

    f32x16 acc_k[CT], acc_v[CT];
    zero<T, C>(acc_k);
    zero<T, C>(acc_v);
    const int64_t q_tiles = (N + kAttnBwdBQT - 1) / kAttnBwdBQT;
    for (int64_t qt = 0; qt < q_tiles; ++qt) {
        const int64_t qb = qt * kAttnBwdBQT, qw = qb + 32 * w;  // the tile's and this wave's first query
        const int64_t query = qw + j;
        const bool q_ok = query < N;
        const float lse_i = q_ok ? lse[(int64_t)b * N + query] : 0.f;
        const float delta_i = q_ok && want_dk ? delta[(int64_t)b * N + query] : 0.f;
        f32x16 s, dp;
#pragma unroll
        for (int r = 0; r < 16; ++r) { s[r] = 0.f; dp[r] = 0.f; }
        if (qw < N) {                                           // (wave-uniform)
            s = over_channels<T, C, false>(qi + (int64_t)(T::EL * h) * N + query, N, q_ok, Ks + j * ROW + T::EL * h);
            if (want_dk) dp = over_channels<T, C, false>(gi + (int64_t)(T::EL * h) * N + query, N, q_ok, Vs + j * ROW + T::EL * h);
        }
        float p[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = q_ok && key0 + tile_row(r, h) < N ? weight(s[r], scale, lse_i) : 0.f;
        if (want_dv) {
#pragma unroll
            for (int r = 0; r < 16; ++r) Ts[tile_row(r, h) * TROW + 32 * w + j] = T::down(p[r]);
            __syncthreads();
            over_tile<T, C, VEC>(acc_v, gi, N, qb, w, j, h, Ts + j * TROW);
            __syncthreads();                                    // (dS, or the next tile's P, follows these reads)
        }
        if (want_dk) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float ds = p[r] * (dp[r] - delta_i);
                Ts[tile_row(r, h) * TROW + 32 * w + j] = T::down(q_ok && key0 + tile_row(r, h) < N ? ds : 0.f);
            }
            __syncthreads();
            over_tile<T, C, VEC>(acc_k, qi, N, qb, w, j, h, Ts + j * TROW);
            __syncthreads();
        }
    }
    if (key0 + j < N) {
        if (want_dv) store_grad<T, C>(acc_v, 1.f, dv, half_out != 0, (int64_t)b, N, key0 + j, w, h);
        if (want_dk) store_grad<T, C>(acc_k, scale, dk, half_out != 0, (int64_t)b, N, key0 + j, w, h);
    }
}

template <class T, int C, bool DQ_VEC, bool DKDV_VEC>
static int launch_one(const AttnBwdCall &c, const AttnBwdPlan &p, hipStream_t s)
{
    using E = const typename T::raw *;
    float *delta = (float *)c.workspace;
    const float scale = (float)c.scale;
    const int half_out = c.grad_dtype != CGIC_DT_F32;
    if (p.pre.run) {
        hipLaunchKernelGGL(attn_bwd_delta_kernel<T>, dim3((unsigned)p.pre.grid), dim3(p.pre.threads), 0, s, (E)c.go, (E)c.out, c.go_batch_stride, (int)c.C,
                           c.N, (unsigned)p.pre.tiles, delta);
        const int rc = launch_check("attn_bwd_delta_kernel");
        if (rc) return rc;
    }
    if (p.dq.run) {
        const auto kernel = attn_bwd_dq_kernel<T, C, DQ_VEC>;
        int rc = ensure_lds_above_48k((const void *)kernel, p.dq.lds_bytes);
        if (rc) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.dq.grid), dim3(p.dq.threads), p.dq.lds_bytes, s, (E)c.go, (E)c.q, (E)c.k, (E)c.v, (const float *)c.lse,
                           (const float *)delta, c.go_batch_stride, c.q_batch_stride, c.k_batch_stride, c.v_batch_stride, c.N, (unsigned)p.dq.tiles, scale,
                           (void *)c.dq, half_out);
        rc = launch_check("attn_bwd_dq_kernel");
        if (rc) return rc;
    }
    if (p.dkdv.run) {
        const auto kernel = attn_bwd_dkdv_kernel<T, C, DKDV_VEC>;
        int rc = ensure_lds_above_48k((const void *)kernel, p.dkdv.lds_bytes);
        if (rc) return rc;
        hipLaunchKernelGGL(kernel, dim3((unsigned)p.dkdv.grid), dim3(p.dkdv.threads), p.dkdv.lds_bytes, s, (E)c.go, (E)c.q, (E)c.k, (E)c.v,
                           (const float *)c.lse, (const float *)delta, c.go_batch_stride, c.q_batch_stride, c.k_batch_stride, c.v_batch_stride, c.N,
                           (unsigned)p.dkdv.tiles, scale, (void *)c.dk, (void *)c.dv, half_out);
        rc = launch_check("attn_bwd_dkdv_kernel");
        if (rc) return rc;
    }
    return CGIC_OK;
}

template <class T, bool DQ_VEC, bool DKDV_VEC>
static int launch_width(const AttnBwdCall &c, const AttnBwdPlan &p, hipStream_t s)
{
    static_assert(attn_width_built(256) && attn_width_built(512), "the plan admits what is instantiated here");
    return c.C == 256 ? launch_one<T, 256, DQ_VEC, DKDV_VEC>(c, p, s) : launch_one<T, 512, DQ_VEC, DKDV_VEC>(c, p, s);
}

template <class T>
static int launch_half(const AttnBwdCall &c, const AttnBwdPlan &p, hipStream_t s)
{
    if (p.dq_vec) return p.dkdv_vec ? launch_width<T, true, true>(c, p, s) : launch_width<T, true, false>(c, p, s);
    return p.dkdv_vec ? launch_width<T, false, true>(c, p, s) : launch_width<T, false, false>(c, p, s);
}

}  // namespace attn
}  // namespace cgic

using namespace cgic;

extern "C" int cgic_attention_backward(const void *go, const void *q, const void *k, const void *v, const void *out, const float *lse, int in_dtype,
                                       int64_t B, int C, int64_t N, int64_t go_batch_stride, int64_t q_batch_stride, int64_t k_batch_stride,
                                       int64_t v_batch_stride, double scale, void *dq, void *dk, void *dv, int grad_dtype, void *workspace,
                                       size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_attention_backward");
    AttnBwdCall c{};
    c.in_dtype = in_dtype; c.grad_dtype = grad_dtype; c.B = B; c.C = C; c.N = N;
    c.go_batch_stride = go_batch_stride; c.q_batch_stride = q_batch_stride; c.k_batch_stride = k_batch_stride; c.v_batch_stride = v_batch_stride;
    c.scale = scale;
    c.go = (uintptr_t)go; c.q = (uintptr_t)q; c.k = (uintptr_t)k; c.v = (uintptr_t)v; c.out = (uintptr_t)out; c.lse = (uintptr_t)lse;
    c.dq = (uintptr_t)dq; c.dk = (uintptr_t)dk; c.dv = (uintptr_t)dv;
    c.workspace = (uintptr_t)workspace; c.workspace_bytes = workspace_bytes;
    AttnBwdPlan p;
    const char *why = "";
    const int rc = attn_bwd_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    if (p.form == 0) return CGIC_OK;
    const hipStream_t s = (hipStream_t)stream;
    if (in_dtype == CGIC_DT_F32) return attn::launch_width<attn::F32, false, false>(c, p, s);
    if (in_dtype == CGIC_DT_F16) return attn::launch_half<attn::F16>(c, p, s);
    return attn::launch_half<attn::BF16>(c, p, s);
}

extern "C" size_t cgic_attention_backward_workspace_bytes(int in_dtype, int64_t B, int C, int64_t N)
{
    AttnBwdPlan p;
    const char *why = "";
    return attn_bwd_form(in_dtype, in_dtype, B, C, N, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" int cgic_attention_backward_supported(int in_dtype, int grad_dtype, int64_t B, int C, int64_t N)
{
    AttnBwdPlan p;
    const char *why = "";
    const int rc = attn_bwd_form(in_dtype, grad_dtype, B, C, N, &p, &why);
    if (rc == CGIC_ERR_UNSUPPORTED) return 0;
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    return 1;
}
