// cgic_attn.hip -- AttnBlock's attention (CGIC/modules/vqvae/decoder.py:189-213, vqvae_blocks.py:168-193) without the
// tokens x tokens matrix:
//     w = softmax_j(scale * sum_c q[c,i] k[c,j]);   out[c,i] = sum_j v[c,j] w[i,j]
// one head as wide as the channel count C, q / k / v / out all [C, N] per image with the tokens contiguous (what the 1x1 convs
// return and what proj_out takes).  cgic_attn_plan.h holds every check and the launch geometry; this file is the kernel.
//
// A workgroup of four waves owns 32 queries of one image and walks the keys in tiles of 128.  Per tile:
//   1. wave w computes S^T[32 keys of its quarter][32 queries] = K^T Q over all C channels (MFMA, A = k, B = q from LDS).  The
//      swapped product leaves the QUERY on the lane (column) and the keys in the 16 result registers, so the running maximum, the
//      rescale factor and the row sum are per-lane scalars.
//   2. the four waves exchange their 32 per-query maxima through LDS; every wave computes the same new maximum from the same four
//      numbers, the weights p = exp2((s - m) * scale * log2 e) in fp32, and writes them, rounded once to the operand type, to the
//      LDS tile P[query][key].  Tail keys get p = 0 by a select (not through exp), and are kept out of the maximum as -inf.
//      v_max_f32 drops a NaN, so a NaN score arrives through exp2: the query becomes NaN, as in torch.  A -inf score weighs 0, also
//      while the maximum itself is still -inf (a leading tile whose keys all score -inf: 0 is subtracted in place of the maximum);
//      a query whose every key scores -inf ends as 0 / 0 = NaN, one with a +inf score as exp2(inf - inf) = NaN, both as in torch.
//   3. wave w owns C / 4 channels of O^T[channel][query] += V[channel][128 keys] P^T (MFMA, A = v straight from memory -- a lane's
//      keys of a channel are consecutive there --, B = P from LDS); the accumulator's column is again the query, so the rescale
//      of step 2 is a per-lane multiply.
// The row sums stay per lane (8 partials per query: 4 waves x 2 lane halves) and are added in a fixed order at the end.  Nothing
// depends on which workgroup ran a tile or on B: an image's bits are a function of its own q, k, v alone.  No atomics, no waiting.
//
// fp32 inputs run the same kernel on v_mfma_f32_32x32x2_f32 (exact fp32 products, one element per lane and k-step); fp16 / bf16 on
// v_mfma_f32_32x32x16_{f16,bf16} (8 elements per lane and k-step), scores / statistics / accumulator in fp32.
#include "cgic_attn_dev.h"

namespace cgic {
namespace attn {

template <class T, int C, bool HOUT, bool VEC>
__global__ __launch_bounds__(kAttnThreads) void attn_kernel(const typename T::raw *__restrict__ q, const typename T::raw *__restrict__ k,
                                                           const typename T::raw *__restrict__ v, int64_t q_stride, int64_t k_stride,
                                                           int64_t v_stride, int64_t N, unsigned q_tiles, float c2, double scale,
                                                           void *__restrict__ out, float *__restrict__ lse)
{
    using raw = typename T::raw;
    using frag = typename T::frag;
    constexpr int QROW = C + T::PAD, PROW = kAttnBK + T::PAD, CT = C / (32 * kAttnWaves);
    static_assert(C % (32 * kAttnWaves) == 0 && C % T::KS == 0 && kAttnBK % T::KS == 0, "whole MFMA tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char attn_smem[];
    raw *Qs = reinterpret_cast<raw *>(attn_smem);           // [32 queries][QROW]: q transposed, channels along the row
    raw *Ps = Qs + kAttnBQ * QROW;                          // [32 queries][PROW]: the tile's weights, keys along the row
    float *stat = reinterpret_cast<float *>(Ps + kAttnBQ * PROW);      // [8][32]

    const unsigned b = blockIdx.x / q_tiles, qt = blockIdx.x - b * q_tiles;
    const int64_t q0 = (int64_t)qt * kAttnBQ;
    const int tid = (int)threadIdx.x, w = tid >> 6, l = tid & 63, j = l & 31, h = l >> 5;
    const raw *qi = q + (int64_t)b * q_stride, *ki = k + (int64_t)b * k_stride, *vi = v + (int64_t)b * v_stride;
    const bool q_ok = q0 + j < N;

    // ---- the 32 queries, transposed into LDS (a tail query reads as zeros and is never stored)
    for (int i = tid; i < C * kAttnBQ; i += kAttnThreads) {
        const int c = i >> 5, jj = i & 31;
        Qs[jj * QROW + c] = q0 + jj < N ? qi[(int64_t)c * N + q0 + jj] : (raw)0;
    }
    __syncthreads();

    float m = -INFINITY, lsum = 0.f;
    f32x16 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int64_t k_tiles = (N + kAttnBK - 1) / kAttnBK;
    for (int64_t kt = 0; kt < k_tiles; ++kt) {
        const int64_t k0 = kt * kAttnBK, kw = k0 + 32 * w;      // the tile's and this wave's first key
        // ---- 1. scores of this wave's 32 keys against the 32 queries
        f32x16 sc[T::CHAINS];
#pragma unroll
        for (int ch = 0; ch < T::CHAINS; ++ch)
#pragma unroll
            for (int r = 0; r < 16; ++r) sc[ch][r] = 0.f;
        if (kw < N) {                                           // (wave-uniform; a quarter that is all tail is masked below anyway)
            const int64_t key = kw + j;
            const bool k_ok = key < N;
            const raw *kp = ki + (int64_t)(T::EL * h) * N + key;
            const raw *qp = Qs + j * QROW + T::EL * h;
            static_assert((C / T::KS) % (8 * T::CHAINS) == 0 || T::CHAINS == 1, "whole rounds of the chains");
#pragma unroll 8 / T::CHAINS
            for (int st = 0; st < C / T::KS; st += T::CHAINS) {
#pragma unroll
                for (int ch = 0; ch < T::CHAINS; ++ch) {
                    const frag a = load_strided<T>(kp + (int64_t)((st + ch) * T::KS) * N, N, k_ok);
                    const frag bq = lds_frag<T>(qp + (st + ch) * T::KS);
                    sc[ch] = T::mma(a, bq, sc[ch]);
                }
            }
        }
        f32x16 s;
        if constexpr (T::CHAINS == 4) s = (sc[0] + sc[1]) + (sc[2] + sc[3]);
        else s = sc[0];
        static_assert(T::CHAINS == 1 || T::CHAINS == 4, "the pairwise sum above");
        // ---- 2. the tile's maximum per query, over the four waves
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, kw + tile_row(r, h) < N ? s[r] : -INFINITY);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
        if (h == 0) stat[w * 32 + j] = tmax;
        __syncthreads();
        const float mn = fmaxf(fmaxf(m, fmaxf(stat[j], stat[32 + j])), fmaxf(stat[64 + j], stat[96 + j]));
        // (0 at the first tile, by a select: m is -inf there, and -inf * c2 is NaN when the scale is 0 or so small that c2 rounds to 0)
        // (... and 0 where it is below 2^-64, like a weight below: see kNegligible)
        const float ax = (m - mn) * c2;
        const float alpha = m == -INFINITY || ax < kNegligible ? 0.f : exp2_above_negligible(ax);
        // (the maximum is still -inf when every key so far scored -inf for this query: s - mn would be NaN.  Against 0 such a key
        //  weighs exp2(-inf) = 0, as in the reference; a NaN score stays NaN, and so does -inf * c2 when the scale is 0)
        const float sub = mn == -INFINITY ? 0.f : mn;
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = tile_row(r, h);
            const float x = (s[r] - sub) * c2;
            const float p = kw + row < N && !(x < kNegligible) ? exp2_above_negligible(x) : 0.f;     // (a NaN exponent compares false and goes through exp2)
            psum += p;
            Ps[j * PROW + 32 * w + row] = T::down(p);
        }
        lsum = lsum * alpha + psum;
        m = mn;
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[t] *= alpha;
        __syncthreads();
        // ---- 3. this wave's channels of O^T += V P^T
        const raw *pp = Ps + j * PROW + T::EL * h;
#pragma unroll 4
        for (int st = 0; st < kAttnBK / T::KS; ++st) {
            const int64_t kk = k0 + st * T::KS;
            if (kk >= N) break;                                 // (uniform over the workgroup: the remaining weights are zeros)
            const int64_t left = N - (kk + T::EL * h);
            const int valid = left >= T::EL ? T::EL : left > 0 ? (int)left : 0;
            const frag bp = lds_frag<T>(pp + st * T::KS);
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int ch = w * (C / kAttnWaves) + 32 * t + j;
                const frag a = load_row<T, VEC>(vi + (int64_t)ch * N + kk + T::EL * h, valid);
                acc[t] = T::mma(a, bp, acc[t]);
            }
        }
        // (the next tile's writes of stat follow this tile's reads of it behind the second barrier; its writes of Ps follow its
        //  own first barrier, which every wave reaches only after these reads of Ps)
    }

    // ---- the row sums: 8 partials per query, added in one fixed order by every lane
    stat[(2 * w + h) * 32 + j] = lsum;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int i = 0; i < 2 * kAttnWaves; ++i) total += stat[i * 32 + j];
    if (q_ok) {
        const int64_t token = q0 + j;
#pragma unroll
        for (int t = 0; t < CT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = w * (C / kAttnWaves) + 32 * t + tile_row(r, h);
                const int64_t at = ((int64_t)b * C + ch) * N + token;
                const float o = acc[t][r] / total;
                if constexpr (HOUT) reinterpret_cast<raw *>(out)[at] = T::down(o);
                else reinterpret_cast<float *>(out)[at] = o;
            }
        // (in float64, rounded once: m * scale + ln(total) in fp32 is three roundings at the size of the result, and 32 lanes of one
        //  wave per workgroup do this once)
        if (lse != nullptr && w == 0 && h == 0) lse[(int64_t)b * N + token] = (float)((double)m * scale + log((double)total));
    }
}

template <class T, int C, bool HOUT, bool VEC>
static int launch_one(const AttnCall &c, const AttnPlan &p, hipStream_t s)
{
    using E = const typename T::raw *;
    const auto kernel = attn_kernel<T, C, HOUT, VEC>;
    const int rc = ensure_lds_above_48k((const void *)kernel, p.lds_bytes);
    if (rc) return rc;
    const float c2 = (float)(c.scale * 1.4426950408889634);
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3(p.threads), p.lds_bytes, s, (E)c.q, (E)c.k, (E)c.v, c.q_batch_stride, c.k_batch_stride,
                       c.v_batch_stride, c.N, (unsigned)p.q_tiles, c2, c.scale, (void *)c.out, (float *)c.lse);
    return launch_check("attn_kernel");
}

template <class T, bool HOUT, bool VEC>
static int launch_width(const AttnCall &c, const AttnPlan &p, hipStream_t s)
{
    static_assert(attn_width_built(256) && attn_width_built(512), "the plan admits what is instantiated here");
    return c.C == 256 ? launch_one<T, 256, HOUT, VEC>(c, p, s) : launch_one<T, 512, HOUT, VEC>(c, p, s);
}

template <class T>
static int launch_half(const AttnCall &c, const AttnPlan &p, hipStream_t s)
{
    const bool hout = c.out_dtype != CGIC_DT_F32;
    if (p.v_vec) return hout ? launch_width<T, true, true>(c, p, s) : launch_width<T, false, true>(c, p, s);
    return hout ? launch_width<T, true, false>(c, p, s) : launch_width<T, false, false>(c, p, s);
}

}  // namespace attn
}  // namespace cgic

using namespace cgic;

extern "C" int cgic_attention(const void *q, const void *k, const void *v, int in_dtype, int64_t B, int C, int64_t N, int64_t q_batch_stride,
                              int64_t k_batch_stride, int64_t v_batch_stride, double scale, void *out, int out_dtype, float *lse,
                              void *workspace, size_t workspace_bytes, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_attention");
    AttnCall c{};
    c.in_dtype = in_dtype; c.out_dtype = out_dtype; c.B = B; c.C = C; c.N = N;
    c.q_batch_stride = q_batch_stride; c.k_batch_stride = k_batch_stride; c.v_batch_stride = v_batch_stride; c.scale = scale;
    c.q = (uintptr_t)q; c.k = (uintptr_t)k; c.v = (uintptr_t)v; c.out = (uintptr_t)out; c.lse = (uintptr_t)lse;
    c.workspace = (uintptr_t)workspace; c.workspace_bytes = workspace_bytes;
    AttnPlan p;
    const char *why = "";
    const int rc = attn_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    if (p.form == 0) return CGIC_OK;
    const hipStream_t s = (hipStream_t)stream;
    if (in_dtype == CGIC_DT_F32) return attn::launch_width<attn::F32, false, false>(c, p, s);
    if (in_dtype == CGIC_DT_F16) return attn::launch_half<attn::F16>(c, p, s);
    return attn::launch_half<attn::BF16>(c, p, s);
}

extern "C" size_t cgic_attention_workspace_bytes(int in_dtype, int64_t B, int C, int64_t N)
{
    AttnPlan p;
    const char *why = "";
    return attn_form(in_dtype, in_dtype, B, C, N, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" int cgic_attention_supported(int in_dtype, int out_dtype, int64_t B, int C, int64_t N)
{
    AttnPlan p;
    const char *why = "";
    const int rc = attn_form(in_dtype, out_dtype, B, C, N, &p, &why);
    if (rc == CGIC_ERR_UNSUPPORTED) return 0;
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    return 1;
}
