// cgic_attn_dev.h -- the device-side pieces that the attention kernels share (cgic_attn.hip: the forward; cgic_attn_bwd.hip: the
// backward): the operand types with their MFMA, the three ways a lane loads a fragment, the threshold below which a weight is an
// exact 0, and the register -> row map of a 32x32 result tile.
#pragma once
#include "cgic_common.h"
#include "cgic_attn_plan.h"

#include <math.h>

namespace cgic {
namespace attn {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));

// an operand type: its storage element, the fragment a lane hands to one MFMA (EL elements: k = EL * (lane >> 5) + e of the KS of
// a step), the rounding of a fp32 value to it, and the MFMA
struct F32 {
    using raw = float;
    using frag = float;
    static constexpr int KS = 2, EL = 1, PAD = 1;
    static constexpr int CHAINS = 4;                // a score is 4 interleaved sums of C / 4 products added pairwise: a single fp32 chain of C erred ~2x more than a blocked GEMM's
    static __device__ __forceinline__ float down(float f) { return f; }
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
};
struct F16 {
    using raw = uint16_t;
    using frag = u16x8;
    static constexpr int KS = 16, EL = 8, PAD = 8, CHAINS = 1;
    static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
};
struct BF16 {
    using raw = uint16_t;
    using frag = u16x8;
    static constexpr int KS = 16, EL = 8, PAD = 8, CHAINS = 1;
    static __device__ __forceinline__ uint16_t down(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
    static __device__ __forceinline__ f32x16 mma(frag a, frag b, f32x16 c)
    {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};

static_assert(attn_pad(CGIC_DT_F32) == F32::PAD && attn_pad(CGIC_DT_F16) == F16::PAD && attn_pad(CGIC_DT_BF16) == BF16::PAD, "the plan sizes the LDS rows");

// EL elements `stride` apart (one token of k, EL consecutive channels), zeros when the token is past the end
template <class T>
__device__ __forceinline__ typename T::frag load_strided(const typename T::raw *p, int64_t stride, bool ok)
{
    if constexpr (T::EL == 1) {
        return ok ? p[0] : 0.f;
    } else {
        typename T::frag f;
#pragma unroll
        for (int e = 0; e < T::EL; ++e) f[e] = ok ? p[(int64_t)e * stride] : (typename T::raw)0;
        return f;
    }
}

// EL consecutive elements (one channel of v, EL consecutive tokens) of which the first `valid` exist; zeros behind them
template <class T, bool VEC>
__device__ __forceinline__ typename T::frag load_row(const typename T::raw *p, int valid)
{
    if constexpr (T::EL == 1) {
        return valid > 0 ? p[0] : 0.f;
    } else {
        if constexpr (VEC)
            if (valid >= T::EL) return *reinterpret_cast<const typename T::frag *>(p);          // (the plan: 16-byte aligned)
        typename T::frag f;
#pragma unroll
        for (int e = 0; e < T::EL; ++e) f[e] = e < valid ? p[e] : (typename T::raw)0;
        return f;
    }
}

// a lane's fragment of an LDS image whose rows are the MFMA's column (query) and whose row elements are its k index
template <class T>
__device__ __forceinline__ typename T::frag lds_frag(const typename T::raw *p)
{
    if constexpr (T::EL == 1) return p[0];
    else return *reinterpret_cast<const typename T::frag *>(p);                                   // (rows and offsets are multiples of 16 bytes)
}

// A weight, or a rescale factor of the accumulator, below 2^-64 of the row's largest weight is taken as exactly 0.  The row sum is at
// least 1 and the accumulator's own roundings are 2^-24 of its largest term, so such a term is 40 binary orders below what fp32 keeps
// unless one v is 2^40 times the terms that carry the result.  It must be an exact 0, not merely small: v_mfma_f32_32x32x16_{f16,bf16}
// returns the predecessor of v * 1 when v is a power of two and its C input is any non-zero number of the opposite sign, however
// small (1 + -2^-149 gives 1 - 2^-24), so a row whose weight is 1 on one key would miss v's own bits by an ulp.
constexpr float kNegligible = -64.f;

// exp2 of an exponent that is not below kNegligible (or is NaN): v_exp_f32 itself, which is what exp2f comes down to once its
// rescaling of results below 2^-126 has nothing to do -- the same bits, and the select against kNegligible costs less than that
static_assert(kNegligible > -126.f, "v_exp_f32 returns 0 for a denormal result; the select must keep such exponents from it");
__device__ __forceinline__ float exp2_above_negligible(float x) { return __builtin_amdgcn_exp2f(x); }

// row of the 32x32 result tile that register r of a lane in half h holds (its column is lane & 31)
__device__ __forceinline__ int tile_row(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

}  // namespace attn
}  // namespace cgic
