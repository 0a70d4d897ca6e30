// cgic_rate_curve.hip -- the exact rate curve over EVERY medium rank of one coarse ratio (include/cgic_hip.h, section I): the
// .bin sizes CGIC.compress would write after per-image routing on the maps as given, for all n8 + 1 values of the one integer
// the medium decision is -- the rank K of the medium threshold among the 8x8-patch entropies (RouterTriple.py:28-32).
//
// Why one sort gives all of them.  With the coarse mask fixed, the router's medium list is e8 * (1 - up2(gate_coarse)): four
// zeros per coarse patch, the entropies of the others.  Its threshold is t = sorted[K - 1], the medium patches are the
// non-coarse ones with e8 < t (strict: tied patches move together), the fine ones the rest.  So in ONE ascending order of that
// list the medium patches of rank K are the first cnt(K) = lower_bound(sorted, sorted[K - 1]) elements (the coarse zeros among
// them carry no symbols), and a stream's size needs only the number and the summed code lengths of its symbols (cgic_rate.hip):
// prefix sums of len[ind_m] and of the four len[ind_f] of every patch in sorted order answer every K with two reads.
//
// One launch, one workgroup per image, everything in LDS:
//   1. sort the image's e16 (bitonic, in place), take the coarse threshold sorted[k_c - 1]; sum the coarse stream
//   2. one 64-bit word per 8x8 patch: the entropy's bit pattern (non-negative floats order as unsigned integers) above its
//      two payloads; coarse patches: 0.  Bitonic sort in place
//   3. inclusive scan of both payloads in sorted order
//   4. every K: a binary search for cnt(K), two prefix reads, five sizes out
#include "cgic_common.h"

#include <math.h>

namespace cgic {

constexpr int kCurveThreads = 1024;
constexpr int64_t kCurveMaxN8 = 12288;               // 8x8 patches of one image (a 768x768 tile has 9216): 12 bytes of LDS each
constexpr size_t kCurveLdsBudget = 152 * 1024;       // dynamic LDS of the workgroup; what the words leave of it stages code lengths
constexpr int kCurveMaxLen = 4095;                   // payload fields: 14 bits medium, 16 bits for the sum of four fine lengths
constexpr int kCurveSummary = 4;                     // int32 per image in the workspace

struct RateCurveArgs {
    const int32_t *len;                              // device [nsym] code lengths (TableDev.len)
    int nsym;
    int staged;                                      // the code lengths fit the LDS behind the words
    const int64_t *ind_c, *ind_m, *ind_f;            // [B, n16], [B, 4 n16], [B, 16 n16]
    const float *e16, *e8;
    int h16, w16;
    int k_c;                                         // coarse rank (0: no coarse patch, also in mode 1)
    int streams;                                     // cgic_mode_streams of mode 0 or mode 1
    int32_t *nbytes;                                 // [B, n8 + 1, 5]
    int32_t *summary;                                // [B, 4]: coarse patches, coarse threshold (bit pattern), medium / fine bits of all non-coarse patches
};

// finite, non-negative floats order as their bit patterns; -0.0 is 0.0
__device__ __forceinline__ unsigned int entropy_key(float e)
{
    return e == 0.0f ? 0u : __float_as_uint(e);
}

__device__ __forceinline__ void cmp_swap(unsigned long long *a, int lo, int hi)
{
    const unsigned long long x = a[lo], y = a[hi];
    if (y < x) { a[lo] = y; a[hi] = x; }
}

// Ascending bitonic sort of a[0 .. n) in LDS by the whole workgroup, in place, any n: the network of the next power of two in
// its form with every comparator pointing the same way (the first step of a merge mirrors its block), where elements beyond n
// count as +infinity -- they would never move, so comparators that reach them are skipped.
__device__ void lds_sort_u64(unsigned long long *a, int n, int tid, int nt)
{
    int lp = 0;
    while ((1 << lp) < n) ++lp;
    const int half = (1 << lp) >> 1;
    for (int lk = 1; lk <= lp; ++lk) {
        const int k = 1 << lk, hk = k >> 1;
        for (int t = tid; t < half; t += nt) {
            const int base = (t >> (lk - 1)) << lk, off = t & (hk - 1);
            const int lo = base + off, hi = base + (k - 1 - off);
            if (lo >= n) break;
            if (hi < n) cmp_swap(a, lo, hi);
        }
        __syncthreads();
        for (int lj = lk - 2; lj >= 0; --lj) {
            const int j = 1 << lj;
            for (int t = tid; t < half; t += nt) {
                const int lo = ((t >> lj) << (lj + 1)) | (t & (j - 1)), hi = lo + j;
                if (lo >= n) break;
                if (hi < n) cmp_swap(a, lo, hi);
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ unsigned int curve_wave_sum(unsigned int v)
{
    return (unsigned int)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(v), kWave - 1);
}

__device__ __forceinline__ int32_t stream_bytes(unsigned int count, unsigned int bits, bool bad)
{
    // HuffmanCoding.compress (indices_coding.py:113-124), as rate_reduce_kernel: no symbols -> empty file; else a header byte +
    // the code bits padded by 1..8 zero bits
    return bad ? (int32_t)(CGIC_ERR_INVALID - 10) : count == 0 ? 0 : (int32_t)(bits / 8u + 2u);
}

__global__ __launch_bounds__(kCurveThreads) void rate_curve_kernel(RateCurveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ unsigned long long scan_tmp[kCurveThreads / kWave + 1];
    __shared__ unsigned int sh_thr, sh_ncoarse, sh_cbits, sh_cbad, sh_first_bad_m, sh_last_bad_f;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t b = blockIdx.x;
    const int n16 = a.h16 * a.w16, n8 = 4 * n16, w8 = 2 * a.w16, w4 = 4 * a.w16;
    unsigned long long *kv = reinterpret_cast<unsigned long long *>(dyn);        // [n8] key << 32 | payload
    unsigned int *sf = reinterpret_cast<unsigned int *>(dyn + (size_t)n8 * 8);  // [n8] fine prefix
    int32_t *slen = reinterpret_cast<int32_t *>(dyn + (size_t)n8 * 12);
    const float *e16 = a.e16 + b * n16, *e8 = a.e8 + b * n8;
    const int64_t *ind_c = a.ind_c + b * n16, *ind_m = a.ind_m + b * n8, *ind_f = a.ind_f + b * 4 * (int64_t)n8;

    if (a.staged)
        for (int i = tid; i < a.nsym; i += nt) slen[i] = a.len[i];
    const int32_t *len = a.staged ? slen : a.len;
    if (tid == 0) { sh_thr = 0; sh_ncoarse = 0; sh_cbits = 0; sh_cbad = 0; sh_first_bad_m = 0xFFFFFFFFu; sh_last_bad_f = 0; }

    // ---- 1. the coarse threshold s16[k_c - 1] (k_c == 0: nothing is below the smallest, RouterTriple.py:24-25) and the coarse stream
    if (a.k_c > 0) {
        for (int i = tid; i < n16; i += nt) kv[i] = entropy_key(e16[i]);
        __syncthreads();
        lds_sort_u64(kv, n16, tid, nt);
        if (tid == 0) sh_thr = (unsigned int)kv[a.k_c - 1];
    }
    __syncthreads();
    const unsigned int thr = sh_thr;                 // (0 without a coarse rank: no key is below it)
    {
        unsigned int bits = 0, cnt = 0, bad = 0;
        for (int i = tid; i < n16; i += nt) {
            if (entropy_key(e16[i]) < thr) {
                const int64_t s = ind_c[i];
                if (s < 0 || s >= a.nsym) bad = 1;
                else bits += (unsigned int)len[s];
                ++cnt;
            }
        }
        bits = curve_wave_sum(bits);
        cnt = curve_wave_sum(cnt);
        bad = curve_wave_sum(bad);
        if ((tid & (kWave - 1)) == 0 && cnt) { atomicAdd(&sh_cbits, bits); atomicAdd(&sh_ncoarse, cnt); atomicAdd(&sh_cbad, bad); }
    }
    __syncthreads();                                 // (also: the sorted e16 keys are dead, the words may be written)

    // ---- 2. one word per 8x8 patch: key | medium bad, fine bad, len[ind_m] (14 bits), the four len[ind_f] (16 bits)
    for (int p = tid; p < n8; p += nt) {
        const int y = p / w8, x = p - y * w8;
        unsigned long long word = 0;                 // a coarse patch: the zero of e8 * (1 - gate), no symbols
        if (!(entropy_key(e16[(y >> 1) * a.w16 + (x >> 1)]) < thr)) {
            unsigned int pm = 0, pf = 0, flags = 0;
            const int64_t sm = ind_m[p];
            if (sm < 0 || sm >= a.nsym) flags |= 0x80000000u;
            else pm = (unsigned int)len[sm];
            const int64_t *f = ind_f + (int64_t)(2 * y) * w4 + 2 * x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t s = f[(q >> 1) * w4 + (q & 1)];
                if (s < 0 || s >= a.nsym) flags |= 0x40000000u;
                else pf += (unsigned int)len[s];
            }
            word = (unsigned long long)entropy_key(e8[p]) << 32 | flags | pm << 16 | pf;
        }
        kv[p] = word;
    }
    __syncthreads();
    lds_sort_u64(kv, n8, tid, nt);

    // ---- 3. prefix sums in sorted order (a contiguous run of words per thread; medium in the low, fine in the high half of one
    // 64-bit scan: kCurveMaxLen x kCurveMaxN8 keeps either total far below 2^32), and where symbols outside the table sit in that order
    const int per = (n8 + nt - 1) / nt;
    const int i0 = tid * per < n8 ? tid * per : n8, i1 = i0 + per < n8 ? i0 + per : n8;
    unsigned long long mine = 0;
    for (int i = i0; i < i1; ++i) {
        const unsigned int w = (unsigned int)kv[i];
        mine += (unsigned long long)(w & 0xFFFFu) << 32 | (w >> 16 & 0x3FFFu);
        if (w & 0x80000000u) atomicMin(&sh_first_bad_m, (unsigned int)i);
        if (w & 0x40000000u) atomicMax(&sh_last_bad_f, (unsigned int)i + 1u);
    }
    unsigned long long total;
    unsigned long long run = block_exclusive_scan<unsigned long long>(mine, scan_tmp, &total);
    for (int i = i0; i < i1; ++i) {
        const unsigned long long w = kv[i];
        const unsigned int lo = (unsigned int)w;
        run += (unsigned long long)(lo & 0xFFFFu) << 32 | (lo >> 16 & 0x3FFFu);
        kv[i] = (w & 0xFFFFFFFF00000000ull) | (unsigned int)run;       // key | medium bits of sorted[0 .. i]
        sf[i] = (unsigned int)(run >> 32);                             // fine bits of sorted[0 .. i]
    }
    __syncthreads();

    // ---- 4. every rank
    const unsigned int ncoarse = sh_ncoarse, zeros = 4u * ncoarse;
    const unsigned int total_f = (unsigned int)(total >> 32);
    const unsigned int first_bad_m = sh_first_bad_m, last_bad_f = sh_last_bad_f;
    const int32_t size_c = (a.streams & 1) ? stream_bytes(ncoarse, sh_cbits, sh_cbad != 0) : 0;
    const int32_t size_mc = (a.streams >> 3 & 1) ? (int32_t)(n16 / 8 + 2) : 0;      // BinaryCoding: one bit per element (mask_coding.py)
    const int32_t size_mm = (a.streams >> 4 & 1) ? (int32_t)(n8 / 8 + 2) : 0;
    int32_t *out = a.nbytes + b * (int64_t)(n8 + 1) * CGIC_NUM_STREAMS;
    for (int K = tid; K <= n8; K += nt) {
        const unsigned int t = (unsigned int)(kv[K ? K - 1 : 0] >> 32);              // sorted[K - 1] (K == 0: index 0, RouterTriple.py:31)
        int lo = 0, hi = K ? K - 1 : 0;                                              // lower bound of t: the first element not below it
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((unsigned int)(kv[mid] >> 32) < t) lo = mid + 1;
            else hi = mid;
        }
        const unsigned int cnt = (unsigned int)lo;                                   // elements with e8 < t; with t > 0 all coarse zeros are among them
        const unsigned int n_med = t ? cnt - zeros : 0u;
        const unsigned int n_fine = (unsigned int)n8 - zeros - n_med;
        const unsigned int bits_m = cnt ? (unsigned int)kv[cnt - 1] : 0u;
        const unsigned int bits_f = total_f - (cnt ? sf[cnt - 1] : 0u);
        int32_t *o = out + (int64_t)K * CGIC_NUM_STREAMS;
        o[0] = size_c;
        o[1] = (a.streams >> 1 & 1) ? stream_bytes(n_med, bits_m, first_bad_m < cnt) : 0;
        o[2] = (a.streams >> 2 & 1) ? stream_bytes(4u * n_fine, bits_f, last_bad_f > cnt) : 0;
        o[3] = size_mc;
        o[4] = size_mm;
    }
    if (tid == 0) {
        int32_t *s = a.summary + b * kCurveSummary;
        s[0] = (int32_t)ncoarse;
        s[1] = (int32_t)thr;
        s[2] = (int32_t)(unsigned int)total;
        s[3] = (int32_t)total_f;
    }
}

}  // namespace cgic

using namespace cgic;

// the rank arithmetic of the router (router_prepare in cgic_router.hip restated: Python's round() is round-half-even on the float64
// product, RouterTriple.py:23,30,42,54,65; ranks a mode does not use are 0)
extern "C" int cgic_router_ranks(double coarse_ratio, double medium_ratio, int64_t n16, int64_t *k_coarse, int64_t *k_medium)
{
    CGIC_REQUIRE(n16 > 0 && n16 < ((int64_t)1 << 29), CGIC_ERR_INVALID, "router_ranks: %lld coarse patches", (long long)n16);
    const int mode = cgic_router_mode(coarse_ratio, medium_ratio);
    const int64_t n8 = 4 * n16;
    double k_c = 0, k_m = 0;
    if (mode == 0 || mode == 2 || mode == 3) k_c = nearbyint((double)n16 * coarse_ratio);
    if (mode == 0) k_m = nearbyint((double)(4 * n16) * coarse_ratio + (double)n8 * medium_ratio);
    if (mode == 1) k_m = nearbyint((double)n8 * medium_ratio);
    CGIC_REQUIRE(k_c >= 0 && k_c <= (double)n16 && k_m >= 0 && k_m <= (double)n8, CGIC_ERR_INVALID,
                 "router: k out of range (k_coarse=%g of %lld, k_medium=%g of %lld); the reference raises IndexError",
                 k_c, (long long)n16, k_m, (long long)n8);
    if (k_coarse) *k_coarse = (int64_t)k_c;
    if (k_medium) *k_medium = (int64_t)k_m;
    return CGIC_OK;
}

extern "C" size_t cgic_rate_curve_workspace_bytes(int64_t B, int64_t h16, int64_t w16)
{
    if (B <= 0 || h16 <= 0 || w16 <= 0) return 0;
    return (((size_t)B * kCurveSummary * sizeof(int32_t)) + 255) & ~(size_t)255;
}

extern "C" int cgic_rate_curve(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f,
                               const float *e16, const float *e8, int64_t B, int64_t h16, int64_t w16, double coarse_ratio,
                               int32_t *nbytes, void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_rate_curve");
    CGIC_REQUIRE(t && ind_c && ind_m && ind_f && e16 && e8 && nbytes, CGIC_ERR_INVALID, "rate_curve: NULL argument");
    CGIC_REQUIRE(B >= 0 && h16 > 0 && w16 > 0, CGIC_ERR_INVALID, "rate_curve: bad shape");
    CGIC_REQUIRE(coarse_ratio >= 0.0 && coarse_ratio <= 1.0, CGIC_ERR_INVALID, "rate_curve: coarse ratio %g outside [0, 1]", coarse_ratio);
    CGIC_REQUIRE(B <= 65535, CGIC_ERR_UNSUPPORTED, "rate_curve: batch %lld exceeds the grid limit", (long long)B);
    CGIC_REQUIRE(h16 <= kCurveMaxN8 && w16 <= kCurveMaxN8 && 4 * h16 * w16 <= kCurveMaxN8, CGIC_ERR_UNSUPPORTED,
                 "rate_curve: an image of %lld 8x8 patches does not fit one workgroup's LDS (at most %lld: 768x1024 pixels)",
                 (long long)(4 * h16 * w16), (long long)kCurveMaxN8);
    const int64_t n16 = h16 * w16, n8 = 4 * n16;
    const int nsym = cgic_table_num_symbols(t);
    CGIC_REQUIRE(nsym > 0 && nsym <= 65536, CGIC_ERR_UNSUPPORTED, "rate_curve: table of %d symbols", nsym);
    CGIC_REQUIRE(cgic_table_max_len(t) <= kCurveMaxLen, CGIC_ERR_UNSUPPORTED, "rate_curve: codes of up to %d bits (at most %d)",
                 cgic_table_max_len(t), kCurveMaxLen);
    // the coarse rank of mode 0 (coarse ratio > 0); coarse ratio == 0 is mode 1: no coarse patch
    const int64_t k_c = coarse_ratio > 0.0 ? (int64_t)nearbyint((double)n16 * coarse_ratio) : 0;
    CGIC_REQUIRE(k_c >= 0 && k_c <= n16, CGIC_ERR_INVALID, "rate_curve: k_coarse=%lld of %lld", (long long)k_c, (long long)n16);
    const size_t need = cgic_rate_curve_workspace_bytes(B > 0 ? B : 1, h16, w16);
    CGIC_REQUIRE(workspace, CGIC_ERR_INVALID, "rate_curve: workspace of %zu bytes required (cgic_rate_curve_workspace_bytes)", need);
    CGIC_REQUIRE(((uintptr_t)workspace & 15u) == 0, CGIC_ERR_INVALID, "rate_curve: the workspace must be 16-byte aligned");
    if (B == 0) return CGIC_OK;
    TableDev tab;
    int rc = table_device_view(t, &tab);
    if (rc) return rc;

    RateCurveArgs a;
    a.len = tab.len; a.nsym = nsym;
    const size_t words = (size_t)n8 * 12;
    a.staged = words + (size_t)nsym * sizeof(int32_t) <= kCurveLdsBudget;
    a.ind_c = ind_c; a.ind_m = ind_m; a.ind_f = ind_f; a.e16 = e16; a.e8 = e8;
    a.h16 = (int)h16; a.w16 = (int)w16;
    a.k_c = (int)k_c;
    a.streams = cgic_mode_streams(coarse_ratio > 0.0 ? 0 : 1);
    a.nbytes = nbytes;
    a.summary = reinterpret_cast<int32_t *>(workspace);
    const size_t lds = words + (a.staged ? (size_t)nsym * sizeof(int32_t) : 0);
    if (lds > 64 * 1024) { rc = ensure_dynamic_lds((const void *)rate_curve_kernel, lds); if (rc) return rc; }
    // one comparator per thread and pass while the image is small; whole waves
    int threads = kCurveThreads;
    while (threads > 256 && threads >= n8) threads >>= 1;
    hipLaunchKernelGGL(rate_curve_kernel, dim3((unsigned)B), dim3((unsigned)threads), lds, (hipStream_t)stream, a);
    return launch_check("rate_curve_kernel");
}
