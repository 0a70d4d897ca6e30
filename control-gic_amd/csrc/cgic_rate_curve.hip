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
//   2. one 64-bit word per 8x8 patch: an order-preserving key of the medium list's element (entropy_key: any float, NaN last
//      like torch.sort, -0 with +0) above its two payloads; coarse patches: the key of the fp32 product e8 * 0 -- a zero, or NaN
//      under a NaN or an infinite entropy -- and no payload.  Bitonic sort in place
//   3. inclusive scan of both payloads in sorted order
//   4. every K: a binary search for cnt(K), two prefix reads, five sizes out
// The comparisons are the router's on every float (cgic_router_dev.h: f2key, float '<'): nothing is below a NaN threshold, a NaN
// is below nothing, the zeros of either sign are equal, and the gated zeros count as medium-list elements below t only when t > 0.
//
// cgic_rate_curve_tiles (section I, ABI 11) runs the same steps 1-3 (curve_sort_scan: ONE body for both kernels) for T tiles of
// mixed shapes, one workgroup per tile, its shape and offsets read from a descriptor; step 4 answers the M requested ranks of the
// tile's shape class, and a second launch sums the tiles of each image per setting and stream.
#include "cgic_common.h"
#include "cgic_rate_plan.h"

#include <math.h>

namespace cgic {

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

// Order-preserving key of any float: key(a) < key(b) == (a < b) for every pair without a NaN; -0.0 is 0.0 (they compare equal), every
// NaN is the largest key (torch.sort puts NaN last).  Key 0 would be a negative NaN: no element has it, so nothing is below 0.
constexpr unsigned int kKeyNaN = 0xFFFFFFFFu, kKeyZero = 0x80000000u;
__device__ __forceinline__ unsigned int entropy_key(float e)
{
    if (e != e) return kKeyNaN;
    const unsigned int u = __float_as_uint(e);
    return (u << 1) == 0u ? kKeyZero : (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the fp32 bit pattern of a key's float (NaN: the quiet NaN; key 0 -- no threshold -- gives 0)
__device__ __forceinline__ unsigned int entropy_key_bits(unsigned int k)
{
    return k == kKeyNaN ? 0x7FC00000u : k == 0u ? 0u : (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
}
// float '<' on keys: a NaN threshold has nothing below it
__device__ __forceinline__ bool key_below(unsigned int k, unsigned int t) { return t != kKeyNaN && k < t; }

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

// one image / tile as steps 1-3 see it
struct CurveTile {
    const int64_t *ind_c, *ind_m, *ind_f;            // [n16], [4 n16], [16 n16]
    const float *e16, *e8;
    int h16, w16;
    int k_c;
};

// what steps 1-3 leave beside the sorted words: kv[i] = key << 32 | medium bits of sorted[0 .. i], sf[i] = fine bits of sorted[0 .. i]
struct CurveSorted {
    const unsigned long long *kv;
    const unsigned int *sf;
    int n8;
    unsigned int ncoarse, gzeros, thr, total_m, total_f, first_bad_m, last_bad_f;      // gzeros: coarse 8x8 patches whose product e8 * 0 is a zero
    int32_t size_c, size_mc, size_mm;
};

// steps 1-3 for one image / tile by the whole workgroup, in the dynamic LDS `dyn` (12 bytes per 8x8 patch, then the staged code
// lengths).  Every argument is workgroup-uniform.  Ends behind a barrier: kv / sf may be read by any thread
__device__ __forceinline__ CurveSorted curve_sort_scan(const CurveTile &c, const int32_t *glen, int nsym, int staged, int streams,
                                                       unsigned char *dyn)
{
    __shared__ unsigned long long scan_tmp[kCurveThreads / kWave + 1];
    __shared__ unsigned int sh_thr, sh_ncoarse, sh_gzeros, sh_cbits, sh_cbad, sh_first_bad_m, sh_last_bad_f;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int n16 = c.h16 * c.w16, n8 = 4 * n16, w8 = 2 * c.w16, w4 = 4 * c.w16;
    unsigned long long *kv = reinterpret_cast<unsigned long long *>(dyn);        // [n8] key << 32 | payload
    unsigned int *sf = reinterpret_cast<unsigned int *>(dyn + (size_t)n8 * 8);  // [n8] fine prefix
    int32_t *slen = reinterpret_cast<int32_t *>(dyn + (size_t)n8 * 12);
    const float *e16 = c.e16, *e8 = c.e8;
    const int64_t *ind_c = c.ind_c, *ind_m = c.ind_m, *ind_f = c.ind_f;

    if (staged)
        for (int i = tid; i < nsym; i += nt) slen[i] = glen[i];
    const int32_t *len = staged ? slen : glen;
    if (tid == 0) { sh_thr = 0; sh_ncoarse = 0; sh_gzeros = 0; sh_cbits = 0; sh_cbad = 0; sh_first_bad_m = 0xFFFFFFFFu; sh_last_bad_f = 0; }

    // ---- 1. the coarse threshold s16[k_c - 1] (k_c == 0: nothing is below the smallest, RouterTriple.py:24-25) and the coarse stream
    if (c.k_c > 0) {
        for (int i = tid; i < n16; i += nt) kv[i] = entropy_key(e16[i]);
        __syncthreads();
        lds_sort_u64(kv, n16, tid, nt);
        if (tid == 0) sh_thr = (unsigned int)kv[c.k_c - 1];
    }
    __syncthreads();
    const unsigned int thr = sh_thr;                 // (0 without a coarse rank: no key is below it)
    {
        unsigned int bits = 0, cnt = 0, bad = 0;
        for (int i = tid; i < n16; i += nt) {
            if (key_below(entropy_key(e16[i]), thr)) {
                const int64_t s = ind_c[i];
                if (s < 0 || s >= nsym) bad = 1;
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
    unsigned int gz = 0;
    for (int p = tid; p < n8; p += nt) {
        const int y = p / w8, x = p - y * w8;
        // a coarse patch: the fp32 product e8 * (1 - gate) as the reference forms it (RouterTriple.py:27), no symbols
        const unsigned int gkey = entropy_key(e8[p] * 0.0f);
        unsigned long long word = (unsigned long long)gkey << 32;
        if (key_below(entropy_key(e16[(y >> 1) * c.w16 + (x >> 1)]), thr)) {
            gz += gkey == kKeyZero ? 1u : 0u;
        } else {
            unsigned int pm = 0, pf = 0, flags = 0;
            const int64_t sm = ind_m[p];
            if (sm < 0 || sm >= nsym) flags |= 0x80000000u;
            else pm = (unsigned int)len[sm];
            const int64_t *f = ind_f + (int64_t)(2 * y) * w4 + 2 * x;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t s = f[(q >> 1) * w4 + (q & 1)];
                if (s < 0 || s >= nsym) flags |= 0x40000000u;
                else pf += (unsigned int)len[s];
            }
            word = (unsigned long long)entropy_key(e8[p]) << 32 | flags | pm << 16 | pf;
        }
        kv[p] = word;
    }
    if (thr) {                                       // (workgroup-uniform; without a coarse threshold there is no coarse patch)
        gz = curve_wave_sum(gz);
        if ((tid & (kWave - 1)) == 0 && gz) atomicAdd(&sh_gzeros, gz);
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

    CurveSorted r;
    r.kv = kv; r.sf = sf; r.n8 = n8;
    r.ncoarse = sh_ncoarse; r.gzeros = sh_gzeros; r.thr = thr;
    r.total_m = (unsigned int)total; r.total_f = (unsigned int)(total >> 32);
    r.first_bad_m = sh_first_bad_m; r.last_bad_f = sh_last_bad_f;
    r.size_c = (streams & 1) ? stream_bytes(r.ncoarse, sh_cbits, sh_cbad != 0) : 0;
    r.size_mc = (streams >> 3 & 1) ? (int32_t)(n16 / 8 + 2) : 0;       // BinaryCoding: one bit per element (mask_coding.py)
    r.size_mm = (streams >> 4 & 1) ? (int32_t)(n8 / 8 + 2) : 0;
    return r;
}

// ---- 4. one rank K in 0 .. n8: five sizes to o[0 .. 5)
__device__ __forceinline__ void curve_rank_sizes(const CurveSorted &r, int K, int streams, int32_t *o)
{
    const unsigned long long *kv = r.kv;
    const unsigned int t = (unsigned int)(kv[K ? K - 1 : 0] >> 32);              // sorted[K - 1] (K == 0: index 0, RouterTriple.py:31)
    int lo = 0, hi = K ? K - 1 : 0;                                              // lower bound of t: the first element not below it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((unsigned int)(kv[mid] >> 32) < t) lo = mid + 1;
        else hi = mid;
    }
    // elements of the medium list below t (none below a NaN); the gated zeros are among them exactly when t > 0, the gated NaNs never
    const unsigned int cnt = t != kKeyNaN ? (unsigned int)lo : 0u;
    const unsigned int n_med = cnt - (cnt && t > kKeyZero ? r.gzeros : 0u);
    const unsigned int n_fine = (unsigned int)r.n8 - 4u * r.ncoarse - n_med;
    const unsigned int bits_m = cnt ? (unsigned int)kv[cnt - 1] : 0u;
    const unsigned int bits_f = r.total_f - (cnt ? r.sf[cnt - 1] : 0u);
    o[0] = r.size_c;
    o[1] = (streams >> 1 & 1) ? stream_bytes(n_med, bits_m, r.first_bad_m < cnt) : 0;
    o[2] = (streams >> 2 & 1) ? stream_bytes(4u * n_fine, bits_f, r.last_bad_f > cnt) : 0;
    o[3] = r.size_mc;
    o[4] = r.size_mm;
}

__device__ __forceinline__ void curve_summary(const CurveSorted &r, int32_t *s)
{
    s[0] = (int32_t)r.ncoarse;
    s[1] = (int32_t)entropy_key_bits(r.thr);
    s[2] = (int32_t)r.total_m;
    s[3] = (int32_t)r.total_f;
}

__global__ __launch_bounds__(kCurveThreads) void rate_curve_kernel(RateCurveArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t b = blockIdx.x;
    const int n16 = a.h16 * a.w16, n8 = 4 * n16;
    CurveTile c;
    c.ind_c = a.ind_c + b * n16; c.ind_m = a.ind_m + b * n8; c.ind_f = a.ind_f + b * 4 * (int64_t)n8;
    c.e16 = a.e16 + b * n16; c.e8 = a.e8 + b * n8;
    c.h16 = a.h16; c.w16 = a.w16; c.k_c = a.k_c;
    const CurveSorted r = curve_sort_scan(c, a.len, a.nsym, a.staged, a.streams, dyn);
    int32_t *out = a.nbytes + b * (int64_t)(n8 + 1) * CGIC_NUM_STREAMS;
    for (int K = tid; K <= n8; K += nt) curve_rank_sizes(r, K, a.streams, out + (int64_t)K * CGIC_NUM_STREAMS);
    if (tid == 0) curve_summary(r, a.summary + b * kCurveSummary);
}

// ---- cgic_rate_curve_tiles: T tiles of mixed shapes, the M requested ranks of each tile's shape class ------------------------
constexpr int32_t kTilesBadRank = CGIC_ERR_INVALID - 11;          // a rank outside 0 .. n8 of the tile (negative: folds to -1)

struct RateTilesArgs {
    const int32_t *len;
    int nsym;
    int staged;                                      // the code lengths fit the LDS behind the words of the LARGEST tile
    const int64_t *ind_c, *ind_m, *ind_f;            // concatenated buffers; a tile's part starts at its descriptor's offsets
    const float *e16, *e8;
    const cgic_rate_tile *tiles;                     // device [T]
    const int32_t *ranks;                            // device [S, M]
    int M;
    int streams;
    int32_t *tile_nbytes;                            // [T, M, 5]
    int32_t *summary;                                // [T, 4], as rate_curve_kernel's
};

// One workgroup per tile.  The descriptor is read at a workgroup-uniform address before the kernel stores anything: scalar loads,
// and everything derived from it (shape, offsets, k_c) lives in scalar registers, like a launch group's argument block
__global__ __launch_bounds__(kCurveThreads) void rate_curve_tiles_kernel(RateTilesArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t t = blockIdx.x;
    const cgic_rate_tile d = a.tiles[t];
    CurveTile c;
    c.ind_c = a.ind_c + d.off_c; c.ind_m = a.ind_m + d.off_m; c.ind_f = a.ind_f + d.off_f;
    c.e16 = a.e16 + d.off_e16; c.e8 = a.e8 + d.off_e8;
    c.h16 = d.h16; c.w16 = d.w16; c.k_c = d.k_c;
    const CurveSorted r = curve_sort_scan(c, a.len, a.nsym, a.staged, a.streams, dyn);
    const int32_t *ranks = a.ranks + (int64_t)d.shape * a.M;
    int32_t *out = a.tile_nbytes + t * (int64_t)a.M * CGIC_NUM_STREAMS;
    for (int j = tid; j < a.M; j += nt) {
        const int K = ranks[j];
        int32_t *o = out + (int64_t)j * CGIC_NUM_STREAMS;
        if (K < 0 || K > r.n8) {
#pragma unroll
            for (int s = 0; s < CGIC_NUM_STREAMS; ++s) o[s] = kTilesBadRank;
        } else {
            curve_rank_sizes(r, K, a.streams, o);
        }
    }
    if (tid == 0) curve_summary(r, a.summary + t * kCurveSummary);
}

// image_nbytes[n, j, :] = the sum over the tiles of image n (blockIdx.y) of tile_nbytes[t, j, :], in descriptor order, as int64; a
// negative tile entry (a symbol outside the table, a rank outside the tile) makes all five -1.  One thread per setting; the walk
// over the descriptors is workgroup-uniform (scalar loads and a scalar branch per tile)
__global__ __launch_bounds__(kFoldThreads) void rate_fold_tiles_kernel(const cgic_rate_tile *tiles, int T, int M,
                                                                       const int32_t *tile_nbytes, int64_t *image_nbytes)
{
    const int n = blockIdx.y;
    const int j = blockIdx.x * kFoldThreads + threadIdx.x;
    if (j >= M) return;
    int64_t acc[CGIC_NUM_STREAMS] = {0, 0, 0, 0, 0};
    bool bad = false;
    for (int t = 0; t < T; ++t) {
        if (tiles[t].image != n) continue;
        const int32_t *p = tile_nbytes + ((int64_t)t * M + j) * CGIC_NUM_STREAMS;
#pragma unroll
        for (int s = 0; s < CGIC_NUM_STREAMS; ++s) {
            const int32_t v = p[s];
            bad |= v < 0;
            acc[s] += v;
        }
    }
    int64_t *o = image_nbytes + ((int64_t)n * M + j) * CGIC_NUM_STREAMS;
#pragma unroll
    for (int s = 0; s < CGIC_NUM_STREAMS; ++s) o[s] = bad ? -1 : acc[s];
}

// ---- cgic_route_to_budget: curve at R requested ranks -> pick under a byte budget read from the device -> masks and indices -----
struct RateRanksArgs {
    const int32_t *len;
    int nsym;
    int staged;
    const int64_t *ind_c, *ind_m, *ind_f;
    const float *e16, *e8;
    int h16, w16;
    int k_c;
    int streams;
    const int32_t *ranks;                            // device [R], ascending
    int R;
    int32_t *total;                                  // [B, R]: the five sizes summed; negative: a selected symbol outside the table
    uint32_t *tkey;                                  // [B, R]: the medium threshold at that rank (fp32 bit pattern)
    int32_t *summary;                                // [B, 4], as rate_curve_kernel's
};

// One workgroup per image: steps 1-3 of rate_curve_kernel, then the R requested ranks -- per rank the image's bytes and the key the
// medium mask compares against
__global__ __launch_bounds__(kCurveThreads) void rate_curve_ranks_kernel(RateRanksArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int64_t b = blockIdx.x;
    const int n16 = a.h16 * a.w16, n8 = 4 * n16;
    CurveTile c;
    c.ind_c = a.ind_c + b * n16; c.ind_m = a.ind_m + b * n8; c.ind_f = a.ind_f + b * 4 * (int64_t)n8;
    c.e16 = a.e16 + b * n16; c.e8 = a.e8 + b * n8;
    c.h16 = a.h16; c.w16 = a.w16; c.k_c = a.k_c;
    const CurveSorted r = curve_sort_scan(c, a.len, a.nsym, a.staged, a.streams, dyn);
    int32_t *total = a.total + b * a.R;
    uint32_t *tkey = a.tkey + b * a.R;
    for (int j = tid; j < a.R; j += nt) {
        const int K = a.ranks[j];
        int32_t sum = kTilesBadRank;                 // (a rank outside 0 .. n8: the caller's list is wrong; counts as unusable)
        uint32_t t = 0;
        if (K >= 0 && K <= n8) {
            int32_t o[CGIC_NUM_STREAMS];
            curve_rank_sizes(r, K, a.streams, o);
            bool bad = false;
            sum = 0;
#pragma unroll
            for (int s = 0; s < CGIC_NUM_STREAMS; ++s) { bad |= o[s] < 0; sum += o[s]; }
            if (bad) sum = (int32_t)(CGIC_ERR_INVALID - 10);
            t = entropy_key_bits((uint32_t)(r.kv[K ? K - 1 : 0] >> 32));
        }
        total[j] = sum;
        tkey[j] = t;
    }
    if (tid == 0) curve_summary(r, a.summary + b * kCurveSummary);
}

// a candidate of the pick: better = the larger (fit) or the smaller (no fit) batch size, then the smaller index (= the smaller rank)
struct PickBest {
    int64_t s;
    int j;                                           // -1: none
};

__device__ __forceinline__ PickBest pick_better(PickBest x, PickBest y, bool larger)
{
    if (x.j < 0) return y;
    if (y.j < 0) return x;
    if (x.s != y.s) return ((x.s > y.s) == larger) ? x : y;
    return x.j < y.j ? x : y;
}

// S[j] = the batch's bytes at requested rank j (int64, integer sums: any order gives the same value), then rate._pick's rule on
// S against the budget.  ONE workgroup: with fewer ranks than threads the images are dealt over `parts` thread rows per rank
// and the rows are added in LDS in row order
__global__ __launch_bounds__(kPickThreads) void rate_pick_kernel(const int32_t *total, const int32_t *ranks, int B, int R,
                                                                 const int64_t *budget_dev, int64_t *choice)
{
    __shared__ int64_t part_s[kPickThreads];
    __shared__ int part_bad[kPickThreads];
    __shared__ PickBest red[2][kPickThreads];
    const int tid = threadIdx.x;
    int cols = kPickThreads;
    while (cols > 1 && (cols >> 1) >= R) cols >>= 1;
    const int parts = kPickThreads / cols, q = tid & (cols - 1), p = tid / cols;
    const int64_t budget = *budget_dev;
    PickBest fit = {0, -1}, low = {0, -1};
    int bad = 0;
    for (int j0 = 0; j0 < R; j0 += cols) {           // (workgroup-uniform trip count; parts > 1 only when one trip covers R)
        const int j = j0 + q;
        int64_t s = 0;
        if (j < R)
            for (int b = p; b < B; b += parts) {
                const int32_t v = total[(int64_t)b * R + j];
                bad |= v < 0;
                s += v;
            }
        if (parts > 1) {
            part_s[tid] = s;
            __syncthreads();
            if (p == 0)
                for (int k = 1; k < parts; ++k) s += part_s[k * cols + q];
            __syncthreads();
        }
        if (p == 0 && j < R) {
            const PickBest me = {s, j};
            if (s <= budget) fit = pick_better(fit, me, true);
            low = pick_better(low, me, false);
        }
    }
    part_bad[tid] = bad;
    red[0][tid] = fit;
    red[1][tid] = low;
    __syncthreads();
    for (int d = kPickThreads >> 1; d > 0; d >>= 1) {
        if (tid < d) {
            red[0][tid] = pick_better(red[0][tid], red[0][tid + d], true);
            red[1][tid] = pick_better(red[1][tid], red[1][tid + d], false);
            part_bad[tid] |= part_bad[tid + d];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const bool any_bad = part_bad[0] != 0;
        const bool fits = red[0][0].j >= 0;
        const PickBest w = fits ? red[0][0] : red[1][0];
        choice[0] = any_bad ? -1 : w.j;
        choice[1] = any_bad ? -1 : ranks[w.j];
        choice[2] = any_bad ? 0 : (fits ? 1 : 0);
        choice[3] = any_bad ? -1 : w.s;
    }
}

struct RateApplyArgs {
    const int64_t *choice;                           // device [4]
    const uint32_t *tkey;                            // [B, R]
    const int32_t *summary;                          // [B, 4]
    const int64_t *ind_c, *ind_m, *ind_f;
    const float *e16, *e8;
    int B, h16, w16, R;
    int k_c;                                         // 0: no coarse patch
    int32_t *mc, *mm, *mf;
    int64_t *ind;
};

// One thread per row of a 4x4 fine block (= one 16x16 pixel patch): four fine mask elements and four merged indices in 16-byte
// stores, the two medium elements of even rows, the coarse element of the block's first row.  The comparisons are the router's float
// '<' against the thresholds the sort found (on keys, which order as '<' does): coarse = e16 < thr_c, medium = not coarse and e8 < t,
// fine = the rest (RouterTriple.py:25,32,34)
__global__ __launch_bounds__(kApplyThreads) void rate_apply_kernel(RateApplyArgs a)
{
    const int64_t j = a.choice[0];
    const int w16 = a.w16, h4 = 4 * a.h16, w8 = 2 * w16, w4 = 4 * w16;
    const int64_t rows = (int64_t)a.B * h4 * w16;
    for (int64_t i = (int64_t)blockIdx.x * kApplyThreads + threadIdx.x; i < rows; i += (int64_t)gridDim.x * kApplyThreads) {
        const int64_t by = i / w16;
        const int xc = (int)(i - by * w16);
        const int64_t b = by / h4;
        const int y = (int)(by - b * h4);
        const int64_t o4 = by * w4 + 4 * xc;                             // (b, y, 4 xc) on the fine grid
        const int64_t o8 = (b * (h4 >> 1) + (y >> 1)) * w8 + 2 * xc;     // (b, y / 2, 2 xc) on the medium grid
        const int64_t o16 = (b * a.h16 + (y >> 2)) * w16 + xc;
        int4 f = make_int4(0, 0, 0, 0);
        int2 m = make_int2(0, 0);
        int c = 0;
        longlong2 v0 = {0, 0}, v1 = {0, 0};
        if (j >= 0) {
            const float thr = __uint_as_float((unsigned int)a.summary[b * kCurveSummary + 1]);
            const float t = __uint_as_float(a.tkey[b * a.R + j]);
            c = a.k_c > 0 && a.e16[o16] < thr;
            const float2 e = *reinterpret_cast<const float2 *>(a.e8 + o8);
            m.x = !c && e.x < t;
            m.y = !c && e.y < t;
            const int f0 = !c && !m.x, f1 = !c && !m.y;
            f = make_int4(f0, f0, f1, f1);
            if (c) {
                const int64_t s = a.ind_c[o16];
                v0 = {s, s}; v1 = {s, s};
            } else {
                const longlong2 sm = *reinterpret_cast<const longlong2 *>(a.ind_m + o8);
                v0 = {sm.x, sm.x}; v1 = {sm.y, sm.y};
                if (f0) v0 = *reinterpret_cast<const longlong2 *>(a.ind_f + o4);
                if (f1) v1 = *reinterpret_cast<const longlong2 *>(a.ind_f + o4 + 2);
            }
        }
        *reinterpret_cast<int4 *>(a.mf + o4) = f;
        *reinterpret_cast<longlong2 *>(a.ind + o4) = v0;
        *reinterpret_cast<longlong2 *>(a.ind + o4 + 2) = v1;
        if ((y & 1) == 0) *reinterpret_cast<int2 *>(a.mm + o8) = m;
        if ((y & 3) == 0) a.mc[o16] = c;
    }
}

}  // namespace cgic

using namespace cgic;

// the rank arithmetic of the router (cgic_encode_plan.h: router_ranks; ranks a mode does not use are 0)
extern "C" int cgic_router_ranks(double coarse_ratio, double medium_ratio, int64_t n16, int64_t *k_coarse, int64_t *k_medium)
{
    CGIC_REQUIRE(n16 > 0 && n16 < ((int64_t)1 << 29), CGIC_ERR_INVALID, "router_ranks: %lld coarse patches", (long long)n16);
    double k_c, k_m;
    CGIC_REQUIRE(router_ranks(router_mode(coarse_ratio, medium_ratio), n16, coarse_ratio, medium_ratio, &k_c, &k_m), CGIC_ERR_INVALID,
                 "router: k out of range (k_coarse=%g of %lld, k_medium=%g of %lld); the reference raises IndexError",
                 k_c, (long long)n16, k_m, (long long)(4 * n16));
    if (k_coarse) *k_coarse = (int64_t)k_c;
    if (k_medium) *k_medium = (int64_t)k_m;
    return CGIC_OK;
}

// ---- the host side of the three curve entry points: each fills a CurveCall, asks cgic_rate_plan.h for the plan once and issues it ----

// what the three calls share: the table as the plan wants it, the five inputs, the workspace
static CurveCall curve_call(CurveEntry entry, const cgic_table *t, const void *ind_c, const void *ind_m, const void *ind_f, const void *e16,
                            const void *e8, double coarse_ratio, const void *workspace)
{
    CurveCall c{};
    c.shape.entry = entry;
    c.table = t != nullptr;
    if (t) { c.nsym = cgic_table_num_symbols(t); c.max_len = cgic_table_max_len(t); }
    c.coarse_ratio = coarse_ratio;
    c.ind_c = (uintptr_t)ind_c; c.ind_m = (uintptr_t)ind_m; c.ind_f = (uintptr_t)ind_f; c.e16 = (uintptr_t)e16; c.e8 = (uintptr_t)e8;
    c.workspace = (uintptr_t)workspace;
    return c;
}

// steps 1-3 as the plan laid them out; fills what the three argument blocks share (table, mode's streams, staging) and launches
template <class A>
static int curve_launch(void (*kernel)(A), const char *name, const cgic_table *t, const CurveCall &c, const CurvePlan &p, A a, hipStream_t stream)
{
    TableDev tab;
    int rc = table_device_view(t, &tab);
    if (rc) return rc;
    a.len = tab.len; a.nsym = c.nsym;
    a.streams = cgic_mode_streams(p.mode);
    a.staged = p.staged;
    if (p.lds_opt_in) { rc = ensure_dynamic_lds((const void *)kernel, p.lds_bytes); if (rc) return rc; }
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.grid), dim3((unsigned)p.threads), p.lds_bytes, stream, a);
    return launch_check(name);
}

extern "C" size_t cgic_rate_curve_workspace_bytes(int64_t B, int64_t h16, int64_t w16)
{
    CurveShape s{};
    s.entry = CURVE_IMAGES; s.B = B; s.h16 = h16; s.w16 = w16;
    return curve_workspace_bytes(s);
}

extern "C" int cgic_rate_curve(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f,
                               const float *e16, const float *e8, int64_t B, int64_t h16, int64_t w16, double coarse_ratio,
                               int32_t *nbytes, void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_rate_curve");
    CurveCall c = curve_call(CURVE_IMAGES, t, ind_c, ind_m, ind_f, e16, e8, coarse_ratio, workspace);
    c.shape.B = B; c.shape.h16 = h16; c.shape.w16 = w16;
    c.nbytes = (uintptr_t)nbytes;
    CurvePlan p;
    const char *why = "";
    const int rc = curve_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);
    if (p.nothing_to_do) return CGIC_OK;

    RateCurveArgs a;
    a.ind_c = ind_c; a.ind_m = ind_m; a.ind_f = ind_f; a.e16 = e16; a.e8 = e8;
    a.h16 = (int)h16; a.w16 = (int)w16; a.k_c = (int)p.k_c;
    a.nbytes = nbytes;
    a.summary = reinterpret_cast<int32_t *>(reinterpret_cast<unsigned char *>(workspace) + p.off_summary);
    return curve_launch(rate_curve_kernel, "rate_curve_kernel", t, c, p, a, (hipStream_t)stream);
}

extern "C" size_t cgic_rate_curve_tiles_workspace_bytes(int64_t T, int64_t M, int tile_nbytes_given)
{
    CurveShape s{};
    s.entry = CURVE_TILES; s.T = T; s.N = 1; s.S = 1; s.M = M; s.tile_nbytes_given = tile_nbytes_given != 0;
    return curve_workspace_bytes(s);
}

extern "C" int cgic_rate_curve_tiles(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f,
                                     const float *e16, const float *e8, const int64_t *count, const cgic_rate_tile *tiles,
                                     const cgic_rate_tile *tiles_dev, int64_t T, int64_t N, double coarse_ratio,
                                     const int32_t *ranks_dev, int64_t S, int64_t M, int64_t *image_nbytes, int32_t *tile_nbytes,
                                     void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_rate_curve_tiles");
    CurveCall c = curve_call(CURVE_TILES, t, ind_c, ind_m, ind_f, e16, e8, coarse_ratio, workspace);
    c.shape.T = T; c.shape.N = N; c.shape.S = S; c.shape.M = M; c.shape.tile_nbytes_given = tile_nbytes != nullptr;
    c.count = count; c.tiles = tiles;
    c.tiles_dev = (uintptr_t)tiles_dev; c.ranks_dev = (uintptr_t)ranks_dev; c.image_nbytes = (uintptr_t)image_nbytes;
    CurvePlan p;
    const char *why = "";
    int rc = curve_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);

    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    RateTilesArgs a;
    a.ind_c = ind_c; a.ind_m = ind_m; a.ind_f = ind_f; a.e16 = e16; a.e8 = e8;
    a.tiles = tiles_dev; a.ranks = ranks_dev; a.M = (int)M;
    a.summary = reinterpret_cast<int32_t *>(ws + p.off_summary);
    a.tile_nbytes = tile_nbytes ? tile_nbytes : reinterpret_cast<int32_t *>(ws + p.off_tile_nbytes);
    if (p.grid > 0 && (rc = curve_launch(rate_curve_tiles_kernel, "rate_curve_tiles_kernel", t, c, p, a, (hipStream_t)stream))) return rc;
    hipLaunchKernelGGL(rate_fold_tiles_kernel, dim3((unsigned)p.fold_grid_x, (unsigned)p.fold_grid_y), dim3(kFoldThreads), 0, (hipStream_t)stream,
                       tiles_dev, (int)T, (int)M, (const int32_t *)a.tile_nbytes, image_nbytes);
    return launch_check("rate_fold_tiles_kernel");
}

extern "C" size_t cgic_route_to_budget_workspace_bytes(int64_t B, int64_t h16, int64_t w16, int64_t R)
{
    CurveShape s{};
    s.entry = CURVE_BUDGET; s.B = B; s.h16 = h16; s.w16 = w16; s.R = R;
    return curve_workspace_bytes(s);
}

extern "C" int cgic_route_to_budget(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f,
                                    const float *e16, const float *e8, int64_t B, int64_t h16, int64_t w16, double coarse_ratio,
                                    const int32_t *ranks_dev, int64_t R, const int64_t *budget_dev, int32_t *mask_c, int32_t *mask_m,
                                    int32_t *mask_f, int64_t *ind, int64_t *choice_dev, void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_route_to_budget");
    CurveCall c = curve_call(CURVE_BUDGET, t, ind_c, ind_m, ind_f, e16, e8, coarse_ratio, workspace);
    c.shape.B = B; c.shape.h16 = h16; c.shape.w16 = w16; c.shape.R = R;
    c.ranks_dev = (uintptr_t)ranks_dev; c.budget_dev = (uintptr_t)budget_dev; c.choice_dev = (uintptr_t)choice_dev;
    c.mask_c = (uintptr_t)mask_c; c.mask_m = (uintptr_t)mask_m; c.mask_f = (uintptr_t)mask_f; c.ind = (uintptr_t)ind;
    CurvePlan p;
    const char *why = "";
    int rc = curve_plan(c, &p, &why);
    CGIC_REQUIRE(rc == CGIC_OK, rc, "%s", why);

    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    RateRanksArgs a;
    a.ind_c = ind_c; a.ind_m = ind_m; a.ind_f = ind_f; a.e16 = e16; a.e8 = e8;
    a.h16 = (int)h16; a.w16 = (int)w16; a.k_c = (int)p.k_c;
    a.ranks = ranks_dev; a.R = (int)R;
    a.summary = reinterpret_cast<int32_t *>(ws + p.off_summary);
    a.total = reinterpret_cast<int32_t *>(ws + p.off_total);
    a.tkey = reinterpret_cast<uint32_t *>(ws + p.off_tkey);
    if ((rc = curve_launch(rate_curve_ranks_kernel, "rate_curve_ranks_kernel", t, c, p, a, (hipStream_t)stream))) return rc;

    hipLaunchKernelGGL(rate_pick_kernel, dim3((unsigned)p.pick_grid), dim3(kPickThreads), 0, (hipStream_t)stream, (const int32_t *)a.total, ranks_dev,
                       (int)B, (int)R, budget_dev, choice_dev);
    rc = launch_check("rate_pick_kernel");
    if (rc) return rc;

    RateApplyArgs q;
    q.choice = choice_dev; q.tkey = a.tkey; q.summary = a.summary;
    q.ind_c = ind_c; q.ind_m = ind_m; q.ind_f = ind_f; q.e16 = e16; q.e8 = e8;
    q.B = (int)B; q.h16 = (int)h16; q.w16 = (int)w16; q.R = (int)R; q.k_c = (int)p.k_c;
    q.mc = mask_c; q.mm = mask_m; q.mf = mask_f; q.ind = ind;
    hipLaunchKernelGGL(rate_apply_kernel, dim3((unsigned)p.apply_grid), dim3(kApplyThreads), 0, (hipStream_t)stream, q);
    return launch_check("rate_apply_kernel");
}
