// cgic_rate.hip -- exact per-ratio rate tables (the bytes CGIC.compress would write for C candidate granularity ratios,
// CGIC/models/model.py:217-262) without writing a stream, and the gather of the merged latent's indices from per-head ones.
//
// Why it is exact (include/cgic_hip.h, section I): the merge in front of the quantiser (vqvae_blocks.py:361-366) hands every
// grain position exactly one head's vector, quant_conv is per position and the VQ per vector, so the indices of every ratio are
// the per-head VQ indices selected by that ratio's masks; and a Huffman / mask file is `nbits // 8 + 2` bytes (empty list: 0),
// so a stream's size depends on the masks only through the number and the summed code lengths of the symbols it selects.
//
// Two launches for C candidates:
//   1. rate_route_kernel   grid (router workgroups of one candidate) x C: the router's own body (threshold selects, band
//                          refinement from the pixels, mask writing) for candidate blockIdx.y into a [C, ...] mask stack.
//                          Candidates whose refinement needs the launch chain of segments beyond the LDS are routed one by
//                          one through cgic_router_f32 instead (sequential on the caller's stream).
//   2. rate_reduce_kernel  grid B x C: per (image, candidate) the count and the summed code lengths of the selected symbols of
//                          each grain (code lengths staged in LDS, DPP wave reductions), five int32 sizes out.
#include "cgic_rate_plan.h"
#include "cgic_router_dev.h"

namespace cgic {

// (cgic_router.hip)
int refine_source(const cgic_pixels *refine, int64_t h16, int64_t w16, RefineSrc *out);
size_t router_big_scratch_bytes(int64_t B, int64_t h16, int64_t w16, int per_image);

static_assert((size_t)kRateLdsSyms * sizeof(int32_t) <= 64 * 1024, "rate_reduce_kernel stages the code lengths without the dynamic-LDS opt-in");

struct RateRouteArgs {
    RouterArgs base;                         // candidate 0's arguments; the fields below replace its per-candidate ones
    int64_t stride_c, stride_m, stride_f;    // int32 elements of one candidate's masks in the stack
    int mode[kRateMaxCand];
    unsigned int rank_c[kRateMaxCand], rank_m[kRateMaxCand];
    signed char stage[kRateMaxCand], rf_on[kRateMaxCand];
};

__global__ __launch_bounds__(kRouterThreads) void rate_route_kernel(RateRouteArgs r)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int c = (int)blockIdx.y;
    RouterArgs a = r.base;
    a.mask_c += c * r.stride_c;
    a.mask_m += c * r.stride_m;
    a.mask_f += c * r.stride_f;
    a.mode = r.mode[c];
    a.rank_c = r.rank_c[c];
    a.rank_m = r.rank_m[c];
    a.stage = r.stage[c];
    if (!r.rf_on[c]) a.rf.x = nullptr;
    router_body<kRouterThreads, false, false>(a, blockIdx.x, dyn);
}

struct RateReduceArgs {
    const int32_t *len;                      // device [nsym] code lengths (TableDev.len)
    int nsym;
    const int64_t *ind[3];                   // per grain: [B, n[g]]
    const int32_t *mask[3];                  // per grain: the stack [C, B, n[g]]
    int64_t n[3];                            // positions per image: h16 w16, 4 h16 w16, 16 h16 w16
    int64_t stride[3];                       // elements of one candidate's mask in the stack
    int64_t B;
    int streams[kRateMaxCand];               // cgic_mode_streams of each candidate
    int32_t *nbytes;                         // [C, B, 5]
};

__device__ __forceinline__ unsigned int wave_sum_u32(unsigned int v)
{
    return (unsigned int)__builtin_amdgcn_readlane((int)wave_inclusive_scan_u32(v), kWave - 1);
}

__global__ __launch_bounds__(kRateThreads) void rate_reduce_kernel(RateReduceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ unsigned int part[kRateThreads / kWave][3];
    int32_t *slen = reinterpret_cast<int32_t *>(dyn);
    const int tid = threadIdx.x, wave = tid / kWave;
    const int64_t b = blockIdx.x;
    const int c = (int)blockIdx.y;
    const int streams = a.streams[c];
    const bool staged = a.nsym <= kRateLdsSyms;
    if (staged)
        for (int i = tid; i < a.nsym; i += kRateThreads) slen[i] = a.len[i];
    __syncthreads();
    const int32_t *len = staged ? slen : a.len;
    int32_t *out = a.nbytes + ((int64_t)c * a.B + b) * CGIC_NUM_STREAMS;
    for (int g = 0; g < 3; ++g) {
        if (!(streams >> g & 1)) {                       // (uniform over the workgroup)
            if (tid == 0) out[g] = 0;
            continue;
        }
        const int64_t n = a.n[g];
        const int64_t *ind = a.ind[g] + b * n;
        const int32_t *mask = a.mask[g] + (int64_t)c * a.stride[g] + b * n;
        unsigned int bits = 0, cnt = 0, bad = 0;
        for (int64_t i = tid; i < n; i += kRateThreads) {
            if (mask[i] == 1) {                          // ind[...][grain_mask == 1] (model.py:219-221)
                const int64_t s = ind[i];
                if (s < 0 || s >= a.nsym) bad = 1;
                else { bits += (unsigned int)len[s]; ++cnt; }
            }
        }
        bits = wave_sum_u32(bits);
        cnt = wave_sum_u32(cnt);
        bad = wave_sum_u32(bad);
        if ((tid & (kWave - 1)) == 0) { part[wave][0] = bits; part[wave][1] = cnt; part[wave][2] = bad; }
        __syncthreads();
        if (tid == 0) {
            unsigned int tb = 0, tc = 0, tx = 0;
            for (int w = 0; w < kRateThreads / kWave; ++w) { tb += part[w][0]; tc += part[w][1]; tx += part[w][2]; }
            // HuffmanCoding.compress (indices_coding.py:113-124): no symbols -> empty file; else one header byte + the code bits
            // padded by 1..8 zero bits (padding is 8 - nbits % 8, also when nbits % 8 == 0)
            out[g] = tx ? (int32_t)(CGIC_ERR_INVALID - 10) : tc == 0 ? 0 : (int32_t)(tb / 8u + 2u);
        }
        __syncthreads();
    }
    if (tid == 0) {
        // BinaryCoding.compress of the flattened int32 masks (mask_coding.py): one bit per element, never empty
        out[3] = (streams >> 3 & 1) ? (int32_t)(a.n[0] / 8 + 2) : 0;
        out[4] = (streams >> 4 & 1) ? (int32_t)(a.n[1] / 8 + 2) : 0;
    }
}

struct GatherArgs {
    const int64_t *ind_c, *ind_m, *ind_f;
    const int32_t *mc, *mm, *mf;
    int64_t B, h, w;
    int64_t *out;
};

__global__ __launch_bounds__(256) void gather_grain_indices_kernel(GatherArgs a)
{
    const int64_t hw = a.h * a.w, total = a.B * hw;
    const int64_t hm = a.h >> 1, wm = a.w >> 1, hc = a.h >> 2, wc = a.w >> 2;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / hw, r = i - b * hw, y = r / a.w, x = r - y * a.w;
        int64_t v;
        if (a.mf[i] == 1) v = a.ind_f[i];
        else {
            const int64_t im = (b * hm + (y >> 1)) * wm + (x >> 1);
            if (a.mm[im] == 1) v = a.ind_m[im];
            else v = a.ind_c[(b * hc + (y >> 2)) * wc + (x >> 2)];
        }
        a.out[i] = v;
    }
}

}  // namespace cgic

using namespace cgic;

extern "C" size_t cgic_rate_table_workspace_bytes(int64_t B, int64_t h16, int64_t w16, int C, int per_image)
{
    RateTablePlan p;
    const char *why = "";
    return rate_table_form(B, h16, w16, C, &p, &why) == CGIC_OK ? p.workspace_needed : 0;
}

extern "C" int cgic_rate_table(const cgic_table *t, const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f,
                               const float *e16, const float *e8, int64_t B, int64_t h16, int64_t w16, int C,
                               const double *coarse, const double *medium, int per_image, const cgic_pixels *refine,
                               int32_t *nbytes, void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_rate_table");
    RateTableCall call{};
    call.table = t != nullptr;
    if (t) { call.nsym = cgic_table_num_symbols(t); call.max_len = cgic_table_max_len(t); }
    call.B = B; call.h16 = h16; call.w16 = w16; call.C = C;
    call.inputs = ind_c && ind_m && ind_f && e16 && e8 && nbytes && coarse && medium;
    call.workspace = (uintptr_t)workspace;
    RateTablePlan p;
    const char *why = "";
    const int prc = rate_table_plan(call, &p, &why);
    CGIC_REQUIRE(prc == CGIC_OK, prc, "%s", why);
    if (p.nothing_to_do) return CGIC_OK;
    const int64_t n16 = h16 * w16, sc = p.stride_c, sm = p.stride_m, sf = p.stride_f;
    unsigned char *ws = reinterpret_cast<unsigned char *>(workspace);
    int32_t *stk_c = reinterpret_cast<int32_t *>(ws + p.off_c);
    int32_t *stk_m = reinterpret_cast<int32_t *>(ws + p.off_m);
    int32_t *stk_f = reinterpret_cast<int32_t *>(ws + p.off_f);

    // ---- every candidate is checked before anything is enqueued (router_plan_args' checks; for the launch chain of segments
    // beyond the LDS also router_big's: the scratch, the pixels, the final launch's arguments)
    const bool have_px = refine && refine->x;
    cgic_pixels px_plain;                    // the pixels without the scratch: the one-launch form takes no refinement queues
    if (have_px) { px_plain = *refine; px_plain.scratch = nullptr; px_plain.scratch_bytes = 0; }
    RateRouteArgs ra;
    memset(&ra, 0, sizeof(ra));
    int64_t nwg = 0;
    size_t lds = 0;
    bool chain = false;                      // some candidate takes router_big: route every candidate through cgic_router_f32
    for (int c = 0; c < C; ++c) {
        const int mode = cgic_router_mode(coarse[c], medium[c]);
        int32_t *mc = stk_c + c * sc, *mm = stk_m + c * sm, *mf = stk_f + c * sf;
        RouterArgs a;
        RouterPlan rp;
        int rc;
        if (have_px && mode <= 3 && !router_refine_in_lds(B, h16, w16, per_image)) {
            const size_t sneed = router_big_scratch_bytes(B, h16, w16, per_image);
            CGIC_REQUIRE(refine->scratch && refine->scratch_bytes >= sneed, CGIC_ERR_INVALID,
                         "rate_table: candidate %d (%g, %g): a routing segment beyond the LDS is refined through patched copies of the "
                         "maps: cgic_pixels.scratch of %zu bytes needed (cgic_router_refine_scratch_bytes), %zu given", c, coarse[c],
                         medium[c], sneed, refine->scratch ? refine->scratch_bytes : (size_t)0);
            CGIC_REQUIRE(((uintptr_t)refine->scratch & 15u) == 0, CGIC_ERR_INVALID, "rate_table: the refinement scratch must be 16-byte aligned");
            RefineSrc rs;
            rc = refine_source(refine, h16, w16, &rs);
            if (rc) return rc;
            const float *e16x = reinterpret_cast<const float *>(refine->scratch), *e8x = e16x + B * n16;
            rc = router_plan_args(e16x, e8x, B, h16, w16, coarse[c], medium[c], per_image, mc, mm, mf, nullptr, 96 * 1024, nullptr, false, &rp, &a);
            if (rc) return rc;
            chain = true;
            continue;
        }
        rc = router_plan_args(e16, e8, B, h16, w16, coarse[c], medium[c], per_image, mc, mm, mf, nullptr, 96 * 1024,
                              have_px ? &px_plain : nullptr, false, &rp, &a);
        if (rc) return rc;
        const int64_t nseg = rp.wgs;
        const size_t l = rp.lds;
        if (c == 0 || (!ra.base.rf.x && a.rf.x)) ra.base = a;      // (the base carries the pixels if any candidate refines)
        CGIC_REQUIRE(nwg == 0 || nwg == nseg, CGIC_ERR_INVALID, "rate_table: candidates disagree on the router's grid");
        nwg = nseg;
        if (l > lds) lds = l;
        ra.mode[c] = a.mode;
        ra.rank_c[c] = a.rank_c;
        ra.rank_m[c] = a.rank_m;
        ra.stage[c] = (signed char)a.stage;
        ra.rf_on[c] = a.rf.x != nullptr;
    }
    TableDev tab;
    int rc = table_device_view(t, &tab);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;

    // ---- 1. the masks of every candidate
    if (chain) {
        // (sequential on the caller's stream: at most one launch that carries the refinement scratch in flight at a time)
        for (int c = 0; c < C; ++c) {
            rc = cgic_router_f32(e16, e8, B, h16, w16, coarse[c], medium[c], per_image, stk_c + c * sc, stk_m + c * sm, stk_f + c * sf,
                                 nullptr, nullptr, refine, stream);
            if (rc) return rc;
        }
    } else {
        ra.base.mask_c = stk_c; ra.base.mask_m = stk_m; ra.base.mask_f = stk_f;
        ra.base.gate = nullptr;
        ra.stride_c = sc; ra.stride_m = sm; ra.stride_f = sf;
        if (lds > 64 * 1024) { rc = ensure_dynamic_lds((const void *)rate_route_kernel, lds); if (rc) return rc; }
        hipLaunchKernelGGL(rate_route_kernel, dim3((unsigned)nwg, (unsigned)C), dim3(kRouterThreads), lds, s, ra);
        rc = launch_check("rate_route_kernel");
        if (rc) return rc;
    }

    // ---- 2. the sizes
    RateReduceArgs r;
    r.len = tab.len; r.nsym = call.nsym;
    r.ind[0] = ind_c; r.ind[1] = ind_m; r.ind[2] = ind_f;
    r.mask[0] = stk_c; r.mask[1] = stk_m; r.mask[2] = stk_f;
    r.n[0] = n16; r.n[1] = 4 * n16; r.n[2] = 16 * n16;
    r.stride[0] = sc; r.stride[1] = sm; r.stride[2] = sf;
    r.B = B;
    for (int c = 0; c < kRateMaxCand; ++c) r.streams[c] = c < C ? cgic_mode_streams(cgic_router_mode(coarse[c], medium[c])) : 0;
    r.nbytes = nbytes;
    hipLaunchKernelGGL(rate_reduce_kernel, dim3((unsigned)p.grid_x, (unsigned)p.grid_y), dim3(kRateThreads), p.lds_bytes, s, r);
    return launch_check("rate_reduce_kernel");
}

extern "C" int cgic_gather_grain_indices(const int64_t *ind_c, const int64_t *ind_m, const int64_t *ind_f, const int32_t *mask_c,
                                         const int32_t *mask_m, const int32_t *mask_f, int64_t B, int64_t h, int64_t w,
                                         int64_t *ind_out, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_gather_grain_indices");
    CGIC_REQUIRE(ind_c && ind_m && ind_f && mask_c && mask_m && mask_f && ind_out, CGIC_ERR_INVALID, "gather_grain_indices: NULL argument");
    CGIC_REQUIRE(B >= 0 && h > 0 && w > 0 && h % 4 == 0 && w % 4 == 0, CGIC_ERR_INVALID,
                 "gather_grain_indices: latent grid %lldx%lld must be positive multiples of 4", (long long)h, (long long)w);
    if (B == 0) return CGIC_OK;
    GatherArgs a;
    a.ind_c = ind_c; a.ind_m = ind_m; a.ind_f = ind_f; a.mc = mask_c; a.mm = mask_m; a.mf = mask_f;
    a.B = B; a.h = h; a.w = w; a.out = ind_out;
    const int64_t total = B * h * w;
    int64_t g = (total + 255) / 256;
    if (g > 4096) g = 4096;
    hipLaunchKernelGGL(gather_grain_indices_kernel, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, a);
    return launch_check("gather_grain_indices_kernel");
}
