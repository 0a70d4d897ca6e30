// cgic_encode_plan.h -- what the router launch and the VQ (+ router) launch of the encode side look like, decided before a ticket
// is requested or anything is enqueued.
// Plain C++17 on purpose (no HIP include, no stream, no device pointer): router_plan() and vq_plan() are pure functions of a
// RouterShape / VqShape, so every decision of the encode host path can be exercised without a GPU (tests/host/encode_plan_main.cpp).
// cgic_router.hip and cgic_vq.hip check the arguments, call the plans and issue what they say.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/cgic_hip.h"

namespace cgic {

// ===== the router =====================================================================================================

// LDS budget of a router workgroup in the fused VQ + router launch (two allocations per 160 KB CU); refinement is offered
// for segments that fit THIS budget, in the stand-alone launch too, so that one answer holds for both
constexpr size_t kRouterFusedLds = (size_t)78 * 1024;
constexpr size_t kRouterLdsMax = 150 * 1024;        // dynamic LDS a router workgroup may ask for
constexpr int kRefBitWords = 176;          // 64-bit words of the band's member bitmap: 11264 elements, more than any segment whose maps fit kRouterFusedLds
constexpr int64_t kRouterMaxQueues = 4096;          // refinement queues (two per segment) that one launch can have

// RouterTriple.py:13: fine = 1 - coarse - medium in float64; :19,36,72
inline int router_mode(double c, double m)
{
    volatile double f = 1.0 - c - m;
    int nz = (f == 0) + (m == 0) + (c == 0);
    if (nz == 0) return 0;
    if (nz == 1) return c == 0 ? 1 : (m == 0 ? 2 : 3);
    return c != 0 ? 4 : (m != 0 ? 5 : 6);
}

// stage 1: e16 and e8 live in LDS (e8 is masked in place for the medium select); stage 2: only e8 (e16 is read from global
// memory by the coarse select's four passes); 0: nothing staged.  `budget`: the fused VQ + router launch keeps a router
// workgroup under half a CU's LDS so that it can share the CU with a VQ workgroup.  `refine`: room for RefineShared behind
// the maps (stage 1 only; *stage = -1 if that does not fit the budget).  `shared_bytes`, `refine_bytes`: kRouterSharedBytes and
// sizeof(RefineShared) of cgic_router_dev.h.
inline size_t router_lds_bytes(int64_t N16, int64_t N8, int *stage, size_t budget, bool refine, size_t shared_bytes, size_t refine_bytes)
{
    size_t lds = shared_bytes + 8 * (size_t)((N16 + 63) / 64);
    int st = 0;
    if (refine) {
        const size_t need = lds + 4 * (size_t)(N16 + N8) + 16 + refine_bytes;
        if (need <= budget) { st = 1; lds = need; } else st = -1;
    } else if (lds + 4 * (size_t)(N16 + N8) <= budget) { st = 1; lds += 4 * (size_t)(N16 + N8); }
    else if (lds + 4 * (size_t)N8 <= budget) { st = 2; lds += 4 * (size_t)N8; }
    if (stage) *stage = st;
    return lds;
}

// a segment of N16 coarse patches is refined inside its router workgroup (else: as a chain of launches, cgic_router.hip: router_big)
inline bool router_refine_fits(int64_t N16, size_t shared_bytes, size_t refine_bytes)
{
    int st = 0;
    router_lds_bytes(N16, 4 * N16, &st, kRouterFusedLds, true, shared_bytes, refine_bytes);
    return st == 1 && 4 * N16 <= 64 * (int64_t)kRefBitWords;
}

// payload of a segment's two refinement queues in the caller's scratch (constexpr: the device side reads it too) ...
constexpr size_t refine_scratch_bytes_per_segment(int64_t N16, int64_t N8) { return 24 * (size_t)(N16 + N8); }
// ... and of a launch's; 0: more segments than a launch can have queues for
inline size_t router_queue_scratch_bytes(int64_t nseg, int64_t N16)
{
    return 2 * nseg <= kRouterMaxQueues ? (size_t)nseg * refine_scratch_bytes_per_segment(N16, 4 * N16) : 0;
}

// Python's round() of the float64 product n * ratio (RouterTriple.py:23,30,42,54,65): round-half-even
inline double rank_round(int64_t n, double ratio) { return nearbyint((double)n * ratio); }

// THE rank arithmetic: the reference's two k for a segment of N16 coarse patches in `mode`, 0 where the mode uses none.  false: a k
// outside its list (the reference raises IndexError).  As float64, the way they are made: a NaN or a huge ratio gives no integer
inline bool router_ranks(int mode, int64_t N16, double c_ratio, double m_ratio, double *k_c, double *k_m)
{
    const int64_t N8 = 4 * N16;
    *k_c = *k_m = 0;
    if (mode == 0 || mode == 2 || mode == 3) *k_c = rank_round(N16, c_ratio);
    if (mode == 0) *k_m = nearbyint((double)(4 * N16) * c_ratio + (double)N8 * m_ratio);
    if (mode == 1) *k_m = rank_round(N8, m_ratio);
    return *k_c >= 0 && *k_c <= (double)N16 && *k_m >= 0 && *k_m <= (double)N8;
}

struct RouterShape {
    int64_t B, h16, w16;        // images, coarse grid of one image
    double c_ratio, m_ratio;
    bool per_image;             // a segment per image (else: the reference's routing over the flattened batch)
    bool refine;                // the pixels behind the maps are given
    bool has_scratch;           // ... and a scratch for the refinement queues, of
    size_t scratch_bytes;
    bool queues;                // the caller wants the launch's refinement queues (the stand-alone launch)
    size_t lds_budget;          // of a router workgroup in this launch
    size_t lds_shared, lds_refine;      // kRouterSharedBytes, sizeof(RefineShared): device struct sizes (router_lds_bytes)
};

// why a plan failed, in the order of the checks (the call site words the message; it checks the pixel source after ROUTER_K_RANGE)
enum RouterWhy { ROUTER_PLANNED, ROUTER_SEGMENT_TOO_LARGE, ROUTER_K_RANGE, ROUTER_LDS_FIT, ROUTER_REFINE_PATCHES, ROUTER_LDS_MAX, ROUTER_SCRATCH_SMALL };

struct RouterPlan {
    int mode;
    int64_t per, nseg;          // images per segment, segments
    int64_t N16, N8;            // coarse and medium patches of a segment
    int64_t k_c, k_m;           // the reference's two k ...
    unsigned int rank_c, rank_m;        // ... and the 0-based ranks of the thresholds
    unsigned int mg_n8, mg_w8, mg_n4, mg_w4;    // magic multipliers of the index divisions
    bool refined;               // the launch re-evaluates threshold bands from the pixels (modes 4-6 compare nothing)
    int stage;                  // RouterArgs::stage
    size_t lds;
    int bands;                  // workgroups per segment
    int64_t wgs;                // workgroups of the launch: nseg * bands
    unsigned int nq;            // refinement queues of the launch (0: none, no ticket is requested)
    size_t scratch_need;        // bytes of the caller's scratch the queues take
};

// CGIC_OK and the plan, or the error code of the call and *why (the plan is filled as far as the failed check: the messages name k, N16, N8)
inline int router_plan(const RouterShape &s, RouterPlan *p, RouterWhy *why)
{
    *p = RouterPlan{};
    *why = ROUTER_PLANNED;
    const int mode = p->mode = router_mode(s.c_ratio, s.m_ratio);
    p->per = s.per_image ? 1 : s.B;
    const int64_t nseg = p->nseg = s.per_image ? s.B : 1;
    const int64_t N16 = p->N16 = p->per * s.h16 * s.w16, N8 = p->N8 = 4 * N16;
    if (!(N8 < (int64_t)1 << 31)) { *why = ROUTER_SEGMENT_TOO_LARGE; return CGIC_ERR_UNSUPPORTED; }
    double k_c, k_m;
    const bool in_range = router_ranks(mode, N16, s.c_ratio, s.m_ratio, &k_c, &k_m);
    // (for the message of a k out of range: what has no int64 reads as the smallest one, as the conversion instruction gives it)
    const auto whole = [](double k) { return k >= -9.0e18 && k <= 9.0e18 ? (int64_t)k : INT64_MIN; };
    p->k_c = whole(k_c); p->k_m = whole(k_m);
    if (!in_range) { *why = ROUTER_K_RANGE; return CGIC_ERR_INVALID; }
    p->rank_c = (unsigned int)(p->k_c != 0 ? p->k_c - 1 : 0);      // sorted[k-1 if k != 0 else k]
    p->rank_m = (unsigned int)(p->k_m != 0 ? p->k_m - 1 : 0);
    {
        // magic multipliers of the index divisions (cgic_router_dev.h: fdiv): exact while (largest dividend) x (divisor) < 2^32
        const int64_t n8 = 4 * s.h16 * s.w16, n4 = 16 * s.h16 * s.w16, w8 = 2 * s.w16, w4 = 4 * s.w16;
        auto magic = [](int64_t nmax, int64_t d) -> unsigned int {
            return (d > 1 && nmax * d < ((int64_t)1 << 32)) ? (unsigned int)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d) : 0u;
        };
        p->mg_n8 = magic(N8, n8); p->mg_w8 = magic(n8, w8);
        p->mg_n4 = magic(4 * N8, n4); p->mg_w4 = magic(n4, w4);
    }
    p->refined = s.refine && mode <= 3;          // (modes 4-6 compare nothing)
    // (with refinement every segment must fit the FUSED launch's budget, so that the stand-alone and the fused launch accept
    // the same shapes)
    p->lds = router_lds_bytes(N16, N8, &p->stage, p->refined ? (s.lds_budget < kRouterFusedLds ? s.lds_budget : kRouterFusedLds) : s.lds_budget,
                              p->refined, s.lds_shared, s.lds_refine);
    if (p->stage < 0) { *why = ROUTER_LDS_FIT; return CGIC_ERR_UNSUPPORTED; }
    if (p->refined && N8 > 64 * (int64_t)kRefBitWords) { *why = ROUTER_REFINE_PATCHES; return CGIC_ERR_UNSUPPORTED; }
    // large per-image segments: several workgroups per image share the mask writing (every one repeats the selects, which
    // costs nothing while most CUs are idle): up to 8, while the launch stays within ~a quarter of the chip
    // (The row bands of a tile that split a threshold band WAIT for each other (refine_select's exchange()): every band of every launch
    // in flight has to be resident.  nseg x bands <= 64 workgroups per launch = a quarter of the chip's CUs, two such workgroups fit a
    // CU: up to FOUR launches in flight -- the pipeline's four hardware queues -- are resident together whatever else runs; more
    // concurrent launches than that are outside the contract of cgic_pixels.scratch, see include/cgic_hip.h.)
    p->bands = 1;
    if (s.per_image && s.h16 * s.w16 >= 32 * 32) {
        int64_t nb = 64 / nseg;
        if (nb > 8) nb = 8;
        if (nb > s.h16) nb = s.h16;
        p->bands = nb >= 2 ? (int)nb : 1;
    }
    p->wgs = nseg * p->bands;
    if (p->lds > kRouterLdsMax) { *why = ROUTER_LDS_MAX; return CGIC_ERR_UNSUPPORTED; }
    // the launch's refinement queues: one header per (segment, select) + the board, in library-owned slots (a pool of their own); payload in the caller's scratch
    // (the fused launch, queues == false, uses headers + scratch only for the row bands' exchange: segments with bands > 1)
    const size_t need = router_queue_scratch_bytes(nseg, N16);
    if ((s.queues || p->bands > 1) && p->refined && s.has_scratch && need != 0) {
        p->scratch_need = need;
        if (s.scratch_bytes < need) { *why = ROUTER_SCRATCH_SMALL; return CGIC_ERR_INVALID; }
        p->nq = (unsigned int)(2 * nseg);
    }
    return CGIC_OK;
}

// ===== the VQ launch, alone or with the router's workgroups in it ======================================================

constexpr int kVqThreads = 256;   // 4 waves
constexpr int kVqMaxK = 8192;
constexpr int kVqfMaxK = 1024;
constexpr int kVqfGroup = 64;                  // vectors per group: two tiles of 32 (one lane per vector in the decide step)
constexpr int kVqfThreads = 512;      // one workgroup per CU, 2 waves per SIMD.  Alone at B=64 x 64x64 latents 512 / 768 / 1024 threads are within 1 us of each other; with several batches in flight (bench.py --lanes 4) 512 leaves a third of the register file to the other batches' kernels: 86.9 vs 83.4 (768) vs 82.9 (1024) GPixel/s
// 128 registers per lane (4-10 spilled, 20-44 bytes of scratch) instead of 144-150: two 512-thread workgroups then fit a CU's
// register file, so a ROUTER workgroup of the fused launch (same launch => same allocation) shares its CU with a VQ workgroup
// instead of holding the CU to itself for ~12 us: fused launch 26.3 -> 24.1 us at B=64 (the VQ kernel alone: 23.3 -> 23.8 on the
// same GPU), no uneven split of the VQ shares needed any more.
constexpr int kVqfVgprCap = 128;

// The time model behind the placement of the router workgroups, in microseconds.  t_router: how long a router workgroup holds its
// CU when it has it to itself (~11 us at 256x256; measured 12 us at 64x64 latents, 21 us at 192x192 with its row bands), by the
// vectors `hw` of an image.  t_vq: a VQ workgroup that owns `per` groups.
inline double t_router(int64_t hw) { return 10.9 + 0.000275 * (double)hw; }
inline double t_vq(int64_t per) { return 3.0 + 1.25 * (double)per; }
constexpr double kRouterBesideVq = 1.6;         // beside an issue-bound VQ workgroup a router runs ~1.6x slower than alone
constexpr double kVqGroupUs = 1.05;             // a group of VQ work per workgroup (~1.05 us each)

enum VqPath { VQ_FILTER, VQ_EXACT };
enum VqVariant { VQ_PLAIN, VQ_PERM, VQ_ROUTER, VQ_ROUTER_PERM, VQ_ROUTER_SPLIT };

struct VqShape {
    int64_t N, hw;              // vectors, vectors per image
    int K;                      // codebook rows
    bool conv;                  // a quant_conv is fused in front of the quantiser
    bool loss;                  // the call wants the loss
    bool perm_image;            // the prepared codebook image is a permuted one (as registered: the plan decides whether that counts)
    int cus;                    // compute units of the device
    double cu_share;            // the launch group's share of them ...
    bool recording;             // ... which counts while a group is being recorded
    int64_t router_wgs;         // router workgroups in the launch (0: none), with
    size_t router_lds;          // their LDS, and
    bool router_queues;         // whether they have refinement queues (RouterPlan::nq != 0)
    size_t lds_filter;          // LDS of the filter path for this K (vqf_lds_bytes: it mirrors the device's layout)
    int kid_aligned, kid_unaligned;     // recorded forms of the fused filter launch (KernelId of cgic_common.h; plain numbers here)
    // dev knobs CGIC_VQ_EXACT, CGIC_VQ_ZT, CGIC_VQ_WGS_PER_CU, CGIC_VQ_NOSPLIT, CGIC_VQ_GE (0: not set)
    int knob_exact, knob_zt, knob_wgs_per_cu, knob_nosplit, knob_ge;
};

struct VqPlan {
    VqPath path;
    int zt;                     // VQ_EXACT: tiles per wave
    bool aligned;               // hw is a multiple of a group: no group straddles two images
    VqVariant variant;          // (VQ_EXACT knows VQ_PLAIN and VQ_ROUTER only)
    int64_t nblk;               // VQ workgroups; VQ_FILTER: workgroups [0, n_early) own g_early groups each, the rest g_late
    int64_t n_early, g_early, g_late;
    bool router_behind;         // the router workgroups follow the VQ workgroups in the grid (else they come first)
    int64_t grid;               // nblk + the router's workgroups
    int threads;
    size_t lds;
    unsigned int tail_mode;     // VqArgs::tail_mode
    int tickets;                // ticket slots to request for the loss hand-off (0: none)
    int kid;                    // recorded form of the launch inside a launch group (0: it is launched on its own)
};

// CGIC_OK and the plan, or the error code of the call and *why
inline int vq_plan(const VqShape &s, VqPlan *p, const char **why)
{
    *p = VqPlan{};
    const int64_t N = s.N, hw = s.hw;
    const int K = s.K;
    const bool router = s.router_wgs != 0;
    p->aligned = hw % kVqfGroup == 0;
    if (s.knob_exact || K % 64 != 0 || K > kVqfMaxK) {
        static_assert(kVqfMaxK == 1024, "the message below names the bound");
        if (s.conv) { *why = "vq: the fused quant_conv needs K % 64 == 0 and K <= 1024"; return CGIC_ERR_UNSUPPORTED; }
        // exact loop; per-wave tile: measured on MI355X (tools/probes/probe_vq.hip) ZT=4 at 4 waves/SIMD is the fastest
        // for large N; smaller N shrinks the tile so that all 256 CUs get work
        const int f = s.knob_zt;          // dev: tile count of the exact loop
        p->path = VQ_EXACT;
        p->zt = (f == 8 || f == 4 || f == 2 || f == 1) ? f : N >= (int64_t)1 << 22 ? 8 : N >= (int64_t)256 * 512 ? 4 : N >= (int64_t)128 * 512 ? 2 : 1;
        const int64_t per_block = 4 * 16 * p->zt;
        p->nblk = (N + per_block - 1) / per_block;
        p->variant = router ? VQ_ROUTER : VQ_PLAIN;
        // (no grouped form: inside a launch group this position is launched group by group)
        p->grid = p->nblk + s.router_wgs;
        p->threads = kVqThreads;
        p->lds = sizeof(float) * (size_t)K * 5;
        if (router && s.router_lds > p->lds) p->lds = s.router_lds;
        return CGIC_OK;
    }
    p->path = VQ_FILTER;
    p->threads = kVqfThreads;
    int cus = s.cus;
    const int64_t ngroups = (N + kVqfGroup - 1) / kVqfGroup;
    // one resident workgroup per CU; its waves take groups from a counter.  Fewer groups than CUs x waves: spread them
    // over the CUs first (a small batch then costs one staging + one group per CU, whatever the waves per workgroup)
    if (s.knob_wgs_per_cu > 1) cus *= s.knob_wgs_per_cu;      // dev: several resident workgroups per CU
    if (s.recording) {          // one shape group of a grouped launch: its share of the chip
        cus = (int)((double)cus * s.cu_share + 0.5);
        cus = cus < 1 ? 1 : cus;
    }
    const int64_t nblk = ngroups < cus ? ngroups : cus;
    p->nblk = nblk;
    // the ticket and, behind it, one 8-byte partial per workgroup: library-owned, zero when handed out, zeroed again by the launch
    // (finish_loss_wave); the caller's workspace is not touched by this path
    p->tickets = s.loss ? 1 + (int)((nblk + 7) / 8) : 0;
    p->tail_mode = s.loss ? 2u : 0u;                   // workgroup 0 collects (VqArgs::tail_mode)
    // groups per workgroup.  Router workgroups in front: the `late` VQ workgroups that must wait for a router's CU
    // (~11 us at 256x256, ~`delta` groups of VQ work) own `g_late` groups, the others `g_early`, a multiple of 4
    const int64_t per = (ngroups + nblk - 1) / nblk;
    int64_t g_early = per, g_late = per, n_early = nblk;
    const int64_t late = router ? nblk + s.router_wgs - cus : 0;
    bool router_first = false;
    // A router workgroup can share its CU with a VQ workgroup.  Behind the VQ workgroups in the grid (every VQ workgroup gets a
    // CU at once and keeps its even share, the routers move in beside them) the router is free as long as it ends before the VQ
    // does -- beside an issue-bound VQ workgroup it runs ~1.6x slower than alone: 64 images of 256x256 24.1 us fused against
    // 23.5 for the VQ alone (in front with even shares: 27.1 -- the VQ workgroups pair up on the free CUs).  Few large tiles
    // (8 of 768x768: router 21 us alone, VQ 26) keep the older scheme: routers in front, uneven VQ shares.
    const bool coresident = kVqfVgprCap <= 128 && router && kRouterBesideVq * t_router(hw) <= t_vq(per);
    if (!coresident && late > 0 && late < nblk && !s.knob_nosplit) {
        // how long a router workgroup holds its CU, in groups of VQ work (~1.05 us each per workgroup): measured 12 us at
        // 64x64 latents, 21 us at 192x192 (with its row bands)
        const int64_t delta = (int64_t)(t_router(hw) / kVqGroupUs + 0.5);
        for (int64_t ge = s.knob_ge ? s.knob_ge : (per / 4 + 1) * 4; ge <= per + 28; ge += 4) {
            const int64_t rest = ngroups - (nblk - late) * ge;
            const int64_t gl = rest > 0 ? (rest + late - 1) / late : 0;
            // (gl == 0: the router outlasts the whole VQ -- the early workgroups simply take everything)
            if (gl + delta <= ge || gl == 0) { g_early = ge; g_late = gl; n_early = nblk - late; router_first = true; break; }
        }
    }
    p->n_early = n_early; p->g_early = g_early; p->g_late = g_late;
    p->router_behind = !router_first;
    p->grid = nblk + s.router_wgs;
    p->lds = s.lds_filter;
    // a prepared image packed by cluster takes the PERM kernels (their own instantiations; inside a launch group and with a fused
    // quant_conv the plain kernels run: they do not trust the permuted image's tag and derive their own)
    const bool perm = !s.conv && !s.recording && s.perm_image;
    if (perm) p->lds += 4 * (size_t)K;
    if (!router) {
        p->variant = perm ? VQ_PERM : VQ_PLAIN;
        return CGIC_OK;
    }
    if (s.router_lds > p->lds) p->lds = s.router_lds;
    // row bands that share a threshold band's re-evaluation run the SPLIT instantiation (cgic_router_dev.h: router_body)
    // ... and images with a workgroup of their own whose band is long start over with the launch's refinement queues (round 6)
    p->variant = perm ? VQ_ROUTER_PERM : s.router_queues ? VQ_ROUTER_SPLIT : VQ_ROUTER;
    if (!perm) p->kid = s.conv ? 0 : p->aligned ? s.kid_aligned : s.kid_unaligned;
    return CGIC_OK;
}

}  // namespace cgic
