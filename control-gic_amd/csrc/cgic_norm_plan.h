// cgic_norm_plan.h -- what one call of cgic_spatial_norm does, decided before anything is enqueued: every check of the call, the
// form (one launch or two), the unit (consecutive elements per thread and access), the chunking of the statistics and the grids.
// Plain C++17 on purpose (no HIP include, no stream; pointers are plain addresses): norm_plan() is a pure function of a NormCall,
// so all of it can be exercised without a GPU (tests/host/norm_plan_main.cpp).  cgic_norm.hip fills a NormCall, calls norm_plan()
// once and launches what the plan says.
//
// The two forms.  A group (b, g) of GroupNorm is one contiguous span of (C / groups) * H * W elements.
//   one launch  : one workgroup of kNormOneThreads threads per span; it reads the span into LDS (in the feature type), reduces,
//                 then applies from LDS.  Chosen when BOTH hold:
//                   (1) the span fits the budget:      span * sizeof(feature element) <= kNormLdsBudget
//                   (2) the grid is not too small:     B * groups >= kNormMinSpansOneLaunch (fewer workgroups than that leave
//                                                      more than half of the chip's 256 CUs without one)
//   two launches: norm_stats_kernel on a grid of (span, chunk) -- every chunk writes one (sum, sum of squares) pair of doubles to
//                 the caller's workspace (and the span's first element, K, once per span) -- and norm_apply_kernel, element-wise, whose workgroups add their span's `chunks`
//                 partials in chunk order.  Ordered by the stream; no workgroup waits for another.
// The chunk count depends on the shape alone (not on the pointers), so the workspace can be sized without them.
// NormCall::plain (value-initialised: false, the modulated call) plans cgic_group_norm: no zq grid is checked, the pointers of zq,
// conv_y and conv_b are neither required nor overlap-tested, every other check is the same under the name group_norm.
// norm_zq_geom, norm_inputs and norm_unit say the rules that the backward's plan (cgic_norm_bwd_plan.h) shares with this one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../include/cgic_hip.h"

namespace cgic {

constexpr int kNormZq = 4;                          // channels of zq (the codebook's e_dim)
constexpr int kNormOneThreads = 512;                // the one-launch form's workgroup
constexpr int kNormThreads = 256;                   // the statistics and the apply workgroups
constexpr int64_t kNormLdsBudget = 64 * 1024;       // (1): bytes of a span that one workgroup holds
constexpr int64_t kNormMinSpansOneLaunch = 128;     // (2)
constexpr int kNormMaxChunks = 32;                  // partials per span that an apply workgroup adds, at most
constexpr int64_t kNormChunkMinElems = 1024;        // a chunk is at least this long (a shorter span: one chunk)
constexpr int64_t kNormStatsGridTarget = 4096;      // chunks stop multiplying once spans * chunks reaches this many workgroups
constexpr int kNormPartUnits = 4 * kNormThreads;    // units of one channel that an apply workgroup takes per step
constexpr int kNormApplyGridCap = 16384;            // 64 workgroups per CU, grid-stride beyond

constexpr int norm_dtype_bytes(int dt) { return dt == CGIC_DT_F32 ? 4 : 2; }

struct NormCall {
    int in_dtype, out_dtype;        // CGIC_DT_*
    int64_t B;
    int64_t C, H, W;
    int64_t hq, wq;                 // zq's grid
    int64_t groups;
    uintptr_t f, zq, gn_weight, gn_bias, wy, by, wb, bb, out;
    uintptr_t workspace;
    size_t workspace_bytes;
    bool plain;                     // cgic_group_norm: no zq and no conv_y / conv_b (hq, wq and their five pointers are not looked at)
};

// how the kernels index a row and zq under it (norm_zq_geom): the part that the forward's plan and the backward's both are
struct NormZqGeom {
    int ymul, ydiv, xmul, xdiv;     // the nearest index: src = dst * mul / div, one of the two being 1 on each axis
    unsigned int mg_w, mg_y, mg_x;  // magic multipliers of the kernels' divisions by W, ydiv, xdiv (norm_magic; 0: divide)
    bool zq_vec;                    // x at ratio 1 and zq 16-byte aligned: a thread reads its pixels of a zq channel in one access
};

struct NormPlan : NormZqGeom {
    int form;                       // 1: one launch; 2: statistics + apply; 0: nothing to launch (an empty batch)
    int unit;                       // consecutive elements of a row per thread and access: 8 (halves only), 4, 2 or 1
    int64_t span;                   // elements of a group
    int64_t spans;                  // B * groups
    int chunks;                     // partials per span (two launches); their number is a function of the shape alone
    int64_t chunk_units;            // units of a chunk (the last one of a span may be shorter)
    int threads_one, threads;       // per workgroup: the one-launch form, the two kernels of the other
    int64_t grid_one, grid_stats, grid_apply;
    int64_t parts;                  // apply: steps of kNormPartUnits units per channel
    size_t lds_bytes;               // one launch: the span (rounded up to 16 bytes) and the waves' partial sums behind it
    size_t workspace_needed;        // bytes; 0 for one launch
    bool in_place;                  // out is f
    char why_text[224];
};

// the name under which a call's checks speak: the modulated layer's or, for the plain call, the GroupNorm's
inline const char *norm_name(bool plain) { return plain ? "group_norm" : "spatial_norm"; }

// the part of the plan that the shape alone decides: the checks of (dtype, B, C, H, W, groups) under the call's name `nm`, the form,
// the chunks and the workspace.  cgic_spatial_norm_workspace_bytes and cgic_spatial_norm_one_launch are this function.
inline int norm_form(const char *nm, int in_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t groups, NormPlan *p, const char **why)
{
    *p = NormPlan{};
    p->threads_one = kNormOneThreads;
    p->threads = kNormThreads;
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    if (in_dtype != CGIC_DT_F32 && in_dtype != CGIC_DT_F16 && in_dtype != CGIC_DT_BF16) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: in_dtype %d (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)", nm, in_dtype);
        return refuse(CGIC_ERR_INVALID);
    }
    if (B < 0 || C <= 0 || H <= 0 || W <= 0) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: features [%lld,%lld,%lld,%lld]", nm, (long long)B, (long long)C, (long long)H, (long long)W);
        return refuse(CGIC_ERR_INVALID);
    }
    if (groups <= 0 || C % groups) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: %lld channels in %lld groups", nm, (long long)C, (long long)groups);
        return refuse(CGIC_ERR_INVALID);
    }
    // (the kernels index a channel's plane and a span's units with 32 bits)
    if (H > (1 << 20) || W > (1 << 20) || C > (1 << 20) || (C / groups) * H * W >= ((int64_t)1 << 31) || B * groups >= ((int64_t)1 << 31)) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: a group of %lld x %lldx%lld elements is beyond 2^31", nm, (long long)(C / groups), (long long)H,
                 (long long)W);
        return refuse(CGIC_ERR_UNSUPPORTED);
    }
    p->span = (C / groups) * H * W;
    p->spans = B * groups;
    if (p->spans == 0) return CGIC_OK;              // (an empty batch: form 0)
    const bool fits = p->span * norm_dtype_bytes(in_dtype) <= kNormLdsBudget;
    const bool fills = p->spans >= kNormMinSpansOneLaunch;
    p->form = fits && fills ? 1 : 2;
    if (p->form == 1) return CGIC_OK;
    int64_t chunks = p->span / kNormChunkMinElems;
    const int64_t enough = (kNormStatsGridTarget + p->spans - 1) / p->spans;
    if (chunks > enough) chunks = enough;
    if (chunks > kNormMaxChunks) chunks = kNormMaxChunks;
    if (chunks < 1) chunks = 1;
    p->chunks = (int)chunks;
    p->workspace_needed = (size_t)p->spans * (2 * (size_t)chunks + 1) * sizeof(double);     // the pairs, then one K per span
    return CGIC_OK;
}

// the nearest index of one axis (torch's "nearest" at an integer ratio): up-sampling src = dst / (n / nq), sub-sampling
// src = dst * (nq / n); any other ratio is not built
inline bool norm_ratio(int64_t n, int64_t nq, int *mul, int *div)
{
    *mul = *div = 1;
    if (nq <= 0) return false;
    if (n % nq == 0) { *div = (int)(n / nq); return true; }
    if (nq % n == 0 && nq / n < ((int64_t)1 << 20)) { *mul = (int)(nq / n); return true; }
    return false;
}

// the multiplier m = ceil(2^32 / d) with n / d == (n * m) >> 32 for every n <= nmax: exact while nmax * d < 2^32 (the rule of
// cgic_encode_plan.h); 0 where that does not hold or d == 1: the kernel divides
inline unsigned int norm_magic(int64_t nmax, int64_t d)
{
    return (d > 1 && nmax * d < ((int64_t)1 << 32)) ? (unsigned int)((((uint64_t)1 << 32) + (uint64_t)d - 1) / (uint64_t)d) : 0u;
}

// zq's grid hq x wq under features of H x W (both at most 2^20, norm_form): CGIC_OK and the geometry, CGIC_ERR_INVALID for a grid
// that is none, CGIC_ERR_UNSUPPORTED for one too large or not at integer ratios.  The plain call has no zq: hq, wq and the address
// are not looked at, every index ratio stays 1 and only the division by W has a multiplier
inline int norm_zq_geom(int64_t H, int64_t W, int64_t hq, int64_t wq, uintptr_t zq, bool plain, NormZqGeom *q)
{
    *q = NormZqGeom{1, 1, 1, 1, norm_magic(H * W, W), 0u, 0u, false};
    if (plain) return CGIC_OK;
    if (hq <= 0 || wq <= 0) return CGIC_ERR_INVALID;
    if (hq > (1 << 20) || wq > (1 << 20) || hq * wq >= ((int64_t)1 << 31) || !norm_ratio(H, hq, &q->ymul, &q->ydiv) || !norm_ratio(W, wq, &q->xmul, &q->xdiv))
        return CGIC_ERR_UNSUPPORTED;
    q->mg_y = norm_magic(H > hq ? H : hq, q->ydiv);
    q->mg_x = norm_magic(W > wq ? W : wq, q->xdiv);
    q->zq_vec = q->xmul == 1 && q->xdiv == 1 && zq % 16 == 0;
    return CGIC_OK;
}
// the text of such a refusal; -> code
inline int norm_zq_refusal(char (&text)[224], const char *nm, int code, int64_t H, int64_t W, int64_t hq, int64_t wq)
{
    if (code == CGIC_ERR_INVALID)
        snprintf(text, sizeof(text), "%s: zq grid %lldx%lld", nm, (long long)hq, (long long)wq);
    else
        snprintf(text, sizeof(text), "%s: zq %lldx%lld under features %lldx%lld (each axis an integer ratio, up or down)", nm, (long long)hq, (long long)wq,
                 (long long)H, (long long)W);
    return code;
}

// a tensor of a call: `align` is the size of its element.  Address 0 (a tensor the call does not have or want) overlaps nothing
struct NormRegion {
    uintptr_t addr;
    int64_t bytes;
    int align;
};
inline bool norm_regions_overlap(const NormRegion &a, const NormRegion &b)
{
    return a.addr && b.addr && a.addr < b.addr + (uintptr_t)b.bytes && b.addr < a.addr + (uintptr_t)a.bytes;
}

// the inputs that the forward and the backward share, in the order (f, zq, gn_weight, gn_bias, wy, by, wb, bb), to r[0 .. kNormIn);
// zq and the conv parameters of a plain call come out with address 0.  -> none that the call has is NULL
constexpr int kNormIn = 8;
template <class Call>
inline bool norm_inputs(const Call &c, NormRegion *r)
{
    const int ib = norm_dtype_bytes(c.in_dtype);
    const int64_t vec = c.C * 4, mat = c.C * kNormZq * 4, nzq = c.plain ? 0 : c.B * kNormZq * c.hq * c.wq * 4;
    const auto mod = [&](uintptr_t a) { return c.plain ? (uintptr_t)0 : a; };
    const NormRegion all[kNormIn] = {{c.f, c.B * c.C * c.H * c.W * ib, ib}, {mod(c.zq), nzq, 4}, {c.gn_weight, vec, 4}, {c.gn_bias, vec, 4},
                                     {mod(c.wy), mat, 4}, {mod(c.by), vec, 4}, {mod(c.wb), mat, 4}, {mod(c.bb), vec, 4}};
    for (int i = 0; i < kNormIn; ++i) r[i] = all[i];
    return c.f && c.gn_weight && c.gn_bias && (c.plain || (c.zq && c.wy && c.by && c.wb && c.bb));
}

// the unit: 16 bytes of the feature type (the first tensor's) where the row width and the address of every tensor named allow,
// else half of that down to 1.  A thread's elements lie in one row; an access is 16 bytes at most (a fp32 tensor at unit 8 is read
// or written as two), and address 0, a tensor that is not wanted, constrains nothing
inline int norm_unit(int64_t W, std::initializer_list<NormRegion> tensors)
{
    for (int u = 16 / tensors.begin()->align; u > 1; u >>= 1) {
        bool ok = W % u == 0;
        for (const NormRegion &t : tensors) ok = ok && t.addr % (uintptr_t)(u * t.align > 16 ? 16 : u * t.align) == 0;
        if (ok) return u;
    }
    return 1;
}

// CGIC_OK and the plan, or the error code of the call and *why
inline int norm_plan(const NormCall &c, NormPlan *p, const char **why)
{
    const char *nm = norm_name(c.plain);
    int rc = norm_form(nm, c.in_dtype, c.B, c.C, c.H, c.W, c.groups, p, why);
    if (rc != CGIC_OK) return rc;
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    // ---- the type pair: F32 -> F32; F16 | BF16 -> F32 | the same
    if (c.out_dtype != CGIC_DT_F32 && c.out_dtype != c.in_dtype) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: out_dtype %d with in_dtype %d (CGIC_DT_F32 or the features' own type)", nm,
                 c.out_dtype, c.in_dtype);
        return refuse(c.out_dtype == CGIC_DT_F16 || c.out_dtype == CGIC_DT_BF16 ? CGIC_ERR_UNSUPPORTED : CGIC_ERR_INVALID);
    }
    // ---- zq's grid
    rc = norm_zq_geom(c.H, c.W, c.hq, c.wq, c.zq, c.plain, p);
    if (rc != CGIC_OK) return refuse(norm_zq_refusal(p->why_text, nm, rc, c.H, c.W, c.hq, c.wq));
    if (p->form == 0) {                             // (an empty batch: its tensors have no storage, NULL is what arrives; no kernel
        p->mg_w = p->mg_y = p->mg_x = 0u;           // will divide, and no zq is there to be aligned)
        p->zq_vec = false;
        return CGIC_OK;
    }
    // ---- the pointers: the inputs, then out
    const int ob = norm_dtype_bytes(c.out_dtype);
    NormRegion r[kNormIn + 1];
    const bool all = norm_inputs(c, r);
    const NormRegion &out = r[kNormIn] = {c.out, c.B * c.C * c.H * c.W * ob, ob};
    if (!all || !c.out) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: NULL tensor", nm);
        return refuse(CGIC_ERR_INVALID);
    }
    for (int i = 0; i <= kNormIn; ++i)
        if (r[i].addr % (uintptr_t)r[i].align) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: a pointer is not aligned to its %d-byte element", nm, r[i].align);
            return refuse(CGIC_ERR_INVALID);
        }
    // ---- aliasing: out may be f itself when the types are equal (both forms read an element before they write it); no other
    // overlap of out with an input
    p->in_place = c.out == c.f && c.out_dtype == c.in_dtype;
    for (int i = (p->in_place ? 1 : 0); i < kNormIn; ++i)
        if (norm_regions_overlap(out, r[i])) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: out overlaps an input (only out == f with equal types, the in-place form, may)", nm);
            return refuse(CGIC_ERR_INVALID);
        }
    // ---- the workspace of the two-launch form
    if (p->workspace_needed) {
        if (!c.workspace || c.workspace_bytes < p->workspace_needed) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: workspace of %zu bytes, need %zu (cgic_spatial_norm_workspace_bytes)", nm,
                     c.workspace ? c.workspace_bytes : (size_t)0, p->workspace_needed);
            return refuse(CGIC_ERR_CAPACITY);
        }
        if (c.workspace % 8) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: the workspace is not aligned to 8 bytes", nm);
            return refuse(CGIC_ERR_INVALID);
        }
        const NormRegion ws = {c.workspace, (int64_t)p->workspace_needed, 8};
        for (int i = 0; i <= kNormIn; ++i)
            if (norm_regions_overlap(ws, r[i])) {
                snprintf(p->why_text, sizeof(p->why_text), "%s: the workspace overlaps a tensor of the call", nm);
                return refuse(CGIC_ERR_INVALID);
            }
    }
    p->unit = norm_unit(c.W, {r[0], out});
    const int64_t units = p->span / p->unit;        // (W % unit == 0, and the span is whole rows)
    if (p->form == 1) {
        p->grid_one = p->spans;
        const size_t span_bytes = ((size_t)p->span * (size_t)r[0].align + 15) & ~(size_t)15;
        p->lds_bytes = span_bytes + 2 * sizeof(double) * (size_t)(kNormOneThreads / 64);
        return CGIC_OK;
    }
    // ---- two launches: the chunks of the statistics, the parts of the apply
    p->chunk_units = (units + p->chunks - 1) / p->chunks;
    p->grid_stats = p->spans * p->chunks;           // (a chunk that begins behind the span's end writes (0, 0))
    const int64_t plane_units = c.H * c.W / p->unit;
    p->parts = (plane_units + kNormPartUnits - 1) / kNormPartUnits;
    const int64_t items = c.B * c.C * p->parts;
    p->grid_apply = items > kNormApplyGridCap ? kNormApplyGridCap : items;
    return CGIC_OK;
}

}  // namespace cgic

