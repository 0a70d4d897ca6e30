// cgic_merge_plan.h -- what one call of the eight merge / pool / blend entry points (cgic_grain_merge, cgic_avgpool,
// cgic_decoder_blend_medium, cgic_decoder_blend_fine, each as _f32 and as _h) does, decided before anything is enqueued.  Plain
// C++17 on purpose (no HIP include, no stream; pointers are plain addresses): merge_plan() is a pure function of a MergeCall, so
// the shape checks, the accepted type pairs, the access width, the aliasing rule and the grid can be exercised without a GPU
// (tests/host/merge_plan_main.cpp).  cgic_merge.hip fills a MergeCall, calls merge_plan() once and launches what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cgic_hip.h"

namespace cgic {

enum MergeOp { MH_MERGE = 0, MH_POOL = 1, MH_BLEND_MEDIUM = 2, MH_BLEND_FINE = 3 };
enum MergeEntry { ME_H = 0, ME_F32 = 1 };       // the family that was called: fp16 / bf16 features, or fp32 in and out

constexpr int kMergeThreads = 256;
constexpr int kMergeGridCap = 8192;             // the merge's cap
constexpr int kStreamGridCap = 16384;           // pools and blends: 64 workgroups per CU, grid-stride beyond

constexpr int dtype_bytes(int dt) { return dt == CGIC_DT_F32 ? 4 : 2; }

// One tensor of a call.  `scale`: fine-grid x per element of a row (1: on the call's grid, 2: at half of it, 4: at a quarter),
// so a thread that takes `unit` consecutive x reads unit / scale elements of it (one at least).
struct MergeTensor {
    uintptr_t addr;
    int elem_bytes;
    int scale;
    int64_t numel;
};

struct MergeCall {
    int op;                     // MergeOp
    int entry;                  // MergeEntry
    int in_dtype, out_dtype;    // CGIC_DT_*
    int64_t B;                  // images; the pool: planes
    int C;                      // channels; the pool: 1
    int64_t h, w;               // the grid of the call; the pool: the INPUT's H, W
    int k;                      // the pool's window
    uintptr_t feat[3];          // merge: coarse, medium, fine; pool: x; blends: h, own
    uintptr_t mask[3];          // merge, fine blend: coarse, medium, fine; medium blend: coarse, medium
    uintptr_t out;
};

struct MergePlan {
    int unit;                   // consecutive x of the call's grid per thread: 8 (halves only), 4, 2 or 1; the pool: input elements
                                // per row and thread (a multiple of k; fp32: k), or 0: one output per thread from element-wise loads
    int threads;                // per workgroup
    int grid;                   // workgroups; 0: nothing to launch (an empty batch)
    int64_t total;              // threads of work: the grid strides over them
    bool in_place;              // out is the blend's h
    int ntensors;
    MergeTensor t[7];       // features, masks, out (last) as the kernel reads them
    char why_text[192];
};

inline const char *merge_name(int op)
{
    return op == MH_MERGE ? "grain_merge" : op == MH_POOL ? "avgpool" : op == MH_BLEND_MEDIUM ? "decoder_blend_medium" : "decoder_blend_fine";
}
inline const char *merge_f32_call(int op)
{
    return op == MH_MERGE ? "cgic_grain_merge_f32" : op == MH_POOL ? "cgic_avgpool_f32"
         : op == MH_BLEND_MEDIUM ? "cgic_decoder_blend_medium_f32" : "cgic_decoder_blend_fine_f32";
}

// bytes a thread moves of tensor t in one access when it takes `unit` x: 16 at most (wider runs are several 16-byte accesses)
inline int merge_access_bytes(const MergeTensor &t, int unit)
{
    int elems = unit / t.scale;
    if (elems < 1) elems = 1;
    const int bytes = elems * t.elem_bytes;
    return bytes > 16 ? 16 : bytes;
}

// CGIC_OK and the plan, or the error code of the call and *why
inline int merge_plan(const MergeCall &c, MergePlan *p, const char **why)
{
    *p = MergePlan{};
    p->threads = kMergeThreads;
    const char *name = merge_name(c.op);
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    // ---- the type pair: (F32, F32) through the _f32 calls, (F16 | BF16, F32 | the same) through the _h calls
    if (c.entry == ME_H && c.in_dtype == CGIC_DT_F32) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: fp32 features are %s's; the _h call takes fp16 or bf16", name, merge_f32_call(c.op));
        return refuse(CGIC_ERR_UNSUPPORTED);
    }
    if (c.entry == ME_F32 ? c.in_dtype != CGIC_DT_F32 : c.in_dtype != CGIC_DT_F16 && c.in_dtype != CGIC_DT_BF16) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: in_dtype %d (%s)", name, c.in_dtype, c.entry == ME_F32 ? "CGIC_DT_F32" : "CGIC_DT_F16 or CGIC_DT_BF16");
        return refuse(CGIC_ERR_INVALID);
    }
    if (c.out_dtype != CGIC_DT_F32 && c.out_dtype != c.in_dtype) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: out_dtype %d with in_dtype %d (CGIC_DT_F32 or the features' own type)", name,
                 c.out_dtype, c.in_dtype);
        return refuse(c.out_dtype == CGIC_DT_F16 || c.out_dtype == CGIC_DT_BF16 ? CGIC_ERR_UNSUPPORTED : CGIC_ERR_INVALID);
    }
    // ---- the shape
    const int64_t B = c.B, h = c.h, w = c.w;
    const int C = c.C, k = c.k;
    bool ok;
    switch (c.op) {
    case MH_POOL:
        if (!(k == 2 || k == 4)) {
            snprintf(p->why_text, sizeof(p->why_text), "avgpool: window %d; the decoder uses 4 and 2 (decoder.py:304-305)", k);
            return refuse(CGIC_ERR_UNSUPPORTED);
        }
        ok = B >= 0 && h > 0 && w > 0 && h % k == 0 && w % k == 0;
        if (!ok) snprintf(p->why_text, sizeof(p->why_text), "avgpool: %lldx%lld is not a multiple of the window", (long long)h, (long long)w);
        break;
    case MH_BLEND_MEDIUM:
        ok = B >= 0 && C > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0;
        if (!ok) snprintf(p->why_text, sizeof(p->why_text), "decoder_blend_medium: medium grid %lldx%lld (need even height and width)",
                          (long long)h, (long long)w);
        break;
    default:
        ok = B >= 0 && C > 0 && h > 0 && w > 0 && h % 4 == 0 && w % 4 == 0;
        if (!ok) snprintf(p->why_text, sizeof(p->why_text), "%s: fine grid %lldx%lld must be positive multiples of 4", name, (long long)h, (long long)w);
        break;
    }
    if (!ok) return refuse(CGIC_ERR_INVALID);
    const int64_t planes = c.op == MH_POOL ? B : B * C;
    if (planes == 0) return CGIC_OK;            // (an empty batch: its tensors have no storage, NULL is what arrives)
    // ---- the tensors as the kernel reads them
    const int ib = dtype_bytes(c.in_dtype), ob = dtype_bytes(c.out_dtype);
    int n = 0;
    const auto add = [&](uintptr_t addr, int elem_bytes, int scale, int64_t numel) { p->t[n++] = MergeTensor{addr, elem_bytes, scale, numel}; };
    switch (c.op) {
    case MH_MERGE:
        add(c.feat[0], ib, 4, planes * (h / 4) * (w / 4)); add(c.feat[1], ib, 2, planes * (h / 2) * (w / 2)); add(c.feat[2], ib, 1, planes * h * w);
        add(c.mask[0], 4, 4, B * (h / 4) * (w / 4)); add(c.mask[1], 4, 2, B * (h / 2) * (w / 2)); add(c.mask[2], 4, 1, B * h * w);
        add(c.out, ob, 1, planes * h * w);
        break;
    case MH_POOL:
        add(c.feat[0], ib, 1, planes * h * w);
        add(c.out, ob, k, planes * (h / k) * (w / k));
        break;
    case MH_BLEND_MEDIUM:
        add(c.feat[0], ib, 1, planes * h * w); add(c.feat[1], ib, 1, planes * h * w);
        add(c.mask[0], 4, 2, B * (h / 2) * (w / 2)); add(c.mask[1], 4, 1, B * h * w);
        add(c.out, ob, 1, planes * h * w);
        break;
    default:
        add(c.feat[0], ib, 1, planes * h * w); add(c.feat[1], ib, 1, planes * h * w);
        add(c.mask[0], 4, 4, B * (h / 4) * (w / 4)); add(c.mask[1], 4, 2, B * (h / 2) * (w / 2)); add(c.mask[2], 4, 1, B * h * w);
        add(c.out, ob, 1, planes * h * w);
        break;
    }
    p->ntensors = n;
    for (int i = 0; i < n; ++i)
        if (!p->t[i].addr) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: NULL tensor", name);
            return refuse(CGIC_ERR_INVALID);
        }
    for (int i = 0; i < n; ++i)
        if (p->t[i].addr % (uintptr_t)p->t[i].elem_bytes) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: a pointer is not aligned to its %d-byte element", name, p->t[i].elem_bytes);
            return refuse(CGIC_ERR_INVALID);
        }
    // ---- aliasing: out may be the blend's h itself when the types are equal; no other overlap of out with an input
    const MergeTensor &o = p->t[n - 1];
    const bool blend = c.op == MH_BLEND_MEDIUM || c.op == MH_BLEND_FINE;
    p->in_place = blend && o.addr == p->t[0].addr && c.out_dtype == c.in_dtype;
    for (int i = (p->in_place ? 1 : 0); i < n - 1; ++i) {
        const MergeTensor &t = p->t[i];
        if (o.addr < t.addr + (uintptr_t)(t.numel * t.elem_bytes) && t.addr < o.addr + (uintptr_t)(o.numel * o.elem_bytes)) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: out overlaps an input (only out == h with equal types, the blends' in-place form, may)", name);
            return refuse(CGIC_ERR_INVALID);
        }
    }
    // ---- the unit: the widest that the row width and every pointer's alignment allow, 16 bytes of the feature type at most (the
    // fp32 pool: one output per thread, so a window's row of k elements)
    const int narrowest = c.op == MH_POOL ? k : 1;
    const int widest = c.op == MH_POOL && ib == 4 ? k : 16 / ib;
    int unit = 0;
    for (int u = widest; u >= narrowest && !unit; u >>= 1) {
        if (w % u) continue;
        bool aligned = true;
        for (int i = 0; i < n; ++i) aligned = aligned && p->t[i].addr % (uintptr_t)merge_access_bytes(p->t[i], u) == 0;
        if (aligned) unit = u;
    }
    // (the pool with a pointer that not even a window's row of k elements may be read from in one access: element by element)
    p->unit = unit;
    p->total = c.op == MH_POOL ? planes * (h / k) * (w / (unit ? unit : k)) : planes * h * (w / unit);
    const int64_t cap = c.op == MH_MERGE ? kMergeGridCap : kStreamGridCap;
    const int64_t nblk = (p->total + kMergeThreads - 1) / kMergeThreads;
    p->grid = (int)(nblk > cap ? cap : nblk);
    return CGIC_OK;
}

// the names of the plan from when it served the _h calls alone; a caller written against them (entry left 0 = ME_H) still builds
using MergeHalfCall = MergeCall;
using MergeHalfPlan = MergePlan;
inline int merge_half_plan(const MergeHalfCall &c, MergeHalfPlan *p, const char **why) { return merge_plan(c, p, why); }

}  // namespace cgic
