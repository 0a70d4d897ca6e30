// cgic_attn_bwd_plan.h -- what one call of cgic_attention_backward does, decided before the first launch: every check of the call
// and the geometry of its (up to) three launches.  Plain C++17 on purpose (no HIP include, no stream; pointers are plain addresses):
// attn_bwd_plan() is a pure function of an AttnBwdCall, so all of it can be exercised without a GPU
// (tests/host/attn_bwd_plan_main.cpp).  cgic_attn_bwd.hip fills an AttnBwdCall, calls attn_bwd_plan() once and launches what the
// plan says.
//
// The one form, three launches ordered by the stream:
//   pre    delta[b, i] = sum_c go[c, i] * out[c, i], fp32, into the workspace: one thread per token, kAttnBwdPreThreads per workgroup,
//          grid ceil(N / kAttnBwdPreThreads) * B.  Launched when dq or dk is wanted (dv needs no delta).
//   dq     a workgroup of kAttnThreads threads owns kAttnBQ consecutive queries of one image and walks the keys in tiles of kAttnBK,
//          as the forward does: grid ceil(N / kAttnBQ) * B.  Launched when dq is wanted.  Its LDS holds
//              q and go of the 32 queries, transposed    2 * kAttnBQ rows of (C + pad) elements of the operand type
//              one tile of dS                            kAttnBQ rows of (kAttnBK + pad) elements
//   dkdv   the forward's structure with the roles swapped: a workgroup owns kAttnBwdBK consecutive keys and walks the queries in
//          tiles of kAttnBwdBQT: grid ceil(N / kAttnBwdBK) * B.  Launched when dk or dv is wanted.  Its LDS holds
//              k and v of the 32 keys, transposed        2 * kAttnBwdBK rows of (C + pad) elements
//              one tile, first of P, then of dS          kAttnBwdBK rows of (kAttnBwdBQT + pad) elements
//          One tile, used twice with a barrier between: a tile each for P and dS would put the fp32 kernel at C = 512 at
//          2 * 32 * 513 * 4 + 2 * 32 * 129 * 4 = 164352 bytes, over the 163840 of a compute unit; with one it is 147840.
// The plan computes the LDS bytes of both kernels and refuses a shape whose bytes exceed kAttnBwdLdsLimit instead of launching it
// (no built width does).  pad as in the forward: 8 elements for the half types, 1 for fp32.
// Workspace: delta alone, 4 bytes per token and image, rounded up to 16 bytes -- a function of the shape alone, never assumed zeroed
// (pre writes every element that dq and dkdv read).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "cgic_attn_plan.h"

namespace cgic {

constexpr int kAttnBwdPreThreads = 256;             // tokens per workgroup of the delta launch
constexpr int kAttnBwdBK = 32;                      // keys per workgroup of the dk / dv launch (one MFMA tile)
constexpr int kAttnBwdBQT = 32 * kAttnWaves;        // queries per tile there: one MFMA tile per wave
constexpr size_t kAttnBwdLdsLimit = 160 * 1024;     // LDS of one compute unit of gfx950: what one workgroup may have

struct AttnBwdCall {
    int in_dtype, grad_dtype;       // CGIC_DT_*
    int64_t B, C, N;
    int64_t go_batch_stride, q_batch_stride, k_batch_stride, v_batch_stride;      // elements
    double scale;
    uintptr_t go, q, k, v, out, lse;
    uintptr_t dq, dk, dv;           // each may be 0: not wanted
    uintptr_t workspace;
    size_t workspace_bytes;
};

struct AttnBwdLaunch {
    bool run;
    int threads;
    int64_t tiles;                  // workgroups per image
    int64_t grid;                   // tiles * B
    size_t lds_bytes;
};

struct AttnBwdPlan {
    int form;                       // 1: the launches below; 0: nothing to launch (an empty batch, or no output wanted)
    AttnBwdLaunch pre, dq, dkdv;
    bool dq_vec;                    // dq: a lane reads its 8 keys of a channel of k in one 16-byte access
    bool dkdv_vec;                  // dkdv: ... its 8 queries of a channel of go and of q
    size_t workspace_needed;
    char why_text[224];
};

// the part of the plan that types and shape alone decide: cgic_attention_backward_supported and _workspace_bytes are this
inline int attn_bwd_form(int in_dtype, int grad_dtype, int64_t B, int64_t C, int64_t N, AttnBwdPlan *p, const char **why)
{
    *p = AttnBwdPlan{};
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    if (in_dtype != CGIC_DT_F32 && in_dtype != CGIC_DT_F16 && in_dtype != CGIC_DT_BF16) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: in_dtype %d (CGIC_DT_F32, CGIC_DT_F16 or CGIC_DT_BF16)", in_dtype);
        return refuse(CGIC_ERR_INVALID);
    }
    if (grad_dtype != CGIC_DT_F32 && grad_dtype != in_dtype) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: grad_dtype %d with in_dtype %d (CGIC_DT_F32 or the inputs' own type)", grad_dtype,
                 in_dtype);
        return refuse(grad_dtype == CGIC_DT_F16 || grad_dtype == CGIC_DT_BF16 ? CGIC_ERR_UNSUPPORTED : CGIC_ERR_INVALID);
    }
    if (B < 0 || C <= 0 || N <= 0) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: q, k, v [%lld,%lld,%lld]", (long long)B, (long long)C, (long long)N);
        return refuse(CGIC_ERR_INVALID);
    }
    if (!attn_width_built(C)) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: %lld channels (built for 256 and 512, the model's widths)", (long long)C);
        return refuse(CGIC_ERR_UNSUPPORTED);
    }
    p->pre.threads = kAttnBwdPreThreads; p->dq.threads = kAttnThreads; p->dkdv.threads = kAttnThreads;
    p->pre.tiles = (N + kAttnBwdPreThreads - 1) / kAttnBwdPreThreads;
    p->dq.tiles = (N + kAttnBQ - 1) / kAttnBQ;
    p->dkdv.tiles = (N + kAttnBwdBK - 1) / kAttnBwdBK;
    // (each grid is one dimension of 32 bits; a token index fits 32 bits, every offset built from it is 64-bit)
    if (N >= ((int64_t)1 << 31) || B >= ((int64_t)1 << 31) || p->dq.tiles * B >= ((int64_t)1 << 31) || p->dkdv.tiles * B >= ((int64_t)1 << 31)) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: %lld images of %lld tokens are beyond a grid of 2^31 workgroups", (long long)B,
                 (long long)N);
        return refuse(CGIC_ERR_UNSUPPORTED);
    }
    const int eb = attn_dtype_bytes(in_dtype), pad = attn_pad(in_dtype);
    // (the kernels lay out the same rows from the same constants: attn_pad is tied to the operand types by cgic_attn_dev.h)
    p->pre.lds_bytes = 0;
    p->dq.lds_bytes = (size_t)kAttnBQ * (size_t)(2 * (C + pad) + kAttnBK + pad) * (size_t)eb;
    p->dkdv.lds_bytes = (size_t)kAttnBwdBK * (size_t)(2 * (C + pad) + kAttnBwdBQT + pad) * (size_t)eb;
    if (p->dq.lds_bytes > kAttnBwdLdsLimit || p->dkdv.lds_bytes > kAttnBwdLdsLimit) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: %lld channels need %zu bytes of LDS, a compute unit has %zu", (long long)C,
                 p->dq.lds_bytes > p->dkdv.lds_bytes ? p->dq.lds_bytes : p->dkdv.lds_bytes, kAttnBwdLdsLimit);
        return refuse(CGIC_ERR_UNSUPPORTED);
    }
    p->pre.grid = p->pre.tiles * B; p->dq.grid = p->dq.tiles * B; p->dkdv.grid = p->dkdv.tiles * B;
    p->workspace_needed = ((size_t)B * (size_t)N * sizeof(float) + 15) / 16 * 16;
    if (B == 0) return CGIC_OK;                     // (an empty batch: form 0)
    p->form = 1;
    return CGIC_OK;
}

// CGIC_OK and the plan, or the error code of the call and *why
inline int attn_bwd_plan(const AttnBwdCall &c, AttnBwdPlan *p, const char **why)
{
    const int rc = attn_bwd_form(c.in_dtype, c.grad_dtype, c.B, c.C, c.N, p, why);
    if (rc != CGIC_OK) return rc;
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    if (!(c.scale >= 0.0) || !(c.scale <= 3.0e38)) {       // (as the forward: lse was made with this scale)
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: scale %g (finite, not negative)", c.scale);
        return refuse(CGIC_ERR_INVALID);
    }
    const int64_t image = c.C * c.N;
    if (c.go_batch_stride < image || c.q_batch_stride < image || c.k_batch_stride < image || c.v_batch_stride < image) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: batch strides %lld, %lld, %lld, %lld below C * N = %lld elements",
                 (long long)c.go_batch_stride, (long long)c.q_batch_stride, (long long)c.k_batch_stride, (long long)c.v_batch_stride, (long long)image);
        return refuse(CGIC_ERR_INVALID);
    }
    if (p->form == 0) return CGIC_OK;               // (an empty batch: its tensors have no storage, NULL is what arrives)
    // (the extents below are (B - 1) * stride + C * N elements of at most 4 bytes: a stride beyond this would wrap them, and the
    //  aliasing check would pass on nonsense.  B * C * N itself is below 2^45 by the grid limit)
    const int64_t stride_cap = ((int64_t)1 << 59) / c.B;
    if (c.go_batch_stride > stride_cap || c.q_batch_stride > stride_cap || c.k_batch_stride > stride_cap || c.v_batch_stride > stride_cap) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: batch strides %lld, %lld, %lld, %lld beyond 2^59 / B = %lld elements",
                 (long long)c.go_batch_stride, (long long)c.q_batch_stride, (long long)c.k_batch_stride, (long long)c.v_batch_stride, (long long)stride_cap);
        return refuse(CGIC_ERR_INVALID);
    }
    if (!c.dq && !c.dk && !c.dv) {                  // (no output wanted: nothing to do, and nothing else is looked at)
        p->form = 0;
        return CGIC_OK;
    }
    // ---- the pointers
    if (!c.go || !c.q || !c.k || !c.v || !c.out || !c.lse) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: NULL input");
        return refuse(CGIC_ERR_INVALID);
    }
    const int ib = attn_dtype_bytes(c.in_dtype), gb = attn_dtype_bytes(c.grad_dtype);
    const struct { uintptr_t addr; int eb; } al[9] = {{c.go, ib}, {c.q, ib}, {c.k, ib}, {c.v, ib}, {c.out, ib}, {c.lse, 4}, {c.dq, gb}, {c.dk, gb}, {c.dv, gb}};
    for (int i = 0; i < 9; ++i)
        if (al[i].addr % (uintptr_t)al[i].eb) {
            snprintf(p->why_text, sizeof(p->why_text), "attention_backward: a pointer is not aligned to its %d-byte element", al[i].eb);
            return refuse(CGIC_ERR_INVALID);
        }
    // ---- the workspace
    if (!c.workspace || c.workspace_bytes < p->workspace_needed) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: workspace of %zu bytes, need %zu (cgic_attention_backward_workspace_bytes)",
                 c.workspace ? c.workspace_bytes : (size_t)0, p->workspace_needed);
        return refuse(CGIC_ERR_CAPACITY);
    }
    if (c.workspace % 16) {
        snprintf(p->why_text, sizeof(p->why_text), "attention_backward: workspace is not 16-byte aligned");
        return refuse(CGIC_ERR_INVALID);
    }
    // ---- aliasing: an output overlaps no input, no other output and not the workspace (workgroups read whole images while others store)
    const auto extent = [&](int64_t stride) { return (uintptr_t)(((c.B - 1) * stride + image) * ib); };
    const struct { const char *name; uintptr_t addr, bytes; } in[7] = {
        {"go", c.go, extent(c.go_batch_stride)}, {"q", c.q, extent(c.q_batch_stride)}, {"k", c.k, extent(c.k_batch_stride)},
        {"v", c.v, extent(c.v_batch_stride)},    {"out", c.out, (uintptr_t)(c.B * image * ib)}, {"lse", c.lse, (uintptr_t)(c.B * c.N * 4)},
        {"the workspace", c.workspace, (uintptr_t)p->workspace_needed}};
    const uintptr_t grad_bytes = (uintptr_t)(c.B * image * gb);
    const struct { const char *name; uintptr_t addr; } outs[3] = {{"dq", c.dq}, {"dk", c.dk}, {"dv", c.dv}};
    for (int o = 0; o < 3; ++o) {
        if (!outs[o].addr) continue;
        for (int i = 0; i < 7; ++i)
            if (outs[o].addr < in[i].addr + in[i].bytes && in[i].addr < outs[o].addr + grad_bytes) {
                snprintf(p->why_text, sizeof(p->why_text), "attention_backward: %s overlaps %s", outs[o].name, in[i].name);
                return refuse(CGIC_ERR_INVALID);
            }
        for (int i = 0; i < o; ++i)
            if (outs[i].addr && outs[o].addr < outs[i].addr + grad_bytes && outs[i].addr < outs[o].addr + grad_bytes) {
                snprintf(p->why_text, sizeof(p->why_text), "attention_backward: %s overlaps %s", outs[o].name, outs[i].name);
                return refuse(CGIC_ERR_INVALID);
            }
    }
    // ---- what is launched
    p->pre.run = c.dq != 0 || c.dk != 0;
    p->dq.run = c.dq != 0;
    p->dkdv.run = c.dk != 0 || c.dv != 0;           // (the kernel skips the products of the one whose pointer is NULL)
    // ---- 16-byte loads: a lane's 8 consecutive tokens of one channel are one access only where every row of every image begins
    // 16-byte aligned (the forward's rule for v): dq reads k that way, dkdv reads go and q
    const auto rows16 = [&](uintptr_t addr, int64_t stride) { return ib == 2 && c.N % 8 == 0 && addr % 16 == 0 && stride % 8 == 0; };
    p->dq_vec = rows16(c.k, c.k_batch_stride);
    p->dkdv_vec = rows16(c.go, c.go_batch_stride) && rows16(c.q, c.q_batch_stride);
    return CGIC_OK;
}

}  // namespace cgic
