// cgic_norm_bwd_plan.h -- what one call of cgic_spatial_norm_train / cgic_spatial_norm_backward does, decided before anything is
// enqueued: every check of the call, the unit, the layout of the partial sums in the workspace, the order in which they are added
// and the three grids.  Plain C++17 like cgic_norm_plan.h (no HIP include, pointers are plain addresses): norm_bwd_plan() is a pure
// function of a NormBwdCall (tests/host/norm_bwd_plan_main.cpp); cgic_norm_bwd.hip launches what it says.  The rules that the forward's
// plan has too -- zq's geometry, the unit, the table of the inputs -- are cgic_norm_plan.h's functions.
//
// The backward is three launches ordered by the stream; no workgroup waits for another and nothing is added atomically:
//   reduce   grid (b, channel block, pixel tile).  A tile is `threads_reduce` units of `unit` consecutive pixels of a row; a thread
//            keeps its unit and walks the block's `chan_block` channels.  Per channel the workgroup adds the twelve plane sums
//            (lanes by shuffles, then the waves in wave order) and writes them to sums[b][c][tile][12] (float64); per pixel the
//            thread adds the channels' dz_k in channel order and writes dz[b][block][k][pixel] (fp32).
//   finish   thread (c, j) adds sums[b][c][0..tiles)[j] in tile order, writes gamma_c times the two sums that df needs to
//            span[b][c][2] and adds the images in batch order into parameter gradient j of channel c; a thread per element of
//            dzq adds its ydiv x xdiv pixels of every channel block in (block, row, column) order -- or writes 0 where a
//            sub-sampled axis never reads that element.
//   apply    the forward's apply grid: a workgroup adds span[b][c'][2] over the channels c' of its group in channel order (S1, S2),
//            recomputes gn per element and writes df.
// The channel block and the tile depend on (C, H, W, unit) and never on B, so an image's df and dzq do not depend on its batch.
// The workspace is sized for the smallest unit, by the shape alone; every partial that is read was written by the same call.
// NormBwdCall::plain (value-initialised: false) plans cgic_group_norm_backward: two plane sums per channel (sums[b][c][tile][2]), no
// dz, no dzq threads in finish; zq, conv_y, conv_b and their gradients are not looked at, every other check is the same.
#pragma once
#include "cgic_norm_plan.h"

namespace cgic {

constexpr int kNormBwdSums = 12;                    // sum gn, gn*xhat, gy, gv, four gy*z_k, four gv*z_k
constexpr int kNormBwdThreads = 256;                // a reduce workgroup at most (64 or 128 where a plane has fewer units); finish
constexpr int kNormBwdChanBlock = 32;               // channels a reduce workgroup walks, at most
constexpr int kNormBwdMinChanBlock = 8;             // ... and at least, where the shape is small:
constexpr int64_t kNormBwdBlocksPerImage = 64;      // the block halves while an image has fewer (block, 1024-pixel tile) pairs

struct NormBwdCall {
    int in_dtype, go_dtype, df_dtype;               // CGIC_DT_*
    int64_t B, C, H, W, hq, wq, groups;
    uintptr_t f, go, zq, stats, gn_weight, gn_bias, wy, by, wb, bb;         // the inputs
    uintptr_t df, dzq, dgn_weight, dgn_bias, dwy, dby, dwb, dbb;            // the outputs: 0 = not wanted
    uintptr_t workspace;
    size_t workspace_bytes;
    bool plain;                     // cgic_group_norm_backward: no zq, no conv_y / conv_b, none of their gradients (those fields are not looked at)
};

struct NormBwdPlan : NormZqGeom {      // (the nearest index, as in NormPlan)
    int unit;                       // consecutive pixels of a row per thread and access: 8 (halves only), 4, 2 or 1
    int64_t span, spans;            // elements of a group; B * groups
    int chan_block;                 // channels per reduce workgroup
    int64_t chan_blocks;            // ceil(C / chan_block)
    int threads_reduce;             // 64, 128 or 256
    int64_t tiles, tiles_max;       // pixel tiles of a plane at this unit; at unit 1 (the workspace's size)
    int64_t grid_reduce;            // B * chan_blocks * tiles
    int64_t grid_sums, grid_dzq;    // finish: workgroups of the (c, j) threads, then of the dzq threads (0: dzq not wanted)
    int64_t grid_apply, parts;      // apply: as the forward's; 0: df not wanted
    bool need_dz;                   // dzq is wanted: reduce writes dz, finish folds it
    bool need_conv;                 // a gradient of conv_y / conv_b is wanted: without, reduce adds and writes only sum gn and sum gn * xhat
    bool need_df;                   // df is wanted: finish writes span[b][c][2], apply runs
    bool in_place;                  // df is go
    int sums;                       // plane sums per channel and tile in the workspace: kNormBwdSums, or 2 for the plain call
    size_t off_sums, off_span, off_dz;      // byte offsets into the workspace
    size_t workspace_needed;
    char why_text[224];
};

// the part that the shape alone decides: the checks of (dtype, B, C, H, W, groups) -- the forward's under the forward's name `nm`,
// the others under <nm>_backward --, the channel block and the workspace (cgic_spatial_norm_backward_workspace_bytes is this
// function; with `plain`, cgic_group_norm_backward_workspace_bytes: two sums per channel and tile instead of twelve, no dz partials)
inline int norm_bwd_shape(const char *nm, bool plain, int in_dtype, int64_t B, int64_t C, int64_t H, int64_t W, int64_t groups, NormBwdPlan *p,
                          const char **why)
{
    *p = NormBwdPlan{};
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    NormPlan fwd;
    const char *fwd_why = "";
    const int rc = norm_form(nm, in_dtype, B, C, H, W, groups, &fwd, &fwd_why);
    if (rc != CGIC_OK) {
        snprintf(p->why_text, sizeof(p->why_text), "%s", fwd_why);
        return refuse(rc);
    }
    if (B == 0) {
        snprintf(p->why_text, sizeof(p->why_text), "%s_backward: an empty batch", nm);
        return refuse(CGIC_ERR_INVALID);
    }
    p->span = fwd.span;
    p->spans = fwd.spans;
    const int64_t plane = H * W;
    int cb = kNormBwdChanBlock;
    while (cb > kNormBwdMinChanBlock && ((C + cb - 1) / cb) * ((plane + 1023) / 1024) < kNormBwdBlocksPerImage) cb /= 2;
    p->chan_block = cb;
    p->chan_blocks = (C + cb - 1) / cb;
    p->tiles_max = (plane + kNormBwdThreads - 1) / kNormBwdThreads;
    if (B * p->chan_blocks * p->tiles_max >= ((int64_t)1 << 31) || B * C * kNormBwdSums >= ((int64_t)1 << 31)) {
        snprintf(p->why_text, sizeof(p->why_text), "%s_backward: [%lld,%lld,%lld,%lld] is beyond a grid of 2^31 workgroups", nm, (long long)B,
                 (long long)C, (long long)H, (long long)W);
        return refuse(CGIC_ERR_UNSUPPORTED);
    }
    p->sums = plain ? 2 : kNormBwdSums;
    p->off_sums = 0;
    p->off_span = p->off_sums + (size_t)(B * C * p->tiles_max) * (size_t)p->sums * sizeof(double);
    p->off_dz = p->off_span + (size_t)(B * C) * 2 * sizeof(double);
    p->workspace_needed = p->off_dz + (plain ? (size_t)0 : (size_t)(B * p->chan_blocks) * kNormZq * (size_t)plane * sizeof(float));
    return CGIC_OK;
}

// CGIC_OK and the plan, or the error code of the call and *why
inline int norm_bwd_plan(const NormBwdCall &c, NormBwdPlan *p, const char **why)
{
    int rc = norm_bwd_shape(norm_name(c.plain), c.plain, c.in_dtype, c.B, c.C, c.H, c.W, c.groups, p, why);
    if (rc != CGIC_OK) return rc;
    const char *nm = c.plain ? "group_norm_backward" : "spatial_norm_backward";
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    // ---- the types: go and df are fp32 or the features' own type
    const int both[2] = {c.go_dtype, c.df_dtype};
    for (int i = 0; i < 2; ++i)
        if (both[i] != CGIC_DT_F32 && both[i] != c.in_dtype) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: %s %d with in_dtype %d (CGIC_DT_F32 or the features' own type)", nm,
                     i ? "df_dtype" : "go_dtype", both[i], c.in_dtype);
            return refuse(both[i] == CGIC_DT_F16 || both[i] == CGIC_DT_BF16 ? CGIC_ERR_UNSUPPORTED : CGIC_ERR_INVALID);
        }
    // ---- zq's grid, and dzq's threads in finish
    rc = norm_zq_geom(c.H, c.W, c.hq, c.wq, c.zq, c.plain, p);
    if (rc == CGIC_OK && !c.plain && c.B * kNormZq * c.hq * c.wq >= ((int64_t)1 << 38)) rc = CGIC_ERR_UNSUPPORTED;
    if (rc != CGIC_OK) return refuse(norm_zq_refusal(p->why_text, nm, rc, c.H, c.W, c.hq, c.wq));
    // ---- the pointers: every input, the outputs that are wanted
    const int gb = norm_dtype_bytes(c.go_dtype), db = norm_dtype_bytes(c.df_dtype);
    const int64_t numel = c.B * c.C * c.H * c.W, nzq = c.plain ? 0 : c.B * kNormZq * c.hq * c.wq, vec = c.C * 4, mat = c.C * kNormZq * 4;
    const int kIn = kNormIn + 2, kOut = 8;
    NormRegion in[kNormIn];
    const bool all = norm_inputs(c, in);
    const auto mod = [&](uintptr_t a) { return c.plain ? (uintptr_t)0 : a; };      // (the plain call has no zq and no conv parameters: none of their gradients)
    const NormRegion r[kIn + kOut] = {
        in[0], {c.go, numel * gb, gb}, in[1], {c.stats, p->spans * 8, 4}, in[2], in[3], in[4], in[5], in[6], in[7],
        {c.df, numel * db, db}, {mod(c.dzq), nzq * 4, 4}, {c.dgn_weight, vec, 4}, {c.dgn_bias, vec, 4}, {mod(c.dwy), mat, 4},
        {mod(c.dby), vec, 4}, {mod(c.dwb), mat, 4}, {mod(c.dbb), vec, 4}};
    if (!all || !c.go || !c.stats) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: NULL input", nm);
        return refuse(CGIC_ERR_INVALID);
    }
    bool any = false;
    for (int i = kIn; i < kIn + kOut; ++i) any = any || r[i].addr;
    if (!any) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: no gradient is wanted (every output is NULL)", nm);
        return refuse(CGIC_ERR_INVALID);
    }
    for (int i = 0; i < kIn + kOut; ++i)
        if (r[i].addr % (uintptr_t)r[i].align) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: a pointer is not aligned to its %d-byte element", nm, r[i].align);
            return refuse(CGIC_ERR_INVALID);
        }
    // ---- aliasing: an output overlaps nothing, except that df may be go itself when their types are equal (apply reads a unit of
    // go before it writes that unit of df, and reduce and finish, which also read go, have finished by then)
    p->in_place = c.df && c.df == c.go && c.df_dtype == c.go_dtype;
    for (int o = kIn; o < kIn + kOut; ++o)
        for (int i = 0; i < o; ++i) {
            if (o == kIn && i == 1 && p->in_place) continue;
            if (norm_regions_overlap(r[o], r[i])) {
                snprintf(p->why_text, sizeof(p->why_text), "%s: an output overlaps another tensor of the call (only df == go with equal types may)", nm);
                return refuse(CGIC_ERR_INVALID);
            }
        }
    // ---- the workspace
    if (!c.workspace || c.workspace_bytes < p->workspace_needed) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: workspace of %zu bytes, need %zu (cgic_%s_workspace_bytes)", nm,
                 c.workspace ? c.workspace_bytes : (size_t)0, p->workspace_needed, nm);
        return refuse(CGIC_ERR_CAPACITY);
    }
    if (c.workspace % 16) {                         // (the dz partials are written 16 bytes at a time)
        snprintf(p->why_text, sizeof(p->why_text), "%s: the workspace is not aligned to 16 bytes", nm);
        return refuse(CGIC_ERR_INVALID);
    }
    const NormRegion ws = {c.workspace, (int64_t)p->workspace_needed, 16};
    for (int i = 0; i < kIn + kOut; ++i)
        if (norm_regions_overlap(ws, r[i])) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: the workspace overlaps a tensor of the call", nm);
            return refuse(CGIC_ERR_INVALID);
        }
    p->unit = norm_unit(c.W, {r[0], r[1], r[kIn]});           // f, go and df
    // ---- the grids
    const int64_t plane_units = c.H * c.W / p->unit;
    p->threads_reduce = plane_units <= 64 ? 64 : plane_units <= 128 ? 128 : kNormBwdThreads;
    p->tiles = (plane_units + p->threads_reduce - 1) / p->threads_reduce;       // (<= tiles_max: at most ceil(H * W / 256), or 1)
    p->grid_reduce = c.B * p->chan_blocks * p->tiles;
    p->need_dz = r[kIn + 1].addr != 0;
    p->need_conv = r[kIn + 4].addr || r[kIn + 5].addr || r[kIn + 6].addr || r[kIn + 7].addr;
    p->need_df = c.df != 0;
    p->grid_sums = (c.C * p->sums + kNormBwdThreads - 1) / kNormBwdThreads;
    p->grid_dzq = p->need_dz ? (nzq + kNormBwdThreads - 1) / kNormBwdThreads : 0;
    if (c.df) {
        p->parts = (plane_units + kNormPartUnits - 1) / kNormPartUnits;
        const int64_t items = c.B * c.C * p->parts;
        p->grid_apply = items > kNormApplyGridCap ? kNormApplyGridCap : items;
    }
    return CGIC_OK;
}

// the training forward: the forward's plan, and the statistics it also writes -- fp32 [B * groups][2] = (mean, rstd) -- must be a
// tensor of its own
inline int norm_train_plan(const NormCall &c, uintptr_t stats, NormPlan *p, const char **why)
{
    const int rc = norm_plan(c, p, why);
    if (rc != CGIC_OK || p->form == 0) return rc;
    const char *nm = c.plain ? "group_norm_train" : "spatial_norm_train";
    const auto refuse = [&](int code) { *why = p->why_text; return code; };
    if (!stats || stats % 4) {
        snprintf(p->why_text, sizeof(p->why_text), "%s: stats is %s", nm, stats ? "not aligned to its 4-byte element" : "NULL");
        return refuse(CGIC_ERR_INVALID);
    }
    const int ob = norm_dtype_bytes(c.out_dtype);
    const NormRegion st = {stats, p->spans * 8, 4};
    NormRegion r[kNormIn + 2];
    norm_inputs(c, r);
    r[kNormIn] = {c.out, c.B * c.C * c.H * c.W * ob, ob};
    r[kNormIn + 1] = {p->workspace_needed ? c.workspace : 0, (int64_t)p->workspace_needed, 8};
    for (int i = 0; i < kNormIn + 2; ++i)
        if (norm_regions_overlap(st, r[i])) {
            snprintf(p->why_text, sizeof(p->why_text), "%s: stats overlaps another tensor of the call", nm);
            return refuse(CGIC_ERR_INVALID);
        }
    return CGIC_OK;
}

}  // namespace cgic
