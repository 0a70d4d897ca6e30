// cgic_rate_plan.h -- what a call of the rate-control family does, decided before anything is enqueued: every check of
// cgic_rate_curve, cgic_rate_curve_tiles, cgic_route_to_budget and cgic_rate_table (the last one up to its per-candidate routing,
// which router_plan_args plans), the curve launch's grid, threads, LDS bytes and staging, the grids of the launches behind it, and
// the layout of each workspace.  Plain C++17 on purpose (no HIP include, no stream; device pointers are plain addresses):
// curve_plan() and rate_table_plan() are pure functions of a CurveCall / RateTableCall, so all of it can be exercised without a GPU
// (tests/host/rate_plan_main.cpp).  cgic_rate_curve.hip and cgic_rate.hip fill a call, ask for the plan once and issue what it says;
// the four *_workspace_bytes queries are the shape parts (curve_form, rate_table_form).
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cgic_hip.h"
#include "cgic_encode_plan.h"

namespace cgic {

constexpr int kCurveThreads = 1024;
constexpr int64_t kCurveMaxN8 = 12288;               // 8x8 patches of one image (a 768x768 tile has 9216): 12 bytes of LDS each
constexpr size_t kCurveLdsBudget = 152 * 1024;       // dynamic LDS of the workgroup; what the words leave of it stages code lengths
constexpr int kCurveMaxLen = 4095;                   // payload fields: 14 bits medium, 16 bits for the sum of four fine lengths
constexpr int kCurveSummary = 4;                     // int32 per image in the workspace
constexpr int64_t kCurveMaxBatch = 65535;            // one workgroup per image / tile: the grid limit
constexpr int kTilesMaxShapes = 16;
constexpr int kTilesMaxSettings = 65536;
constexpr int kTilesMaxTiles = 65535;
constexpr int kFoldThreads = 256;
constexpr int kPickThreads = 1024;
constexpr int kApplyThreads = 256;
constexpr int kRateMaxCand = 64;
constexpr int kRateThreads = 256;
constexpr int kRateLdsSyms = 16384;                  // code-length tables up to this many symbols are staged in LDS (64 KB)

// every part of a workspace starts on a 256-byte boundary
constexpr size_t rate_slab(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// CGIC_OK never; the refusal's text goes to `text`, its code comes back
template <size_t N>
__attribute__((format(printf, 4, 5))) inline int rate_refuse(char (&text)[N], const char **why, int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, N, fmt, ap);
    va_end(ap);
    *why = text;
    return code;
}

// ===== the three curve entry points ====================================================================================
// They launch the same steps 1-3 under the same limits; what differs between them follows from the entry: the name at the front
// of every message, whether coarse ratio 1 is allowed (the budget route's masks are mode 0 / 1 only), the smallest batch

enum CurveEntry { CURVE_IMAGES, CURVE_TILES, CURVE_BUDGET };     // cgic_rate_curve, cgic_rate_curve_tiles, cgic_route_to_budget

constexpr const char *curve_who(CurveEntry e) { return e == CURVE_IMAGES ? "rate_curve" : e == CURVE_TILES ? "rate_curve_tiles" : "route_to_budget"; }

// what the shape alone decides (no table, no ratio, no pointer): the *_workspace_bytes queries know this much
struct CurveShape {
    CurveEntry entry;
    int64_t B, h16, w16;                // CURVE_IMAGES, CURVE_BUDGET: images, coarse grid of one image
    int64_t R;                          // CURVE_BUDGET: requested ranks
    int64_t T, N, S, M;                 // CURVE_TILES: tiles, images, shape classes, settings
    bool tile_nbytes_given;             // CURVE_TILES: the caller hands in tile_nbytes (else it is part of the workspace)
};

struct CurveCall {
    CurveShape shape;
    bool table;                         // a table was given, of
    int nsym, max_len;                  // cgic_table_num_symbols / cgic_table_max_len (read only when it was)
    double coarse_ratio;
    const int64_t *count;               // CURVE_TILES, host: elements of the five concatenated buffers
    const cgic_rate_tile *tiles;        // CURVE_TILES, host [T]
    // device addresses (0: NULL); each entry point looks at its own
    uintptr_t ind_c, ind_m, ind_f, e16, e8;
    uintptr_t nbytes;                                                   // CURVE_IMAGES
    uintptr_t tiles_dev, image_nbytes;                                  // CURVE_TILES
    uintptr_t ranks_dev;                                                // CURVE_TILES, CURVE_BUDGET
    uintptr_t budget_dev, mask_c, mask_m, mask_f, ind, choice_dev;      // CURVE_BUDGET
    uintptr_t workspace;
};

// the first limit a shape misses, in the order the entry points look (the plan words the message)
enum CurveFault { CURVE_FITS, CURVE_COUNTS, CURVE_BATCH_MIN, CURVE_BATCH_MAX, CURVE_SHAPE, CURVE_SHAPE_LDS, CURVE_RANKS, CURVE_TILES_GRID,
                  CURVE_TILES_SHAPES, CURVE_TILES_SETTINGS };

struct CurvePlan {
    bool nothing_to_do;                 // cgic_rate_curve of an empty batch
    int mode;                           // the curve's router mode: 0, or 1 at coarse ratio 0 (no coarse patch)
    int64_t k_c;                        // coarse rank (CURVE_TILES: every tile's own is checked against its descriptor)
    int64_t n8_max;                     // 8x8 patches of the call's largest image / tile: LDS and threads go by it
    int64_t grid;                       // one workgroup per image / tile; 0: no curve launch (CURVE_TILES with T == 0 still folds)
    int threads;
    size_t lds_bytes;
    bool staged;                        // the code lengths fit the LDS behind the words
    bool lds_opt_in;                    // more than the 64 KB a kernel gets without asking
    size_t workspace_needed;            // (of at least one image / tile: a call that launches no curve still hands one in)
    size_t off_summary, off_total, off_tkey, off_tile_nbytes;   // bytes into the workspace; the last: where tile_nbytes is when not given
    int64_t fold_grid_x, fold_grid_y;   // CURVE_TILES: rate_fold_tiles_kernel, kFoldThreads
    int64_t pick_grid, apply_grid;      // CURVE_BUDGET: rate_pick_kernel (kPickThreads), rate_apply_kernel (kApplyThreads)
    char why_text[512];
};

// one shape: positive, within one workgroup's LDS
inline CurveFault curve_shape_fault(int64_t h16, int64_t w16)
{
    if (!(h16 > 0 && w16 > 0)) return CURVE_SHAPE;
    if (!(h16 <= kCurveMaxN8 && w16 <= kCurveMaxN8 && 4 * h16 * w16 <= kCurveMaxN8)) return CURVE_SHAPE_LDS;
    return CURVE_FITS;
}

// the limits and, for a shape within them, the workspace's layout and the grids behind the curve launch
inline CurveFault curve_form(const CurveShape &s, CurvePlan *p)
{
    *p = CurvePlan{};
    if (s.entry == CURVE_TILES) {
        if (!(s.T >= 0 && s.N >= 1 && s.S >= 1 && s.M >= 1)) return CURVE_COUNTS;
        if (!(s.T <= kTilesMaxTiles && s.N <= kTilesMaxTiles)) return CURVE_TILES_GRID;
        if (!(s.S <= kTilesMaxShapes)) return CURVE_TILES_SHAPES;
        if (!(s.M <= kTilesMaxSettings)) return CURVE_TILES_SETTINGS;
        p->grid = s.T;
    } else {
        if (!(s.B >= (s.entry == CURVE_BUDGET ? 1 : 0))) return CURVE_BATCH_MIN;     // (no image: the budget route has nothing to pick from)
        if (!(s.B <= kCurveMaxBatch)) return CURVE_BATCH_MAX;
        const CurveFault f = curve_shape_fault(s.h16, s.w16);
        if (f != CURVE_FITS) return f;
        p->n8_max = 4 * s.h16 * s.w16;
        if (s.entry == CURVE_BUDGET && !(s.R >= 1 && s.R <= p->n8_max + 1)) return CURVE_RANKS;
        p->grid = s.B;
    }
    // the per-image / per-tile summary in front; a call that launches no curve still hands in the workspace of one image / tile
    const size_t held = (size_t)(p->grid > 0 ? p->grid : 1);
    const size_t summary = rate_slab(held * kCurveSummary * sizeof(int32_t));
    p->workspace_needed = summary;
    if (s.entry == CURVE_TILES) {
        p->off_tile_nbytes = summary;
        if (!s.tile_nbytes_given) p->workspace_needed += held * (size_t)s.M * CGIC_NUM_STREAMS * sizeof(int32_t);
        p->fold_grid_x = (s.M + kFoldThreads - 1) / kFoldThreads;
        p->fold_grid_y = s.N;
    }
    if (s.entry == CURVE_BUDGET) {
        // per image and requested rank the bytes (int32), then the medium threshold's key (uint32)
        const size_t block = rate_slab(held * (size_t)s.R * sizeof(int32_t));
        p->off_total = summary;
        p->off_tkey = summary + block;
        p->workspace_needed = summary + 2 * block;
        p->pick_grid = 1;
        p->apply_grid = (s.B * p->n8_max + kApplyThreads - 1) / kApplyThreads;
        if (p->apply_grid > 65536) p->apply_grid = 65536;
    }
    return CURVE_FITS;
}

// what the size queries answer: the workspace of a shape within the limits that launches a curve, else 0
inline size_t curve_workspace_bytes(const CurveShape &s)
{
    CurvePlan p;
    return curve_form(s, &p) == CURVE_FITS && p.grid > 0 ? p.workspace_needed : 0;
}

// CGIC_OK and the plan, or the error code of the call and *why.  The checks in the order the entry points have always made them: the
// pointers, (tiles: the counts,) the ratio and the table, the shape's limits, (tiles: every descriptor,) the workspace, (budget
// route: the alignments)
inline int curve_plan(const CurveCall &c, CurvePlan *p, const char **why)
{
    const CurveShape &s = c.shape;
    const CurveEntry e = s.entry;
    const char *who = curve_who(e);
    const CurveFault fault = curve_form(s, p);
    char(&text)[sizeof p->why_text] = p->why_text;
    bool given = c.table && c.ind_c && c.ind_m && c.ind_f && c.e16 && c.e8;
    if (e == CURVE_IMAGES) given = given && c.nbytes;
    if (e == CURVE_TILES) given = given && c.count && c.tiles && c.tiles_dev && c.ranks_dev && c.image_nbytes;
    if (e == CURVE_BUDGET) given = given && c.ranks_dev && c.budget_dev && c.mask_c && c.mask_m && c.mask_f && c.ind && c.choice_dev;
    if (!given) return rate_refuse(text, why, CGIC_ERR_INVALID, "%s: NULL argument", who);
    if (fault == CURVE_COUNTS)
        return rate_refuse(text, why, CGIC_ERR_INVALID, "rate_curve_tiles: bad counts (T=%lld, N=%lld, S=%lld, M=%lld)", (long long)s.T, (long long)s.N,
                           (long long)s.S, (long long)s.M);
    // ---- the coarse ratio's range (its top end included or not) and the table
    const bool one_allowed = e != CURVE_BUDGET;             // (coarse ratio 1 leaves the curve's mode)
    if (!(c.coarse_ratio >= 0.0 && (one_allowed ? c.coarse_ratio <= 1.0 : c.coarse_ratio < 1.0)))
        return rate_refuse(text, why, CGIC_ERR_INVALID, "%s: coarse ratio %g outside [0, 1%s", who, c.coarse_ratio,
                           one_allowed ? "]" : "): the curve's mode is 0, or 1 at coarse ratio 0");
    if (!(c.nsym > 0 && c.nsym <= 65536)) return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED, "%s: table of %d symbols", who, c.nsym);
    if (!(c.max_len <= kCurveMaxLen))
        return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED, "%s: codes of up to %d bits (at most %d)", who, c.max_len, kCurveMaxLen);
    // ---- the shape's limits, worded
    const auto shape_refusal = [&](CurveFault f, int64_t tile, int64_t h16, int64_t w16) {
        char item[32];
        if (tile < 0) snprintf(item, sizeof item, "an image");
        else snprintf(item, sizeof item, "tile %lld", (long long)tile);
        if (f == CURVE_SHAPE) return rate_refuse(text, why, CGIC_ERR_INVALID, "%s: %s: bad shape", who, item);
        return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED,
                           "%s: %s of %lld x %lld coarse patches does not fit one workgroup's LDS (at most %lld 8x8 patches: 768x1024 pixels)", who,
                           item, (long long)h16, (long long)w16, (long long)kCurveMaxN8);
    };
    switch (fault) {
    case CURVE_FITS: case CURVE_COUNTS: break;
    case CURVE_BATCH_MIN: return rate_refuse(text, why, CGIC_ERR_INVALID, "%s: bad shape", who);
    case CURVE_BATCH_MAX: return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED, "%s: batch %lld exceeds the grid limit", who, (long long)s.B);
    case CURVE_SHAPE: case CURVE_SHAPE_LDS: return shape_refusal(fault, -1, s.h16, s.w16);
    case CURVE_RANKS:
        return rate_refuse(text, why, CGIC_ERR_INVALID, "route_to_budget: %lld requested ranks (1 .. %lld)", (long long)s.R, (long long)(p->n8_max + 1));
    case CURVE_TILES_GRID:
        return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED, "rate_curve_tiles: %lld tiles of %lld images exceed the grid limit (%d)", (long long)s.T,
                           (long long)s.N, kTilesMaxTiles);
    case CURVE_TILES_SHAPES:
        return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED, "rate_curve_tiles: %lld tile shapes (at most %d)", (long long)s.S, kTilesMaxShapes);
    case CURVE_TILES_SETTINGS:
        return rate_refuse(text, why, CGIC_ERR_UNSUPPORTED, "rate_curve_tiles: %lld settings (at most %d)", (long long)s.M, kTilesMaxSettings);
    }
    // ---- the coarse rank of a shape: the router's, in the curve's mode (the medium ratio plays no part in it).  At coarse ratio 1 the
    // router itself is in mode 4; the curve stays in mode 0 and takes all n16 patches
    p->mode = c.coarse_ratio > 0.0 ? 0 : 1;
    const auto coarse_rank = [&](int64_t n16) {
        double k_c, k_m;
        router_ranks(p->mode, n16, c.coarse_ratio, 0.0, &k_c, &k_m);        // (in range: the ratio is within [0, 1])
        return (int64_t)k_c;
    };
    if (e != CURVE_TILES) p->k_c = coarse_rank(s.h16 * s.w16);
    else {
        for (int i = 0; i < 5; ++i)
            if (!(c.count[i] >= 0)) return rate_refuse(text, why, CGIC_ERR_INVALID, "rate_curve_tiles: negative element count");
        // every descriptor: its shape fits one workgroup, its class has ONE shape, its coarse rank is the one cgic_rate_curve takes,
        // and its five parts lie inside the buffers
        int64_t class_h[kTilesMaxShapes] = {}, class_w[kTilesMaxShapes] = {};
        for (int64_t i = 0; i < s.T; ++i) {
            const cgic_rate_tile &d = c.tiles[i];
            const int64_t h16 = d.h16, w16 = d.w16;
            const CurveFault f = curve_shape_fault(h16, w16);
            if (f != CURVE_FITS) return shape_refusal(f, i, h16, w16);
            const int64_t n16 = h16 * w16, n8 = 4 * n16, k_c = coarse_rank(n16);
            if (!(d.shape >= 0 && d.shape < s.S && d.image >= 0 && d.image < s.N && d.reserved == 0))
                return rate_refuse(text, why, CGIC_ERR_INVALID, "rate_curve_tiles: tile %lld: shape class %d of %lld, image %d of %lld", (long long)i,
                                   d.shape, (long long)s.S, d.image, (long long)s.N);
            if (class_h[d.shape] == 0) { class_h[d.shape] = h16; class_w[d.shape] = w16; }
            if (!(class_h[d.shape] == h16 && class_w[d.shape] == w16))
                return rate_refuse(text, why, CGIC_ERR_INVALID, "rate_curve_tiles: tile %lld: shape class %d holds tiles of two shapes", (long long)i,
                                   d.shape);
            if (!(d.k_c == k_c))
                return rate_refuse(text, why, CGIC_ERR_INVALID, "rate_curve_tiles: tile %lld: k_coarse=%d, the ratio gives %lld of %lld", (long long)i,
                                   d.k_c, (long long)k_c, (long long)n16);
            const int64_t off[5] = {d.off_c, d.off_m, d.off_f, d.off_e16, d.off_e8};
            const int64_t len[5] = {n16, n8, 4 * n8, n16, n8};
            for (int k = 0; k < 5; ++k)
                if (!(off[k] >= 0 && off[k] <= c.count[k] && len[k] <= c.count[k] - off[k]))
                    return rate_refuse(text, why, CGIC_ERR_INVALID,
                                       "rate_curve_tiles: tile %lld: part %d at offset %lld + %lld elements is outside its buffer of %lld", (long long)i,
                                       k, (long long)off[k], (long long)len[k], (long long)c.count[k]);
            if (n8 > p->n8_max) p->n8_max = n8;
        }
    }
    // ---- the workspace
    if (!(p->workspace_needed > 0 && c.workspace))
        return rate_refuse(text, why, CGIC_ERR_INVALID, "%s: workspace of %zu bytes required (cgic_%s_workspace_bytes)", who, p->workspace_needed, who);
    if (!((c.workspace & 15u) == 0)) return rate_refuse(text, why, CGIC_ERR_INVALID, "%s: the workspace must be 16-byte aligned", who);
    if (e == CURVE_BUDGET
        && !(((c.ind_m | c.ind_f | c.mask_m | c.mask_f | c.ind) & 15u) == 0 && (c.e8 & 7u) == 0 && (c.budget_dev & 7u) == 0 && (c.choice_dev & 7u) == 0))
        return rate_refuse(text, why, CGIC_ERR_INVALID,
                           "route_to_budget: ind_m, ind_f, mask_m, mask_f and ind must be 16-byte aligned, e8, the budget and the choice 8-byte aligned");
    p->nothing_to_do = e == CURVE_IMAGES && s.B == 0;      // (an empty batch is not an error here)
    // ---- THE launch plan of steps 1-3: one workgroup per image / tile, LDS and threads by the call's largest
    const size_t words = (size_t)p->n8_max * 12, lens = (size_t)c.nsym * sizeof(int32_t);
    p->staged = words + lens <= kCurveLdsBudget;
    p->lds_bytes = words + (p->staged ? lens : 0);
    p->lds_opt_in = p->lds_bytes > 64 * 1024;
    p->threads = kCurveThreads;                     // one comparator per thread and pass while the image is small; whole waves
    while (p->threads > 256 && p->threads >= p->n8_max) p->threads >>= 1;
    return CGIC_OK;
}

// ===== cgic_rate_table ===================================================================================================
// Its checks up to the workspace, the mask stacks in the workspace and the reduce launch.  What each candidate's routing looks like
// (router_plan_args: it needs device struct sizes) is planned behind this, still before anything is enqueued.

struct RateTableCall {
    bool table;                         // a table was given, of
    int nsym, max_len;                  // cgic_table_num_symbols / cgic_table_max_len (read only when it was)
    int64_t B, h16, w16;
    int C;                              // candidates
    bool inputs;                        // ind_c, ind_m, ind_f, e16, e8, nbytes, coarse and medium are all given
    uintptr_t workspace;
};

struct RateTablePlan {
    bool nothing_to_do;                 // an empty batch
    // one candidate's masks in a stack: [B, h16 w16], [B, 4 h16 w16], [B, 16 h16 w16] int32, each padded to 256 bytes
    int64_t stride_c, stride_m, stride_f;       // int32 elements
    size_t off_c, off_m, off_f;         // bytes into the workspace of the three stacks [C, stride]
    size_t workspace_needed;
    int64_t grid_x, grid_y;             // rate_reduce_kernel: (B, C) workgroups of kRateThreads
    size_t lds_bytes;                   // ... with the code lengths staged when the table is small enough
    char why_text[512];
};

// the part the shape alone decides: cgic_rate_table_workspace_bytes is this
inline int rate_table_form(int64_t B, int64_t h16, int64_t w16, int C, RateTablePlan *p, const char **why)
{
    *p = RateTablePlan{};
    if (!(C >= 1 && C <= kRateMaxCand)) return rate_refuse(p->why_text, why, CGIC_ERR_INVALID, "rate_table: %d candidates (1..%d)", C, kRateMaxCand);
    if (!(B >= 0 && h16 > 0 && w16 > 0)) return rate_refuse(p->why_text, why, CGIC_ERR_INVALID, "rate_table: bad shape");
    if (!(B <= 65535)) return rate_refuse(p->why_text, why, CGIC_ERR_UNSUPPORTED, "rate_table: batch %lld exceeds the grid limit", (long long)B);
    if (B == 0) { p->nothing_to_do = true; return CGIC_OK; }
    if (!(h16 < ((int64_t)1 << 22) && w16 < ((int64_t)1 << 22) && 16 * h16 * w16 < ((int64_t)1 << 26)))       // (no product before its factors are known small)
        return rate_refuse(p->why_text, why, CGIC_ERR_UNSUPPORTED, "rate_table: latent grid too large");
    const int64_t n16 = h16 * w16;
    const auto elems = [](int64_t n) { return (int64_t)(rate_slab((size_t)n * sizeof(int32_t)) / sizeof(int32_t)); };
    p->stride_c = elems(B * n16); p->stride_m = elems(4 * B * n16); p->stride_f = elems(16 * B * n16);
    p->off_c = 0;
    p->off_m = (size_t)C * (size_t)p->stride_c * sizeof(int32_t);
    p->off_f = p->off_m + (size_t)C * (size_t)p->stride_m * sizeof(int32_t);
    p->workspace_needed = p->off_f + (size_t)C * (size_t)p->stride_f * sizeof(int32_t);
    p->grid_x = B; p->grid_y = C;
    return CGIC_OK;
}

// CGIC_OK and the plan, or the error code of the call and *why
inline int rate_table_plan(const RateTableCall &c, RateTablePlan *p, const char **why)
{
    *p = RateTablePlan{};
    if (!(c.table && c.inputs)) return rate_refuse(p->why_text, why, CGIC_ERR_INVALID, "rate_table: NULL argument");
    const int rc = rate_table_form(c.B, c.h16, c.w16, c.C, p, why);
    if (rc != CGIC_OK || p->nothing_to_do) return rc;
    if (!(c.nsym > 0 && c.nsym <= 65536)) return rate_refuse(p->why_text, why, CGIC_ERR_UNSUPPORTED, "rate_table: table of %d symbols", c.nsym);
    if (!((uint64_t)c.max_len * (uint64_t)(16 * c.h16 * c.w16) < 0xFFFFFF00ull))
        return rate_refuse(p->why_text, why, CGIC_ERR_UNSUPPORTED, "rate_table: a stream could exceed 2^32 bits");
    if (!c.workspace)
        return rate_refuse(p->why_text, why, CGIC_ERR_INVALID, "rate_table: workspace of %zu bytes required (cgic_rate_table_workspace_bytes)",
                           p->workspace_needed);
    if (!((c.workspace & 15u) == 0)) return rate_refuse(p->why_text, why, CGIC_ERR_INVALID, "rate_table: the workspace must be 16-byte aligned");
    p->lds_bytes = c.nsym <= kRateLdsSyms ? (size_t)c.nsym * sizeof(int32_t) : 0;
    return CGIC_OK;
}

}  // namespace cgic
