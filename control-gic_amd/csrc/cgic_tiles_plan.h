// cgic_tiles_plan.h -- what the launches of cgic_cut_tiles / cgic_paste_tiles / cgic_partition_map look like, decided before anything
// is enqueued: every limit of the three descriptor tables, the tile clipped to the image, the pairwise-disjoint rule, the work items
// of a tile and the grid.
// Plain C++17 on purpose (no HIP include, no stream; the device addresses in a descriptor are looked at as numbers, never
// dereferenced): the plans are pure functions of the host arrays, so every limit can be exercised without a GPU
// (tests/host/tiles_plan_main.cpp).  cgic_tiles.hip checks its NULL arguments, calls the plan, turns a refusal into the message of
// the call and issues what the plan says.  The checks run in the order the entry points always had: a call with several faults
// reports the same one.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cgic_hip.h"

namespace cgic {

// descriptors of one launch: they travel as kernel arguments (4 KB)
constexpr int kCutMaxTiles = 96;
constexpr int kPasteMaxTiles = 96;
constexpr int kPartitionMaxTiles = 84;
constexpr int64_t kTilesMaxImages = 65535;      // gridDim.y / .z
constexpr int kTilesMaxSide = 65535;            // extents that travel as unsigned short
constexpr int kTilesReach = 1 << 30;            // image sides below it, tile origins strictly inside +- it
constexpr unsigned int kTilesThreads = 256;     // one thread = one 4-pixel unit of a tile row
constexpr unsigned int kCutMaxBlocks = 16384;   // 64 workgroups per CU; grid-stride beyond
constexpr unsigned int kPasteMaxBlocks = 4096;  // per tile (paste and partition); grid-stride beyond

enum TilesWhy {
    TILES_PLANNED,
    // the three calls
    TILES_IMAGE_SHAPE, TILES_IMAGES, TILES_COUNT, TILES_TILE_SHAPE, TILES_TILE_SIDE, TILES_ORIGIN, TILES_OVERLAP,
    // cut
    CUT_ALIGN, CUT_WAVE, CUT_TOO_LARGE,
    // paste
    PASTE_SOURCE, PASTE_STRIDE, PASTE_WEIGHT_PAIR, PASTE_WEIGHT_ALIGN,
    // partition
    PARTITION_SRC_KIND, PARTITION_IMAGE_ALIGN, PARTITION_IMAGE_SIDE, PARTITION_F32_ON_SRC, PARTITION_U8_ON_SRC, PARTITION_OUTPUTS,
    PARTITION_FORM, PARTITION_MIXED, PARTITION_STRIDE, PARTITION_MASK_SIDES, PARTITION_MASK_GRID, PARTITION_MASK_ALIGN,
    PARTITION_INDEX_GRID, PARTITION_INDEX_CELL, PARTITION_INDEX_ALIGN
};

inline const char *tiles_why_name(TilesWhy w)
{
    static const char *const name[] = {
        "PLANNED", "IMAGE_SHAPE", "IMAGES", "COUNT", "TILE_SHAPE", "TILE_SIDE", "ORIGIN", "OVERLAP", "CUT_ALIGN", "CUT_WAVE", "CUT_TOO_LARGE",
        "PASTE_SOURCE", "PASTE_STRIDE", "PASTE_WEIGHT_PAIR", "PASTE_WEIGHT_ALIGN", "PARTITION_SRC_KIND", "PARTITION_IMAGE_ALIGN",
        "PARTITION_IMAGE_SIDE", "PARTITION_F32_ON_SRC", "PARTITION_U8_ON_SRC", "PARTITION_OUTPUTS", "PARTITION_FORM", "PARTITION_MIXED",
        "PARTITION_STRIDE", "PARTITION_MASK_SIDES", "PARTITION_MASK_GRID", "PARTITION_MASK_ALIGN", "PARTITION_INDEX_GRID", "PARTITION_INDEX_CELL",
        "PARTITION_INDEX_ALIGN"};
    return name[w];
}

// why a plan refused, and where: tile k (tiles j < k for an overlap)
struct TilesFault {
    TilesWhy why;
    int j, k;
};

inline int tiles_refuse(TilesFault *f, int code, TilesWhy why, int k = 0, int j = 0)
{
    f->why = why; f->k = k; f->j = j;
    return code;
}

// ---- what the three calls share --------------------------------------------------------------------------------------------------
inline bool tiles_count_ok(int ntiles, int most) { return ntiles >= 1 && ntiles <= most; }
inline bool tiles_origin_ok(int y0, int x0) { return y0 > -kTilesReach && x0 > -kTilesReach && y0 < kTilesReach && x0 < kTilesReach; }
inline bool tiles_aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// workgroups for `items` 4-pixel units: one unit per thread up to `most` workgroups
inline unsigned int tiles_blocks(uint64_t items, unsigned int most)
{
    const uint64_t b = (items + kTilesThreads - 1) / kTilesThreads;
    return b < most ? (unsigned int)b : most;
}

// the tile clipped to the image; a tile that lies wholly inside the pad is empty
struct TileClip {
    int64_t y0, y1, x0, x1;
    bool empty;
};
inline TileClip tile_clip(int y0, int x0, int th, int tw, int64_t H, int64_t W)
{
    TileClip c;
    c.y0 = y0 > 0 ? y0 : 0; c.y1 = (int64_t)y0 + th < H ? (int64_t)y0 + th : H;
    c.x0 = x0 > 0 ? x0 : 0; c.x1 = (int64_t)x0 + tw < W ? (int64_t)x0 + tw : W;
    c.empty = c.y0 >= c.y1 || c.x0 >= c.x1;
    return c;
}

// one tile per pixel: the closed forms (and a race-free launch) need the clipped tiles pairwise disjoint.  false: *j < *k overlap
inline bool tiles_disjoint(const TileClip *c, int n, int *j, int *k)
{
    for (int b = 0; b < n; ++b) {
        if (c[b].empty) continue;
        for (int a = 0; a < b; ++a) {
            if (c[a].empty) continue;
            const bool apart = c[b].y1 <= c[a].y0 || c[a].y1 <= c[b].y0 || c[b].x1 <= c[a].x0 || c[a].x1 <= c[b].x0;
            if (!apart) { *j = a; *k = b; return false; }
        }
    }
    return true;
}

// ---- cgic_cut_tiles ----------------------------------------------------------------------------------------------------------------
struct CutPlan {
    unsigned int first[kCutMaxTiles];       // first work item of tile k: the running sum of (u8 ? 1 : 3) * th * (tw / 4)
    unsigned int total;                     // work items per image
    unsigned int blocks;                    // grid (blocks, N)
};

// CGIC_OK and the plan, or the error code of the call and *f
inline int cut_plan(int is_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_tile *tiles, CutPlan *p, TilesFault *f)
{
    *p = CutPlan{};
    *f = TilesFault{TILES_PLANNED, 0, 0};
    if (!(N >= 0 && H > 0 && W > 0 && H < kTilesReach && W < kTilesReach)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_IMAGE_SHAPE);
    if (!tiles_count_ok(ntiles, kCutMaxTiles)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_COUNT);
    uint64_t at = 0;
    for (int k = 0; k < ntiles; ++k) {
        const cgic_tile &t = tiles[k];
        if (!(t.dst && t.th > 0 && t.tw > 0 && t.tw % 4 == 0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_TILE_SHAPE, k);
        if (!(tiles_aligned(t.dst, is_u8 ? 4 : 16) && t.image_stride % 4 == 0)) return tiles_refuse(f, CGIC_ERR_INVALID, CUT_ALIGN, k);
        // a tile may reach into the pad, never lie wholly outside the image by more than itself
        if (!tiles_origin_ok(t.y0, t.x0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_ORIGIN, k);
        p->first[k] = (unsigned int)at;
        at += (uint64_t)(is_u8 ? 1 : 3) * (uint64_t)t.th * (uint64_t)(t.tw / 4);
        // the 64 items of a wave share their tile: its search and its descriptor stay on the scalar unit
        if (at % 64 != 0) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, CUT_WAVE, k);
        if (at >= ((uint64_t)1 << 31)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, CUT_TOO_LARGE, k);
    }
    if (N > kTilesMaxImages) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_IMAGES);
    p->total = (unsigned int)at;
    p->blocks = tiles_blocks(at, kCutMaxBlocks);
    return CGIC_OK;
}

// ---- cgic_paste_tiles ------------------------------------------------------------------------------------------------------------
struct PastePlan {
    unsigned int stride4[kPasteMaxTiles];   // image_stride / 4
    unsigned int most;                      // work items th * (tw / 4) of the largest tile
    unsigned int blocks;                    // grid (blocks, ntiles, N): smaller tiles' surplus workgroups leave at once
};

inline int paste_plan(int64_t N, int64_t H, int64_t W, int ntiles, const cgic_paste_tile *tiles, PastePlan *p, TilesFault *f)
{
    *p = PastePlan{};
    *f = TilesFault{TILES_PLANNED, 0, 0};
    if (!(N >= 0 && H > 0 && W > 0 && H < kTilesReach && W < kTilesReach)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_IMAGE_SHAPE);
    if (!tiles_count_ok(ntiles, kPasteMaxTiles)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_COUNT);
    if (N > kTilesMaxImages) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_IMAGES);
    TileClip clip[kPasteMaxTiles];
    for (int k = 0; k < ntiles; ++k) {
        const cgic_paste_tile &t = tiles[k];
        if (!(t.src && t.th > 0 && t.tw > 0 && t.tw % 4 == 0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_TILE_SHAPE, k);
        if (!(t.th <= kTilesMaxSide && t.tw <= kTilesMaxSide)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_TILE_SIDE, k);
        if (!(tiles_aligned(t.src, 16) && t.image_stride >= 0 && t.image_stride % 4 == 0)) return tiles_refuse(f, CGIC_ERR_INVALID, PASTE_SOURCE, k);
        if (!(t.image_stride < ((int64_t)1 << 34))) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, PASTE_STRIDE, k);
        if ((t.wx != nullptr) != (t.wy != nullptr)) return tiles_refuse(f, CGIC_ERR_INVALID, PASTE_WEIGHT_PAIR, k);
        if (!(tiles_aligned(t.wx, 16) && tiles_aligned(t.wy, 8))) return tiles_refuse(f, CGIC_ERR_INVALID, PASTE_WEIGHT_ALIGN, k);
        if (!tiles_origin_ok(t.y0, t.x0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_ORIGIN, k);
        clip[k] = tile_clip(t.y0, t.x0, t.th, t.tw, H, W);
        p->stride4[k] = (unsigned int)(t.image_stride / 4);
        const unsigned int items = (unsigned int)t.th * (unsigned int)(t.tw / 4);
        if (items > p->most) p->most = items;
    }
    int j = 0, k = 0;
    if (!tiles_disjoint(clip, ntiles, &j, &k)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_OVERLAP, k, j);
    p->blocks = tiles_blocks(p->most, kPasteMaxBlocks);
    return CGIC_OK;
}

// ---- cgic_partition_map ------------------------------------------------------------------------------------------------------------
struct PartitionPlan {
    bool masks_form;                        // all tiles: the router's three masks (else: the indices)
    unsigned short gh[kPartitionMaxTiles], gw[kPartitionMaxTiles];      // the index grid of tile k (masks form: th / 4, tw / 4)
    unsigned int most;                      // work items th * ceil(tw / 4) of the largest tile
    unsigned int blocks;                    // grid (blocks, ntiles, N)
};

inline int partition_plan(const void *src, int src_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_partition_tile *tiles,
                          const float *out_f32, const unsigned char *out_u8, PartitionPlan *p, TilesFault *f)
{
    *p = PartitionPlan{};
    *f = TilesFault{TILES_PLANNED, 0, 0};
    if (!(src_u8 == 0 || src_u8 == 1)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_SRC_KIND);
    if (!((src_u8 || tiles_aligned(src, 4)) && tiles_aligned(out_f32, 4))) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_IMAGE_ALIGN);
    if (!(N >= 0 && H > 0 && W > 0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_IMAGE_SHAPE);
    if (!(H <= kTilesMaxSide && W <= kTilesMaxSide)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, PARTITION_IMAGE_SIDE);
    if (N > kTilesMaxImages) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_IMAGES);
    if (!tiles_count_ok(ntiles, kPartitionMaxTiles)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_COUNT);
    // an output may BE the source (same address, same layout); any other overlap of two of the three images is a race
    {
        const uintptr_t px = (uintptr_t)N * 3 * (uintptr_t)H * (uintptr_t)W;
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + px * (src_u8 ? 1 : 4);
        const uintptr_t f0 = (uintptr_t)out_f32, f1 = f0 + px * 4, u0 = (uintptr_t)out_u8, u1 = u0 + px;
        const bool f_is_src = out_f32 && !src_u8 && f0 == s0, u_is_src = out_u8 && src_u8 && u0 == s0;
        if (!(!out_f32 || f_is_src || f1 <= s0 || s1 <= f0)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_F32_ON_SRC);
        if (!(!out_u8 || u_is_src || u1 <= s0 || s1 <= u0)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_U8_ON_SRC);
        if (!(!out_f32 || !out_u8 || f1 <= u0 || u1 <= f0)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_OUTPUTS);
    }
    TileClip clip[kPartitionMaxTiles];
    for (int k = 0; k < ntiles; ++k) {
        const cgic_partition_tile &t = tiles[k];
        const int nmask = (t.mask_c != nullptr) + (t.mask_m != nullptr) + (t.mask_f != nullptr);
        if (!((nmask == 3 && !t.indices) || (nmask == 0 && t.indices))) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_FORM, k);
        if (k == 0) p->masks_form = nmask == 3;
        if (p->masks_form != (nmask == 3)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_MIXED, k);
        if (!(t.th > 0 && t.tw > 0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_TILE_SHAPE, k);
        if (!(t.th <= kTilesMaxSide && t.tw <= kTilesMaxSide)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_TILE_SIDE, k);
        if (!(t.image_stride_tiles >= 0 && t.image_stride_tiles < ((int64_t)1 << 31))) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_STRIDE, k);
        if (!tiles_origin_ok(t.y0, t.x0)) return tiles_refuse(f, CGIC_ERR_INVALID, TILES_ORIGIN, k);
        int gh = t.gh, gw = t.gw;
        if (p->masks_form) {
            if (!(t.th % 16 == 0 && t.tw % 16 == 0)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_MASK_SIDES, k);
            if (!((gh == 0 && gw == 0) || (gh == t.th / 4 && gw == t.tw / 4))) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_MASK_GRID, k);
            gh = t.th / 4; gw = t.tw / 4;
            if (!(tiles_aligned(t.mask_c, 4) && tiles_aligned(t.mask_m, 4) && tiles_aligned(t.mask_f, 4))) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_MASK_ALIGN, k);
        } else {
            if (!(gh >= 1 && gw >= 1)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_INDEX_GRID, k);
            if (!(gh <= t.th && gw <= t.tw)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, PARTITION_INDEX_CELL, k);
            if (!tiles_aligned(t.indices, 8)) return tiles_refuse(f, CGIC_ERR_INVALID, PARTITION_INDEX_ALIGN, k);
        }
        clip[k] = tile_clip(t.y0, t.x0, t.th, t.tw, H, W);
        p->gh[k] = (unsigned short)gh; p->gw[k] = (unsigned short)gw;
        const unsigned int items = (unsigned int)t.th * (unsigned int)((t.tw + 3) / 4);
        if (items > p->most) p->most = items;
    }
    int j = 0, k = 0;
    if (!tiles_disjoint(clip, ntiles, &j, &k)) return tiles_refuse(f, CGIC_ERR_UNSUPPORTED, TILES_OVERLAP, k, j);
    p->blocks = tiles_blocks(p->most, kPasteMaxBlocks);
    return CGIC_OK;
}

}  // namespace cgic
