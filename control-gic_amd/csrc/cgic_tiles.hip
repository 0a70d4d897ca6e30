// cgic_tiles.hip -- the tiled high-resolution path (inference_high_resolution.py) as one launch each: the way in (cgic_cut_tiles: pad +
// crop of every tile of every image), the way out (cgic_paste_tiles: blend + normalise + clamp + unpad, fp32 or uint8 frames) and the
// partition map (cgic_partition_map: the grain grid of every tile).  The descriptors of a launch travel as kernel arguments; what a
// launch looks like -- every limit, the clipped tiles, the grid -- is decided in cgic_tiles_plan.h before anything is enqueued.
#include "cgic_common.h"
#include "cgic_tiles_plan.h"

namespace cgic {

// ---- cgic_cut_tiles: pad + crop of the tiling driver as ONE pass -------------------------------------------------------
// inference_high_resolution.py pads the image to a multiple of 16 (centred zeros, :145-173,:227-228) and crops it tile by
// tile (:236-244).  Here every tile of every image is written straight from the UNPADDED image: a destination element is the
// source pixel it covers, or zero where the tile reaches into the pad.  One thread = 4 consecutive destination pixels of one
// row (tile widths are multiples of 16: 16-byte stores; the source is read element-wise because the centred pad may shift it
// by an odd count).  fp32 [N,3,H,W] -> per tile [N, .., 3, th, tw];  uint8 [N,H,W,3] -> per tile [N, .., th, tw, 3].
struct CutTile {
    void *dst;               // element (image 0, this tile, channel 0 / row 0)
    int64_t image_stride;    // elements between the same tile of consecutive images
    int y0, x0;              // the tile's origin in UNPADDED source coordinates (negative inside the pad)
    int th, tw;
    unsigned int first;      // first work item (4-pixel unit) of this tile
};
struct CutArgs {
    const void *src;
    int H, W, ntiles;
    unsigned int total;      // work items per image
    CutTile t[kCutMaxTiles];
};

template <bool U8>
__global__ __launch_bounds__(256) void cut_tiles_kernel(CutArgs a)
{
    const int64_t n = blockIdx.y;
    const int H = a.H, W = a.W;
    for (unsigned int item = blockIdx.x * 256u + threadIdx.x; item < a.total; item += gridDim.x * 256u) {
        // which tile: every tile's work items are a multiple of 64 (checked on the host; tiles of the x16 grid are), so the 64
        // consecutive items of a wave share their tile: the search and the tile's descriptor stay on the scalar unit
        const unsigned int wbase = __builtin_amdgcn_readfirstlane(item);
        int k = 0;
        while (k + 1 < a.ntiles && wbase >= a.t[k + 1].first) ++k;
        const CutTile &t = a.t[k];
        const unsigned int rel = item - t.first, q = (unsigned int)t.tw >> 2;
        if (U8) {
            const unsigned int r = rel / q, c4 = (rel - r * q) * 4;                 // row, first of 4 columns
            const int sy = t.y0 + (int)r;
            const unsigned char *src = (const unsigned char *)a.src + ((n * H + sy) * (int64_t)W) * 3;
            unsigned int w[3] = {0u, 0u, 0u};
            if (sy >= 0 && sy < H) {
                const int sx = t.x0 + (int)c4;
                if (sx >= 0 && sx + 3 < W && ((((uintptr_t)src) + (unsigned int)sx * 3u) & 3u) == 0) {
                    const unsigned int *p = (const unsigned int *)(src + (int64_t)sx * 3);
                    w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
                } else {
#pragma unroll
                    for (int j = 0; j < 12; ++j) {
                        const int sxj = sx + j / 3;
                        const unsigned int v = (sxj >= 0 && sxj < W) ? src[(int64_t)sxj * 3 + j % 3] : 0u;
                        w[j >> 2] |= v << (8 * (j & 3));
                    }
                }
            }
            unsigned int *dst = (unsigned int *)((unsigned char *)t.dst + n * t.image_stride + ((int64_t)r * t.tw + c4) * 3);
            dst[0] = w[0]; dst[1] = w[1]; dst[2] = w[2];
        } else {
            const unsigned int per_plane = (unsigned int)t.th * q;
            const unsigned int ch = rel / per_plane, rr = rel - ch * per_plane, r = rr / q, c4 = (rr - r * q) * 4;
            const int sy = t.y0 + (int)r;
            const float *src = (const float *)a.src + ((n * 3 + ch) * (int64_t)H + sy) * W;
            float4 v = {0.f, 0.f, 0.f, 0.f};
            if (sy >= 0 && sy < H) {
                const int sx = t.x0 + (int)c4;
                if (sx >= 0 && sx + 3 < W) {
                    if ((((uintptr_t)(src + sx)) & 15u) == 0) v = *reinterpret_cast<const float4 *>(src + sx);
                    else { v.x = src[sx]; v.y = src[sx + 1]; v.z = src[sx + 2]; v.w = src[sx + 3]; }
                } else {
                    if (sx >= 0 && sx < W) v.x = src[sx];
                    if (sx + 1 >= 0 && sx + 1 < W) v.y = src[sx + 1];
                    if (sx + 2 >= 0 && sx + 2 < W) v.z = src[sx + 2];
                    if (sx + 3 >= 0 && sx + 3 < W) v.w = src[sx + 3];
                }
            }
            float *dst = (float *)t.dst + n * t.image_stride + ((int64_t)ch * t.th + r) * t.tw + c4;
            *reinterpret_cast<float4 *>(dst) = v;
        }
    }
}

// ---- cgic_paste_tiles: blend + normalise + clamp + unpad (+ uint8 frames) of the tiling driver as ONE pass ------------------
// inference_high_resolution.py:231-255 accumulates `tile * weights` and the weights into two padded float32 images, divides,
// clamps and slices the pad off; write_images (:103) makes the uint8 frame.  The tiles do not overlap, so per value the loop is
// the closed form of paste_value below (include/cgic_hip.h): the same roundings in the same order, bit-identical to the CPU loop.
// One workgroup column per tile (blockIdx.y: the descriptor is wave-uniform by construction and stays on the scalar unit),
// blockIdx.z = image; one thread = 4 consecutive pixels of one tile row across the three planes: three 16-byte loads, the weight
// product once per pixel for three channels, 16-byte fp32 stores / dword uint8 stores where the unpad shift leaves the output
// address aligned, element-wise otherwise.  No workgroup waits on another, no atomics.  The file is compiled without
// contraction: (double)p * w is a product followed by one conversion.
struct PasteTile {           // 40 bytes: 96 of them and the header stay below 4 KB of kernel arguments
    const float *src;        // element (image 0, this tile, channel 0, row 0)
    const double *wx, *wy;   // [tw], [th] or both NULL
    unsigned int stride4;    // image_stride / 4
    int y0, x0;              // the tile's origin in UNPADDED output coordinates (negative inside the pad)
    unsigned short th, tw;
};
struct PasteArgs {
    float *out_f32;          // [N,3,H,W] or NULL
    unsigned char *out_u8;   // [N,H,W,3] or NULL
    int H, W;
    PasteTile t[kPasteMaxTiles];
};
static_assert(sizeof(PasteTile) == 40 && sizeof(PasteArgs) <= 4096, "paste_tiles: the descriptors travel as kernel arguments");

__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }       // NaN stays NaN

__device__ __forceinline__ float paste_value(float p, double w)
{
    const float acc = (float)((double)p * w);      // rec += tile * wts: float32 += float64 product onto 0
    const float con = (float)w;                    // contrib += wts
    return clamp01(__fdiv_rn(acc, con));
}

__device__ __forceinline__ unsigned int frame_byte(float v)       // (255 * x).astype(uint8) on a clamped value; NaN -> 0
{
    return v == v ? (unsigned int)(255.0f * v) : 0u;
}

__global__ __launch_bounds__(256) void paste_tiles_kernel(PasteArgs a)
{
    const PasteTile &t = a.t[blockIdx.y];
    const int64_t n = blockIdx.z;
    const int H = a.H, W = a.W;
    const unsigned int th = t.th, tw = t.tw, q = tw >> 2, items = th * q;
    const size_t plane = (size_t)th * tw;
    const float *src = t.src + n * ((int64_t)t.stride4 << 2);
    const bool weighted = t.wx != nullptr;
    for (unsigned int item = blockIdx.x * 256u + threadIdx.x; item < items; item += gridDim.x * 256u) {
        const unsigned int r = item / q, c4 = (item - r * q) * 4;
        const int oy = t.y0 + (int)r, ox = t.x0 + (int)c4;
        if (oy < 0 || oy >= H || ox + 3 < 0 || ox >= W) continue;         // the unit lies in the pad: dropped unread
        float v[3][4];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float4 p = *reinterpret_cast<const float4 *>(src + ch * plane + (size_t)r * tw + c4);
            v[ch][0] = p.x; v[ch][1] = p.y; v[ch][2] = p.z; v[ch][3] = p.w;
        }
        if (weighted) {
            const double wyv = t.wy[r];
            const double2 wa = *reinterpret_cast<const double2 *>(t.wx + c4), wb = *reinterpret_cast<const double2 *>(t.wx + c4 + 2);
            const double w[4] = {wyv * wa.x, wyv * wa.y, wyv * wb.x, wyv * wb.y};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[ch][j] = paste_value(v[ch][j], w[j]);
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
#pragma unroll
                for (int j = 0; j < 4; ++j) v[ch][j] = clamp01(v[ch][j]);
        }
        const bool whole = ox >= 0 && ox + 3 < W;
        if (a.out_f32) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float *row = a.out_f32 + ((n * 3 + ch) * (int64_t)H + oy) * W;
                if (whole && (((uintptr_t)(row + ox)) & 15u) == 0) {
                    *reinterpret_cast<float4 *>(row + ox) = make_float4(v[ch][0], v[ch][1], v[ch][2], v[ch][3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (ox + j >= 0 && ox + j < W) row[ox + j] = v[ch][j];
                }
            }
        }
        if (a.out_u8) {
            unsigned char *row = a.out_u8 + (n * (int64_t)H + oy) * W * 3;
            unsigned int b[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) b[j][ch] = frame_byte(v[ch][j]);
            if (whole && (((uintptr_t)(row + (int64_t)ox * 3)) & 3u) == 0) {
                unsigned int *d = reinterpret_cast<unsigned int *>(row + (int64_t)ox * 3);
                d[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
                d[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
                d[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (ox + j >= 0 && ox + j < W) {
                        unsigned char *d = row + (int64_t)(ox + j) * 3;
                        d[0] = (unsigned char)b[j][0]; d[1] = (unsigned char)b[j][1]; d[2] = (unsigned char)b[j][2];
                    }
            }
        }
    }
}

// ---- cgic_partition_map: draw_triple_grain_256res (CGIC/modules/draw.py:78-119) for all tiles of all images as ONE pass -----------
// The reference draws the grain grid with three nested Python loops and two strided slice assignments per cell; per pixel that is a
// select between the source value and the line value, by the closed form in include/cgic_hip.h.  Shaped like paste_tiles_kernel:
// one workgroup column per tile (blockIdx.y: the descriptor is workgroup-uniform and stays on the scalar unit), blockIdx.z = image,
// one thread = 4 consecutive pixels of one tile row across the three channels.  The source is the UNPADDED image itself, so loads
// and stores share their addresses: 16-byte fp32 / dword uint8 accesses where the row length and the unpad shift leave them
// aligned, element accesses otherwise.  A thread reads its pixels before it writes them and no other thread touches them: an
// output may be the source.  No LDS, no atomics, no workgroup waits on another.
struct PartTile {            // 48 bytes: 84 of them and the header stay below 4 KB of kernel arguments
    const void *a, *b, *c;   // masks form: mask_c, mask_m, mask_f (int32) of image 0; indices form: a = indices (int64), b = c = NULL
    unsigned int stride_tiles;
    int y0, x0;              // the tile's origin in UNPADDED image coordinates (negative inside the pad)
    unsigned short th, tw, gh, gw;
    unsigned int reserved;
};
struct PartArgs {
    const void *src;         // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    float *out_f32;          // [N,3,H,W] or NULL
    unsigned char *out_u8;   // [N,H,W,3] or NULL
    int H, W;
    PartTile t[kPartitionMaxTiles];
};
static_assert(sizeof(PartTile) == 48 && sizeof(PartArgs) <= 4096, "partition_map: the descriptors travel as kernel arguments");

template <bool MASKS, bool SRC_U8>
__global__ __launch_bounds__(256) void partition_map_kernel(PartArgs a)
{
    const PartTile &t = a.t[blockIdx.y];
    const int64_t n = blockIdx.z;
    const int H = a.H, W = a.W;
    const unsigned int th = t.th, tw = t.tw, gh = t.gh, gw = t.gw, q = (tw + 3) >> 2, items = th * q;
    const int64_t adv = n * (int64_t)t.stride_tiles;                     // tiles from image 0's to this image's
    const int32_t *mc = nullptr, *mm = nullptr, *mf = nullptr;
    const int64_t *idx = nullptr;
    unsigned int sh = 1, sw = 1;
    if (MASKS) {
        mc = (const int32_t *)t.a + adv * (int64_t)((th >> 4) * (tw >> 4));
        mm = (const int32_t *)t.b + adv * (int64_t)((th >> 3) * (tw >> 3));
        mf = (const int32_t *)t.c + adv * (int64_t)((th >> 2) * (tw >> 2));
    } else {
        idx = (const int64_t *)t.a + adv * (int64_t)(gh * gw);
        sh = th / gh; sw = tw / gw;                                      // >= 1 (checked on the host)
    }
    for (unsigned int item = blockIdx.x * 256u + threadIdx.x; item < items; item += gridDim.x * 256u) {
        const unsigned int r = item / q, c4 = (item - r * q) * 4;
        const int oy = t.y0 + (int)r, ox = t.x0 + (int)c4;
        if (oy < 0 || oy >= H || ox + 3 < 0 || ox >= W) continue;         // the unit lies in the pad: dropped unread
        unsigned int valid = 0;                                           // bit j: pixel c4 + j lies in the tile and in the image
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (ox + j >= 0 && ox + j < W && c4 + j < tw) valid |= 1u << j;
        const bool whole = valid == 15u;
        float v[3][4];                                                    // SRC_U8: unused
        unsigned int b[4][3];                                             // !SRC_U8: filled when the uint8 output is made
        if (SRC_U8) {
            const unsigned char *row = (const unsigned char *)a.src + (n * (int64_t)H + oy) * W * 3;
            if (whole && (((uintptr_t)(row + (int64_t)ox * 3)) & 3u) == 0) {
                const unsigned int *p = reinterpret_cast<const unsigned int *>(row + (int64_t)ox * 3);
                const unsigned int w0 = p[0], w1 = p[1], w2 = p[2];
                b[0][0] = w0 & 255u; b[0][1] = (w0 >> 8) & 255u; b[0][2] = (w0 >> 16) & 255u; b[1][0] = w0 >> 24;
                b[1][1] = w1 & 255u; b[1][2] = (w1 >> 8) & 255u; b[2][0] = (w1 >> 16) & 255u; b[2][1] = w1 >> 24;
                b[2][2] = w2 & 255u; b[3][0] = (w2 >> 8) & 255u; b[3][1] = (w2 >> 16) & 255u; b[3][2] = w2 >> 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) b[j][ch] = (valid >> j & 1u) ? row[(int64_t)(ox + j) * 3 + ch] : 0u;
            }
        } else {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const float *row = (const float *)a.src + ((n * 3 + ch) * (int64_t)H + oy) * W;
                if (whole && (((uintptr_t)(row + ox)) & 15u) == 0) {
                    const float4 p = *reinterpret_cast<const float4 *>(row + ox);
                    v[ch][0] = p.x; v[ch][1] = p.y; v[ch][2] = p.z; v[ch][3] = p.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[ch][j] = (valid >> j & 1u) ? row[ox + j] : 0.f;
                }
            }
        }
        unsigned int line = 0;                                            // bit j: pixel c4 + j is a line pixel
        if (MASKS) {
            // the cell grid is 4 px: the unit is one fine cell; coarse lines every 16 px whatever the masks hold.  The three mask
            // words are loaded unconditionally, next to the pixel loads above: no load waits for a branch on another
            const int cw = mc[(r >> 4) * (tw >> 4) + (c4 >> 4)], mw = mm[(r >> 3) * (tw >> 3) + (c4 >> 3)], fw = mf[(r >> 2) * (tw >> 2) + (c4 >> 2)];
            const unsigned int med = (unsigned int)(cw == 0) & (unsigned int)(mw != 0);          // first maximum: coarse, else medium, else fine
            const unsigned int fin = (unsigned int)(cw == 0) & (unsigned int)(mw == 0) & (unsigned int)(fw != 0);
            const unsigned int row = (unsigned int)((r & 15u) == 0) | (med & (unsigned int)((r & 7u) == 0)) | (fin & (unsigned int)((r & 3u) == 0));
            const unsigned int col = (unsigned int)((c4 & 15u) == 0) | (med & (unsigned int)((c4 & 7u) == 0)) | fin;
            line = row ? 15u : (col ? 1u : 0u);
        } else {
            const unsigned int cy = r / sh;
            const bool ry0 = r - cy * sh == 0;                            // first row of its cell
            unsigned int cx = c4 / sw, rx = c4 - cx * sw;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool rx0 = rx == 0;
                bool l = cy < (gh & ~3u) && cx < (gw & ~3u) && ((ry0 && (cy & 3u) == 0) || (rx0 && (cx & 3u) == 0));
                if (!l && cy < (gh & ~1u) && cx < (gw & ~1u) && ((ry0 && (cy & 1u) == 0) || (rx0 && (cx & 1u) == 0)))
                    l = idx[(size_t)(cy & ~1u) * gw + (cx & ~1u)] == 1;
                if (!l && cy < gh && cx < gw && (ry0 || rx0)) l = idx[(size_t)cy * gw + cx] == 2;
                if (l) line |= 1u << j;
                if (++rx == sw) { rx = 0; ++cx; }
            }
        }
        if (a.out_f32) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float p = SRC_U8 ? __fdiv_rn((float)b[j][ch], 255.0f) : v[ch][j];
                    o[j] = (line >> j & 1u) ? -1.0f : p;
                }
                float *row = a.out_f32 + ((n * 3 + ch) * (int64_t)H + oy) * W;
                if (whole && (((uintptr_t)(row + ox)) & 15u) == 0) {
                    *reinterpret_cast<float4 *>(row + ox) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (valid >> j & 1u) row[ox + j] = o[j];
                }
            }
        }
        if (a.out_u8) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    if (!SRC_U8) b[j][ch] = frame_byte(clamp01(v[ch][j]));
                    if (line >> j & 1u) b[j][ch] = 1u;
                }
            unsigned char *row = a.out_u8 + (n * (int64_t)H + oy) * W * 3;
            if (whole && (((uintptr_t)(row + (int64_t)ox * 3)) & 3u) == 0) {
                unsigned int *d = reinterpret_cast<unsigned int *>(row + (int64_t)ox * 3);
                d[0] = b[0][0] | b[0][1] << 8 | b[0][2] << 16 | b[1][0] << 24;
                d[1] = b[1][1] | b[1][2] << 8 | b[2][0] << 16 | b[2][1] << 24;
                d[2] = b[2][2] | b[3][0] << 8 | b[3][1] << 16 | b[3][2] << 24;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (valid >> j & 1u) {
                        unsigned char *d = row + (int64_t)(ox + j) * 3;
                        d[0] = (unsigned char)b[j][0]; d[1] = (unsigned char)b[j][1]; d[2] = (unsigned char)b[j][2];
                    }
            }
        }
    }
}

// the last tile repeated up to the end of the table (never selected)
template <class T, int M>
static void pad_table(T (&t)[M], int ntiles)
{
    for (int k = ntiles; k < M; ++k) t[k] = t[ntiles - 1];
}

}  // namespace cgic

using namespace cgic;

extern "C" int cgic_cut_tiles(const void *x, int is_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_tile *tiles,
                              cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_cut_tiles");
    CGIC_REQUIRE(x && tiles, CGIC_ERR_INVALID, "cut_tiles: NULL argument");
    CutPlan p;
    TilesFault f;
    const int rc = cut_plan(is_u8, N, H, W, ntiles, tiles, &p, &f);
    const int k = f.k;
    CGIC_REQUIRE(f.why != TILES_IMAGE_SHAPE, rc, "cut_tiles: bad image shape");
    CGIC_REQUIRE(f.why != TILES_COUNT, rc, "cut_tiles: %d tiles (1..%d)", ntiles, kCutMaxTiles);
    CGIC_REQUIRE(f.why != TILES_TILE_SHAPE, rc, "cut_tiles: tile %d: %dx%d (width must be a positive multiple of 4)", k, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != CUT_ALIGN, rc, "cut_tiles: tile %d: destination not aligned", k);
    CGIC_REQUIRE(f.why != TILES_ORIGIN, rc, "cut_tiles: tile %d origin", k);
    CGIC_REQUIRE(f.why != CUT_WAVE, rc, "cut_tiles: tile %d: th * tw / 4 = %lld must be a multiple of 64 (tiles of the x16 grid are)",
                 k, (long long)tiles[k].th * (tiles[k].tw / 4));
    CGIC_REQUIRE(f.why != CUT_TOO_LARGE, rc, "cut_tiles: image too large");
    CGIC_REQUIRE(f.why != TILES_IMAGES, rc, "cut_tiles: more than 65535 images");
    CutArgs a;
    a.src = x; a.H = (int)H; a.W = (int)W; a.ntiles = ntiles; a.total = p.total;
    for (int i = 0; i < ntiles; ++i) {
        const cgic_tile &t = tiles[i];
        a.t[i].dst = t.dst; a.t[i].image_stride = t.image_stride; a.t[i].y0 = t.y0; a.t[i].x0 = t.x0; a.t[i].th = t.th; a.t[i].tw = t.tw;
        a.t[i].first = p.first[i];
    }
    pad_table(a.t, ntiles);
    if (N == 0) return CGIC_OK;
    const dim3 grid(p.blocks, (unsigned)N);
    if (is_u8)
        hipLaunchKernelGGL(cut_tiles_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(cut_tiles_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, a);
    return launch_check("cut_tiles_kernel");
}

extern "C" int cgic_tile_weights_host(int n, int axis, double *out)
{
    CGIC_REQUIRE(out, CGIC_ERR_INVALID, "tile_weights_host: NULL output");
    CGIC_REQUIRE(n >= 1, CGIC_ERR_INVALID, "tile_weights_host: extent %d", n);
    CGIC_REQUIRE(axis == 0 || axis == 1, CGIC_ERR_INVALID, "tile_weights_host: axis %d (0 = x, 1 = y)", axis);
    // _gaussian_weights (:127-143) term by term in the order Python evaluates it; libm's exp, no contraction (Makefile)
    const double var = 0.01;
    const double mid = axis == 0 ? (double)(n - 1) / 2 : (double)n / 2;
    const double nn = (double)((int64_t)n * n);
    const double norm = sqrt(2 * 3.141592653589793 * var);
    for (int x = 0; x < n; ++x) {
        const double d = (double)x - mid;
        out[x] = exp(-d * d / nn / (2 * var)) / norm;
    }
    return CGIC_OK;
}

extern "C" int cgic_paste_tiles(int64_t N, int64_t H, int64_t W, int ntiles, const cgic_paste_tile *tiles, float *out_f32,
                                unsigned char *out_u8, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_paste_tiles");
    CGIC_REQUIRE(tiles, CGIC_ERR_INVALID, "paste_tiles: NULL argument");
    CGIC_REQUIRE(out_f32 || out_u8, CGIC_ERR_INVALID, "paste_tiles: no output (out_f32 and out_u8 are both NULL)");
    CGIC_REQUIRE(((uintptr_t)out_f32 & 3u) == 0, CGIC_ERR_INVALID, "paste_tiles: out_f32 not aligned");
    PastePlan p;
    TilesFault f;
    const int rc = paste_plan(N, H, W, ntiles, tiles, &p, &f);
    const int k = f.k;
    CGIC_REQUIRE(f.why != TILES_IMAGE_SHAPE, rc, "paste_tiles: bad image shape");
    CGIC_REQUIRE(f.why != TILES_COUNT, rc, "paste_tiles: %d tiles (1..%d)", ntiles, kPasteMaxTiles);
    CGIC_REQUIRE(f.why != TILES_IMAGES, rc, "paste_tiles: more than 65535 images");
    CGIC_REQUIRE(f.why != TILES_TILE_SHAPE, rc, "paste_tiles: tile %d: %dx%d (width must be a positive multiple of 4)", k, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != TILES_TILE_SIDE, rc, "paste_tiles: tile %d: %dx%d (at most 65535 a side)", k, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != PASTE_SOURCE, rc, "paste_tiles: tile %d: source not 16-byte aligned or image stride not a multiple of 4", k);
    CGIC_REQUIRE(f.why != PASTE_STRIDE, rc, "paste_tiles: tile %d: image stride beyond 2^34", k);
    CGIC_REQUIRE(f.why != PASTE_WEIGHT_PAIR, rc, "paste_tiles: tile %d: wx and wy must both be set or both be NULL", k);
    CGIC_REQUIRE(f.why != PASTE_WEIGHT_ALIGN, rc, "paste_tiles: tile %d: weights not aligned (wx 16 bytes, wy 8)", k);
    CGIC_REQUIRE(f.why != TILES_ORIGIN, rc, "paste_tiles: tile %d origin", k);
    CGIC_REQUIRE(f.why != TILES_OVERLAP, rc, "paste_tiles: tiles %d and %d overlap (the reference's grid never does)", f.j, k);
    PasteArgs a;
    a.out_f32 = out_f32; a.out_u8 = out_u8; a.H = (int)H; a.W = (int)W;
    for (int i = 0; i < ntiles; ++i) {
        const cgic_paste_tile &t = tiles[i];
        PasteTile &d = a.t[i];
        d.src = t.src; d.wx = t.wx; d.wy = t.wy; d.stride4 = p.stride4[i];
        d.y0 = t.y0; d.x0 = t.x0; d.th = (unsigned short)t.th; d.tw = (unsigned short)t.tw;
    }
    pad_table(a.t, ntiles);
    if (N == 0) return CGIC_OK;
    hipLaunchKernelGGL(paste_tiles_kernel, dim3(p.blocks, (unsigned)ntiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    return launch_check("paste_tiles_kernel");
}

extern "C" int cgic_partition_map(const void *src, int src_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_partition_tile *tiles,
                                  float *out_f32, unsigned char *out_u8, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_partition_map");
    CGIC_REQUIRE(src && tiles, CGIC_ERR_INVALID, "partition_map: NULL argument");
    CGIC_REQUIRE(out_f32 || out_u8, CGIC_ERR_INVALID, "partition_map: no output (out_f32 and out_u8 are both NULL)");
    PartitionPlan p;
    TilesFault f;
    const int rc = partition_plan(src, src_u8, N, H, W, ntiles, tiles, out_f32, out_u8, &p, &f);
    const int k = f.k;
    CGIC_REQUIRE(f.why != PARTITION_SRC_KIND, rc, "partition_map: src_u8 = %d (0 = fp32 [N,3,H,W], 1 = uint8 [N,H,W,3])", src_u8);
    CGIC_REQUIRE(f.why != PARTITION_IMAGE_ALIGN, rc, "partition_map: fp32 image not 4-byte aligned");
    CGIC_REQUIRE(f.why != TILES_IMAGE_SHAPE, rc, "partition_map: bad image shape");
    CGIC_REQUIRE(f.why != PARTITION_IMAGE_SIDE, rc, "partition_map: image %lldx%lld (at most 65535 a side)", (long long)H, (long long)W);
    CGIC_REQUIRE(f.why != TILES_IMAGES, rc, "partition_map: more than 65535 images");
    CGIC_REQUIRE(f.why != TILES_COUNT, rc, "partition_map: %d tiles (1..%d a launch)", ntiles, kPartitionMaxTiles);
    CGIC_REQUIRE(f.why != PARTITION_F32_ON_SRC, rc, "partition_map: out_f32 overlaps src without being it (in place = the same address and the same layout)");
    CGIC_REQUIRE(f.why != PARTITION_U8_ON_SRC, rc, "partition_map: out_u8 overlaps src without being it (in place = the same address and the same layout)");
    CGIC_REQUIRE(f.why != PARTITION_OUTPUTS, rc, "partition_map: out_f32 and out_u8 overlap");
    CGIC_REQUIRE(f.why != PARTITION_FORM, rc, "partition_map: tile %d: give the three masks or the indices, exactly one of the two forms", k);
    CGIC_REQUIRE(f.why != PARTITION_MIXED, rc, "partition_map: tile %d: every tile of a call must be in the same form (masks or indices)", k);
    CGIC_REQUIRE(f.why != TILES_TILE_SHAPE, rc, "partition_map: tile %d: %dx%d", k, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != TILES_TILE_SIDE, rc, "partition_map: tile %d: %dx%d (at most 65535 a side)", k, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != PARTITION_STRIDE, rc, "partition_map: tile %d: image_stride_tiles %lld", k, (long long)tiles[k].image_stride_tiles);
    CGIC_REQUIRE(f.why != TILES_ORIGIN, rc, "partition_map: tile %d origin", k);
    CGIC_REQUIRE(f.why != PARTITION_MASK_SIDES, rc, "partition_map: tile %d: %dx%d (the router's masks belong to tiles whose sides are multiples of 16)",
                 k, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != PARTITION_MASK_GRID, rc, "partition_map: tile %d: index grid %dx%d; the masks' is th/4 x tw/4 (or leave it 0)", k, tiles[k].gh, tiles[k].gw);
    CGIC_REQUIRE(f.why != PARTITION_MASK_ALIGN, rc, "partition_map: tile %d: masks not 4-byte aligned", k);
    CGIC_REQUIRE(f.why != PARTITION_INDEX_GRID, rc, "partition_map: tile %d: index grid %dx%d", k, tiles[k].gh, tiles[k].gw);
    CGIC_REQUIRE(f.why != PARTITION_INDEX_CELL, rc, "partition_map: tile %d: index grid %dx%d on %dx%d pixels (a cell needs at least one pixel a side)",
                 k, tiles[k].gh, tiles[k].gw, tiles[k].th, tiles[k].tw);
    CGIC_REQUIRE(f.why != PARTITION_INDEX_ALIGN, rc, "partition_map: tile %d: indices not 8-byte aligned", k);
    CGIC_REQUIRE(f.why != TILES_OVERLAP, rc, "partition_map: tiles %d and %d overlap (the reference's grid never does)", f.j, k);
    PartArgs a;
    a.src = src; a.out_f32 = out_f32; a.out_u8 = out_u8; a.H = (int)H; a.W = (int)W;
    for (int i = 0; i < ntiles; ++i) {
        const cgic_partition_tile &t = tiles[i];
        PartTile &d = a.t[i];
        d.a = p.masks_form ? (const void *)t.mask_c : (const void *)t.indices; d.b = t.mask_m; d.c = t.mask_f;
        d.stride_tiles = (unsigned int)t.image_stride_tiles; d.y0 = t.y0; d.x0 = t.x0;
        d.th = (unsigned short)t.th; d.tw = (unsigned short)t.tw; d.gh = p.gh[i]; d.gw = p.gw[i]; d.reserved = 0;
    }
    pad_table(a.t, ntiles);
    if (N == 0) return CGIC_OK;
    const dim3 grid(p.blocks, (unsigned)ntiles, (unsigned)N);
    if (p.masks_form) {
        if (src_u8) hipLaunchKernelGGL((partition_map_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((partition_map_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
        if (src_u8) hipLaunchKernelGGL((partition_map_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((partition_map_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    return launch_check("partition_map_kernel");
}
