// cgic_merge.hip -- the mask-weighted three-grain latent merge that sits directly in front of the
// quantiser (reference: CGIC/modules/vqvae/vqvae_blocks.py:361-366):
//     h = up4(h_coarse) * up4(mask0) + up2(h_medium) * up2(mask1) + h_fine * mask2
// (nearest-neighbour upsampling, masks are 0/1 int32 converted to float).  The reference materialises
// four upsampled temporaries; this is one pass: read the three feature maps at their own resolution,
// write h once.  HBM-bound elementwise work; the products and the left-to-right sums are the
// reference's fp32 operations in the reference's order, so the result is bit-identical.
#include "cgic_common.h"

namespace cgic {

__global__ __launch_bounds__(256) void grain_merge_kernel(
    const float *__restrict__ hc, const float *__restrict__ hm, const float *__restrict__ hf,
    const int32_t *__restrict__ mc, const int32_t *__restrict__ mm, const int32_t *__restrict__ mf,
    int64_t B, int C, int64_t h, int64_t w, float *__restrict__ out)
{
    const int64_t w4 = w >> 2, h4 = h >> 2, w2 = w >> 1, h2 = h >> 1, wq = w >> 2;
    const int64_t total = B * C * h * wq;                       // one thread = 4 consecutive x
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xq = t % wq, r = t / wq;
        const int64_t y = r % h, bc = r / h;
        const int64_t b = bc / C;
        const int64_t x = xq << 2;
        const float a = hc[(bc * h4 + (y >> 2)) * w4 + xq];
        const float m0 = (float)mc[(b * h4 + (y >> 2)) * w4 + xq];
        const float2 b2 = *reinterpret_cast<const float2 *>(&hm[(bc * h2 + (y >> 1)) * w2 + (x >> 1)]);
        const int2 m1 = *reinterpret_cast<const int2 *>(&mm[(b * h2 + (y >> 1)) * w2 + (x >> 1)]);
        const float4 c4 = *reinterpret_cast<const float4 *>(&hf[(bc * h + y) * w + x]);
        const int4 m2 = *reinterpret_cast<const int4 *>(&mf[(b * h + y) * w + x]);
        const float am = a * m0;
        const float p0 = b2.x * (float)m1.x, p1 = b2.y * (float)m1.y;
        float4 o;
        o.x = (am + p0) + c4.x * (float)m2.x;
        o.y = (am + p0) + c4.y * (float)m2.y;
        o.z = (am + p1) + c4.z * (float)m2.z;
        o.w = (am + p1) + c4.w * (float)m2.w;
        *reinterpret_cast<float4 *>(&out[(bc * h + y) * w + x]) = o;
    }
}


// ---- decoder side (reference: CGIC/modules/vqvae/decoder.py:304-305,366-378) ---------------------------------
// avgpool_layer1/2 = AvgPool2d(4,4,0) / (2,2,0) on the coarse / medium branch, then inside the up path
//   level -2:  h = h * up2(mask0) + h_medium * mask1                      (medium grid)
//   level -3:  h = h * up4(mask0) + h * up2(mask1) + h_fine * mask2       (fine grid)
// 512 channels at the reference's config: 0.5 GB per tensor at B=64 -- pure HBM streams.  One pass each, float4
// per thread, the reference's products and left-to-right sums (bit-identical; in place is fine: out may alias h).
// The average is the window's row-major running sum divided by the window size, the order of ATen's CPU kernel.

__global__ __launch_bounds__(256) void avgpool_kernel(const float *__restrict__ x, int64_t planes, int64_t H, int64_t W, int k,
                                                      float *__restrict__ out)
{
    const int64_t Ho = H / k, Wo = W / k;
    const int64_t total = planes * Ho * Wo;
    const float div = (float)(k * k);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xo = t % Wo, r = t / Wo;
        const int64_t yo = r % Ho, pl = r / Ho;
        const float *src = x + (pl * H + yo * k) * W + xo * k;
        float sum = 0.f;
        if (k == 4) {
#pragma unroll
            for (int dy = 0; dy < 4; ++dy) {
                const float4 v = *reinterpret_cast<const float4 *>(src + dy * W);     // W % 4 == 0, xo * 4 aligned
                sum += v.x; sum += v.y; sum += v.z; sum += v.w;
            }
        } else {
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
                const float2 v = *reinterpret_cast<const float2 *>(src + dy * W);
                sum += v.x; sum += v.y;
            }
        }
        out[t] = sum / div;
    }
}

// FINE = false: medium grid [B,C,h,w], masks mask0 [B,h/2,w/2], mask1 [B,h,w]
// FINE = true : fine grid   [B,C,h,w], masks mask0 [B,h/4,w/4], mask1 [B,h/2,w/2], mask2 [B,h,w]
template <bool FINE>
__global__ __launch_bounds__(256) void decoder_blend_kernel(
    const float *__restrict__ hin, const float *__restrict__ own, const int32_t *__restrict__ m0,
    const int32_t *__restrict__ m1, const int32_t *__restrict__ m2, int64_t B, int C, int64_t h, int64_t w,
    float *__restrict__ out)
{
    const int64_t wq = w >> 2;
    const int64_t total = B * C * h * wq;                       // one thread = 4 consecutive x
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xq = t % wq, r = t / wq;
        const int64_t y = r % h, bc = r / h;
        const int64_t b = bc / C;
        const int64_t x = xq << 2;
        const float4 hv = *reinterpret_cast<const float4 *>(&hin[(bc * h + y) * w + x]);
        const float4 ov = *reinterpret_cast<const float4 *>(&own[(bc * h + y) * w + x]);
        float4 o;
        if (FINE) {
            const float a = (float)m0[(b * (h >> 2) + (y >> 2)) * (w >> 2) + xq];
            const int2 q1 = *reinterpret_cast<const int2 *>(&m1[(b * (h >> 1) + (y >> 1)) * (w >> 1) + (x >> 1)]);
            const int4 q2 = *reinterpret_cast<const int4 *>(&m2[(b * h + y) * w + x]);
            o.x = (hv.x * a + hv.x * (float)q1.x) + ov.x * (float)q2.x;
            o.y = (hv.y * a + hv.y * (float)q1.x) + ov.y * (float)q2.y;
            o.z = (hv.z * a + hv.z * (float)q1.y) + ov.z * (float)q2.z;
            o.w = (hv.w * a + hv.w * (float)q1.y) + ov.w * (float)q2.w;
        } else {
            const int2 q0 = *reinterpret_cast<const int2 *>(&m0[(b * (h >> 1) + (y >> 1)) * (w >> 1) + (x >> 1)]);
            const int4 q1 = *reinterpret_cast<const int4 *>(&m1[(b * h + y) * w + x]);
            o.x = hv.x * (float)q0.x + ov.x * (float)q1.x;
            o.y = hv.y * (float)q0.x + ov.y * (float)q1.y;
            o.z = hv.z * (float)q0.y + ov.z * (float)q1.z;
            o.w = hv.w * (float)q0.y + ov.w * (float)q1.w;
        }
        *reinterpret_cast<float4 *>(&out[(bc * h + y) * w + x]) = o;
    }
}

// medium blend for widths that are even but not multiples of 4 (a 272-px tile column of the 2K path gives a
// 34-wide medium grid): one thread = 2 consecutive x = one coarse-mask element
__global__ __launch_bounds__(256) void decoder_blend_medium2_kernel(
    const float *__restrict__ hin, const float *__restrict__ own, const int32_t *__restrict__ m0,
    const int32_t *__restrict__ m1, int64_t B, int C, int64_t h, int64_t w, float *__restrict__ out)
{
    const int64_t wh = w >> 1;
    const int64_t total = B * C * h * wh;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t xh = t % wh, r = t / wh;
        const int64_t y = r % h, bc = r / h;
        const int64_t b = bc / C;
        const int64_t x = xh << 1;
        const float2 hv = *reinterpret_cast<const float2 *>(&hin[(bc * h + y) * w + x]);
        const float2 ov = *reinterpret_cast<const float2 *>(&own[(bc * h + y) * w + x]);
        const float q0 = (float)m0[(b * (h >> 1) + (y >> 1)) * wh + xh];
        const int2 q1 = *reinterpret_cast<const int2 *>(&m1[(b * h + y) * w + x]);
        float2 o;
        o.x = hv.x * q0 + ov.x * (float)q1.x;
        o.y = hv.y * q0 + ov.y * (float)q1.y;
        *reinterpret_cast<float2 *>(&out[(bc * h + y) * w + x]) = o;
    }
}

// ---- cgic_cut_tiles: pad + crop of the tiling driver as ONE pass -------------------------------------------------------
// inference_high_resolution.py pads the image to a multiple of 16 (centred zeros, :145-173,:227-228) and crops it tile by
// tile (:236-244).  Here every tile of every image is written straight from the UNPADDED image: a destination element is the
// source pixel it covers, or zero where the tile reaches into the pad.  One thread = 4 consecutive destination pixels of one
// row (tile widths are multiples of 16: 16-byte stores; the source is read element-wise because the centred pad may shift it
// by an odd count).  fp32 [N,3,H,W] -> per tile [N, .., 3, th, tw];  uint8 [N,H,W,3] -> per tile [N, .., th, tw, 3].
constexpr int kCutMaxTiles = 96;
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
constexpr int kPasteMaxTiles = 96;
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
constexpr int kPartitionMaxTiles = 84;
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

}  // namespace cgic

using namespace cgic;

extern "C" int cgic_grain_merge_f32(const float *h_coarse, const float *h_medium, const float *h_fine,
                                    const int32_t *mask_c, const int32_t *mask_m, const int32_t *mask_f, int64_t B,
                                    int C, int64_t h, int64_t w, float *out, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_grain_merge_f32");
    CGIC_REQUIRE(B >= 0 && C > 0 && h > 0 && w > 0 && h % 4 == 0 && w % 4 == 0, CGIC_ERR_INVALID,
                 "grain_merge: fine grid %lldx%lld must be positive multiples of 4", (long long)h, (long long)w);
    const int64_t total = B * C * h * (w >> 2);
    if (total == 0) return CGIC_OK;                   // (an empty batch: its tensors have no storage, NULL is what arrives)
    CGIC_REQUIRE(h_coarse && h_medium && h_fine && mask_c && mask_m && mask_f && out, CGIC_ERR_INVALID, "grain_merge: NULL tensor");
    int nblk = (int)((total + 255) / 256);
    if (nblk > 8192) nblk = 8192;
    hipLaunchKernelGGL(grain_merge_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, h_coarse, h_medium, h_fine,
                       mask_c, mask_m, mask_f, B, C, h, w, out);
    return launch_check("grain_merge_kernel");
}

static int stream_grid(int64_t total)
{
    int64_t nblk = (total + 255) / 256;
    if (nblk > 16384) nblk = 16384;       // 64 workgroups per CU, grid-stride beyond
    return (int)nblk;
}

extern "C" int cgic_avgpool_f32(const float *x, int64_t planes, int64_t H, int64_t W, int k, float *out, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_avgpool_f32");
    CGIC_REQUIRE(k == 2 || k == 4, CGIC_ERR_UNSUPPORTED, "avgpool: window %d; the decoder uses 4 and 2 (decoder.py:304-305)", k);
    CGIC_REQUIRE(planes >= 0 && H > 0 && W > 0 && H % k == 0 && W % k == 0, CGIC_ERR_INVALID,
                 "avgpool: %lldx%lld is not a multiple of the window", (long long)H, (long long)W);
    const int64_t total = planes * (H / k) * (W / k);
    if (total == 0) return CGIC_OK;
    CGIC_REQUIRE(x && out, CGIC_ERR_INVALID, "avgpool: NULL tensor");
    hipLaunchKernelGGL(avgpool_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, x, planes, H, W, k, out);
    return launch_check("avgpool_kernel");
}

extern "C" int cgic_decoder_blend_medium_f32(const float *h, const float *h_medium, const int32_t *mask_c, const int32_t *mask_m,
                                             int64_t B, int C, int64_t hh, int64_t ww, float *out, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_decoder_blend_medium_f32");
    CGIC_REQUIRE(B >= 0 && C > 0 && hh > 0 && ww > 0 && hh % 2 == 0 && ww % 2 == 0, CGIC_ERR_INVALID,
                 "decoder_blend_medium: medium grid %lldx%lld (need even height and width)", (long long)hh, (long long)ww);
    const int64_t total = B * C * hh * (ww % 4 != 0 ? ww >> 1 : ww >> 2);     // one thread = 2 or 4 consecutive x
    if (total == 0) return CGIC_OK;
    CGIC_REQUIRE(h && h_medium && mask_c && mask_m && out, CGIC_ERR_INVALID, "decoder_blend_medium: NULL tensor");
    if (ww % 4 != 0) {
        hipLaunchKernelGGL(decoder_blend_medium2_kernel, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, h, h_medium,
                           mask_c, mask_m, B, C, hh, ww, out);
        return launch_check("decoder_blend_medium2_kernel");
    }
    hipLaunchKernelGGL(decoder_blend_kernel<false>, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, h, h_medium, mask_c,
                       mask_m, (const int32_t *)nullptr, B, C, hh, ww, out);
    return launch_check("decoder_blend_kernel<medium>");
}

extern "C" int cgic_decoder_blend_fine_f32(const float *h, const float *h_fine, const int32_t *mask_c, const int32_t *mask_m,
                                           const int32_t *mask_f, int64_t B, int C, int64_t hh, int64_t ww, float *out,
                                           cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_decoder_blend_fine_f32");
    CGIC_REQUIRE(B >= 0 && C > 0 && hh > 0 && ww > 0 && hh % 4 == 0 && ww % 4 == 0, CGIC_ERR_INVALID,
                 "decoder_blend_fine: fine grid %lldx%lld must be positive multiples of 4", (long long)hh, (long long)ww);
    const int64_t total = B * C * hh * (ww >> 2);
    if (total == 0) return CGIC_OK;
    CGIC_REQUIRE(h && h_fine && mask_c && mask_m && mask_f && out, CGIC_ERR_INVALID, "decoder_blend_fine: NULL tensor");
    hipLaunchKernelGGL(decoder_blend_kernel<true>, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, h, h_fine, mask_c,
                       mask_m, mask_f, B, C, hh, ww, out);
    return launch_check("decoder_blend_kernel<fine>");
}

extern "C" int cgic_cut_tiles(const void *x, int is_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_tile *tiles,
                              cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_cut_tiles");
    CGIC_REQUIRE(x && tiles, CGIC_ERR_INVALID, "cut_tiles: NULL argument");
    CGIC_REQUIRE(N >= 0 && H > 0 && W > 0 && H < (1 << 30) && W < (1 << 30), CGIC_ERR_INVALID, "cut_tiles: bad image shape");
    CGIC_REQUIRE(ntiles >= 1 && ntiles <= kCutMaxTiles, CGIC_ERR_UNSUPPORTED, "cut_tiles: %d tiles (1..%d)", ntiles, kCutMaxTiles);
    CutArgs a;
    a.src = x; a.H = (int)H; a.W = (int)W; a.ntiles = ntiles;
    uint64_t at = 0;
    for (int k = 0; k < ntiles; ++k) {
        const cgic_tile &t = tiles[k];
        CGIC_REQUIRE(t.dst && t.th > 0 && t.tw > 0 && t.tw % 4 == 0, CGIC_ERR_INVALID, "cut_tiles: tile %d: %dx%d (width must be a positive multiple of 4)", k, t.th, t.tw);
        CGIC_REQUIRE(((uintptr_t)t.dst & (is_u8 ? 3u : 15u)) == 0 && (is_u8 ? t.image_stride % 4 == 0 : t.image_stride % 4 == 0), CGIC_ERR_INVALID,
                     "cut_tiles: tile %d: destination not aligned", k);
        // a tile may reach into the pad, never lie wholly outside the image by more than itself
        CGIC_REQUIRE(t.y0 > -(1 << 30) && t.x0 > -(1 << 30) && t.y0 < (1 << 30) && t.x0 < (1 << 30), CGIC_ERR_INVALID, "cut_tiles: tile %d origin", k);
        a.t[k].dst = t.dst; a.t[k].image_stride = t.image_stride; a.t[k].y0 = t.y0; a.t[k].x0 = t.x0; a.t[k].th = t.th; a.t[k].tw = t.tw;
        a.t[k].first = (unsigned int)at;
        at += (uint64_t)(is_u8 ? 1 : 3) * (uint64_t)t.th * (uint64_t)(t.tw / 4);
        CGIC_REQUIRE(at % 64 == 0, CGIC_ERR_UNSUPPORTED, "cut_tiles: tile %d: th * tw / 4 = %lld must be a multiple of 64 (tiles of the x16 grid are)",
                     k, (long long)t.th * (t.tw / 4));
        CGIC_REQUIRE(at < ((uint64_t)1 << 31), CGIC_ERR_UNSUPPORTED, "cut_tiles: image too large");
    }
    for (int k = ntiles; k < kCutMaxTiles; ++k) a.t[k] = a.t[ntiles - 1];
    a.total = (unsigned int)at;
    if (N == 0 || at == 0) return CGIC_OK;
    CGIC_REQUIRE(N <= 65535, CGIC_ERR_UNSUPPORTED, "cut_tiles: more than 65535 images");
    unsigned int nblk = (unsigned int)((at + 255) / 256);          // one item per thread up to 64 workgroups per CU, grid-stride beyond
    if (nblk > 16384) nblk = 16384;
    const dim3 grid(nblk, (unsigned)N);
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
    CGIC_REQUIRE(N >= 0 && H > 0 && W > 0 && H < (1 << 30) && W < (1 << 30), CGIC_ERR_INVALID, "paste_tiles: bad image shape");
    CGIC_REQUIRE(ntiles >= 1 && ntiles <= kPasteMaxTiles, CGIC_ERR_UNSUPPORTED, "paste_tiles: %d tiles (1..%d)", ntiles, kPasteMaxTiles);
    CGIC_REQUIRE(N <= 65535, CGIC_ERR_UNSUPPORTED, "paste_tiles: more than 65535 images");
    PasteArgs a;
    a.out_f32 = out_f32; a.out_u8 = out_u8; a.H = (int)H; a.W = (int)W;
    int64_t clip[kPasteMaxTiles][4];                  // the tile clipped to the image: y0, y1, x0, x1 (empty when y0 >= y1 or x0 >= x1)
    unsigned int most = 0;
    for (int k = 0; k < ntiles; ++k) {
        const cgic_paste_tile &t = tiles[k];
        CGIC_REQUIRE(t.src && t.th > 0 && t.tw > 0 && t.tw % 4 == 0, CGIC_ERR_INVALID,
                     "paste_tiles: tile %d: %dx%d (width must be a positive multiple of 4)", k, t.th, t.tw);
        CGIC_REQUIRE(t.th <= 65535 && t.tw <= 65535, CGIC_ERR_UNSUPPORTED, "paste_tiles: tile %d: %dx%d (at most 65535 a side)", k, t.th, t.tw);
        CGIC_REQUIRE(((uintptr_t)t.src & 15u) == 0 && t.image_stride >= 0 && t.image_stride % 4 == 0, CGIC_ERR_INVALID,
                     "paste_tiles: tile %d: source not 16-byte aligned or image stride not a multiple of 4", k);
        CGIC_REQUIRE(t.image_stride < ((int64_t)1 << 34), CGIC_ERR_UNSUPPORTED, "paste_tiles: tile %d: image stride beyond 2^34", k);
        CGIC_REQUIRE((t.wx != nullptr) == (t.wy != nullptr), CGIC_ERR_INVALID, "paste_tiles: tile %d: wx and wy must both be set or both be NULL", k);
        CGIC_REQUIRE(((uintptr_t)t.wx & 15u) == 0 && ((uintptr_t)t.wy & 7u) == 0, CGIC_ERR_INVALID,
                     "paste_tiles: tile %d: weights not aligned (wx 16 bytes, wy 8)", k);
        CGIC_REQUIRE(t.y0 > -(1 << 30) && t.x0 > -(1 << 30) && t.y0 < (1 << 30) && t.x0 < (1 << 30), CGIC_ERR_INVALID, "paste_tiles: tile %d origin", k);
        clip[k][0] = t.y0 > 0 ? t.y0 : 0; clip[k][1] = (int64_t)t.y0 + t.th < H ? (int64_t)t.y0 + t.th : H;
        clip[k][2] = t.x0 > 0 ? t.x0 : 0; clip[k][3] = (int64_t)t.x0 + t.tw < W ? (int64_t)t.x0 + t.tw : W;
        PasteTile &d = a.t[k];
        d.src = t.src; d.wx = t.wx; d.wy = t.wy; d.stride4 = (unsigned int)(t.image_stride / 4);
        d.y0 = t.y0; d.x0 = t.x0; d.th = (unsigned short)t.th; d.tw = (unsigned short)t.tw;
        const unsigned int items = (unsigned int)t.th * (unsigned int)(t.tw / 4);
        if (items > most) most = items;
    }
    // one tile per pixel: the closed form (and a race-free launch) needs the clipped tiles pairwise disjoint
    for (int k = 0; k < ntiles; ++k) {
        if (clip[k][0] >= clip[k][1] || clip[k][2] >= clip[k][3]) continue;
        for (int j = 0; j < k; ++j) {
            if (clip[j][0] >= clip[j][1] || clip[j][2] >= clip[j][3]) continue;
            const bool apart = clip[k][1] <= clip[j][0] || clip[j][1] <= clip[k][0] || clip[k][3] <= clip[j][2] || clip[j][3] <= clip[k][2];
            CGIC_REQUIRE(apart, CGIC_ERR_UNSUPPORTED, "paste_tiles: tiles %d and %d overlap (the reference's grid never does)", j, k);
        }
    }
    for (int k = ntiles; k < kPasteMaxTiles; ++k) a.t[k] = a.t[ntiles - 1];
    if (N == 0) return CGIC_OK;
    unsigned int nblk = (most + 255) / 256;            // of the largest tile; smaller tiles' surplus workgroups leave at once
    if (nblk > 4096) nblk = 4096;                      // grid-stride beyond
    hipLaunchKernelGGL(paste_tiles_kernel, dim3(nblk, (unsigned)ntiles, (unsigned)N), dim3(256), 0, (hipStream_t)stream, a);
    return launch_check("paste_tiles_kernel");
}

extern "C" int cgic_partition_map(const void *src, int src_u8, int64_t N, int64_t H, int64_t W, int ntiles, const cgic_partition_tile *tiles,
                                  float *out_f32, unsigned char *out_u8, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_partition_map");
    CGIC_REQUIRE(src && tiles, CGIC_ERR_INVALID, "partition_map: NULL argument");
    CGIC_REQUIRE(out_f32 || out_u8, CGIC_ERR_INVALID, "partition_map: no output (out_f32 and out_u8 are both NULL)");
    CGIC_REQUIRE(src_u8 == 0 || src_u8 == 1, CGIC_ERR_INVALID, "partition_map: src_u8 = %d (0 = fp32 [N,3,H,W], 1 = uint8 [N,H,W,3])", src_u8);
    CGIC_REQUIRE((src_u8 || ((uintptr_t)src & 3u) == 0) && ((uintptr_t)out_f32 & 3u) == 0, CGIC_ERR_INVALID, "partition_map: fp32 image not 4-byte aligned");
    CGIC_REQUIRE(N >= 0 && H > 0 && W > 0, CGIC_ERR_INVALID, "partition_map: bad image shape");
    CGIC_REQUIRE(H <= 65535 && W <= 65535, CGIC_ERR_UNSUPPORTED, "partition_map: image %lldx%lld (at most 65535 a side)", (long long)H, (long long)W);
    CGIC_REQUIRE(N <= 65535, CGIC_ERR_UNSUPPORTED, "partition_map: more than 65535 images");
    CGIC_REQUIRE(ntiles >= 1 && ntiles <= kPartitionMaxTiles, CGIC_ERR_UNSUPPORTED, "partition_map: %d tiles (1..%d a launch)", ntiles, kPartitionMaxTiles);
    // an output may BE the source (same address, same layout); any other overlap of two of the three images is a race
    {
        const uintptr_t px = (uintptr_t)N * 3 * (uintptr_t)H * (uintptr_t)W;
        const uintptr_t s0 = (uintptr_t)src, s1 = s0 + px * (src_u8 ? 1 : 4);
        const uintptr_t f0 = (uintptr_t)out_f32, f1 = f0 + px * 4, u0 = (uintptr_t)out_u8, u1 = u0 + px;
        const bool f_is_src = out_f32 && !src_u8 && f0 == s0, u_is_src = out_u8 && src_u8 && u0 == s0;
        CGIC_REQUIRE(!out_f32 || f_is_src || f1 <= s0 || s1 <= f0, CGIC_ERR_INVALID,
                     "partition_map: out_f32 overlaps src without being it (in place = the same address and the same layout)");
        CGIC_REQUIRE(!out_u8 || u_is_src || u1 <= s0 || s1 <= u0, CGIC_ERR_INVALID,
                     "partition_map: out_u8 overlaps src without being it (in place = the same address and the same layout)");
        CGIC_REQUIRE(!out_f32 || !out_u8 || f1 <= u0 || u1 <= f0, CGIC_ERR_INVALID, "partition_map: out_f32 and out_u8 overlap");
    }
    PartArgs a;
    a.src = src; a.out_f32 = out_f32; a.out_u8 = out_u8; a.H = (int)H; a.W = (int)W;
    int64_t clip[kPartitionMaxTiles][4];              // the tile clipped to the image: y0, y1, x0, x1 (empty when y0 >= y1 or x0 >= x1)
    unsigned int most = 0;
    bool masks_form = false;
    for (int k = 0; k < ntiles; ++k) {
        const cgic_partition_tile &t = tiles[k];
        const int nmask = (t.mask_c != nullptr) + (t.mask_m != nullptr) + (t.mask_f != nullptr);
        CGIC_REQUIRE((nmask == 3 && !t.indices) || (nmask == 0 && t.indices), CGIC_ERR_INVALID,
                     "partition_map: tile %d: give the three masks or the indices, exactly one of the two forms", k);
        if (k == 0) masks_form = nmask == 3;
        CGIC_REQUIRE(masks_form == (nmask == 3), CGIC_ERR_INVALID, "partition_map: tile %d: every tile of a call must be in the same form (masks or indices)", k);
        CGIC_REQUIRE(t.th > 0 && t.tw > 0, CGIC_ERR_INVALID, "partition_map: tile %d: %dx%d", k, t.th, t.tw);
        CGIC_REQUIRE(t.th <= 65535 && t.tw <= 65535, CGIC_ERR_UNSUPPORTED, "partition_map: tile %d: %dx%d (at most 65535 a side)", k, t.th, t.tw);
        CGIC_REQUIRE(t.image_stride_tiles >= 0 && t.image_stride_tiles < ((int64_t)1 << 31), CGIC_ERR_INVALID,
                     "partition_map: tile %d: image_stride_tiles %lld", k, (long long)t.image_stride_tiles);
        CGIC_REQUIRE(t.y0 > -(1 << 30) && t.x0 > -(1 << 30) && t.y0 < (1 << 30) && t.x0 < (1 << 30), CGIC_ERR_INVALID, "partition_map: tile %d origin", k);
        int gh = t.gh, gw = t.gw;
        if (masks_form) {
            CGIC_REQUIRE(t.th % 16 == 0 && t.tw % 16 == 0, CGIC_ERR_INVALID,
                         "partition_map: tile %d: %dx%d (the router's masks belong to tiles whose sides are multiples of 16)", k, t.th, t.tw);
            CGIC_REQUIRE((gh == 0 && gw == 0) || (gh == t.th / 4 && gw == t.tw / 4), CGIC_ERR_INVALID,
                         "partition_map: tile %d: index grid %dx%d; the masks' is th/4 x tw/4 (or leave it 0)", k, gh, gw);
            gh = t.th / 4; gw = t.tw / 4;
            CGIC_REQUIRE((((uintptr_t)t.mask_c | (uintptr_t)t.mask_m | (uintptr_t)t.mask_f) & 3u) == 0, CGIC_ERR_INVALID,
                         "partition_map: tile %d: masks not 4-byte aligned", k);
        } else {
            CGIC_REQUIRE(gh >= 1 && gw >= 1, CGIC_ERR_INVALID, "partition_map: tile %d: index grid %dx%d", k, gh, gw);
            CGIC_REQUIRE(gh <= t.th && gw <= t.tw, CGIC_ERR_UNSUPPORTED,
                         "partition_map: tile %d: index grid %dx%d on %dx%d pixels (a cell needs at least one pixel a side)", k, gh, gw, t.th, t.tw);
            CGIC_REQUIRE(((uintptr_t)t.indices & 7u) == 0, CGIC_ERR_INVALID, "partition_map: tile %d: indices not 8-byte aligned", k);
        }
        clip[k][0] = t.y0 > 0 ? t.y0 : 0; clip[k][1] = (int64_t)t.y0 + t.th < H ? (int64_t)t.y0 + t.th : H;
        clip[k][2] = t.x0 > 0 ? t.x0 : 0; clip[k][3] = (int64_t)t.x0 + t.tw < W ? (int64_t)t.x0 + t.tw : W;
        PartTile &d = a.t[k];
        d.a = masks_form ? (const void *)t.mask_c : (const void *)t.indices; d.b = t.mask_m; d.c = t.mask_f;
        d.stride_tiles = (unsigned int)t.image_stride_tiles; d.y0 = t.y0; d.x0 = t.x0;
        d.th = (unsigned short)t.th; d.tw = (unsigned short)t.tw; d.gh = (unsigned short)gh; d.gw = (unsigned short)gw; d.reserved = 0;
        const unsigned int items = (unsigned int)t.th * (unsigned int)((t.tw + 3) / 4);
        if (items > most) most = items;
    }
    // one tile per pixel: a race-free launch (and a defined in-place draw) needs the clipped tiles pairwise disjoint
    for (int k = 0; k < ntiles; ++k) {
        if (clip[k][0] >= clip[k][1] || clip[k][2] >= clip[k][3]) continue;
        for (int j = 0; j < k; ++j) {
            if (clip[j][0] >= clip[j][1] || clip[j][2] >= clip[j][3]) continue;
            const bool apart = clip[k][1] <= clip[j][0] || clip[j][1] <= clip[k][0] || clip[k][3] <= clip[j][2] || clip[j][3] <= clip[k][2];
            CGIC_REQUIRE(apart, CGIC_ERR_UNSUPPORTED, "partition_map: tiles %d and %d overlap (the reference's grid never does)", j, k);
        }
    }
    for (int k = ntiles; k < kPartitionMaxTiles; ++k) a.t[k] = a.t[ntiles - 1];
    if (N == 0) return CGIC_OK;
    unsigned int nblk = (most + 255) / 256;            // of the largest tile; smaller tiles' surplus workgroups leave at once
    if (nblk > 4096) nblk = 4096;                      // grid-stride beyond
    const dim3 grid(nblk, (unsigned)ntiles, (unsigned)N);
    if (masks_form) {
        if (src_u8) hipLaunchKernelGGL((partition_map_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((partition_map_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    } else {
        if (src_u8) hipLaunchKernelGGL((partition_map_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, a);
        else hipLaunchKernelGGL((partition_map_kernel<false, false>), grid, dim3(256), 0, (hipStream_t)stream, a);
    }
    return launch_check("partition_map_kernel");
}
