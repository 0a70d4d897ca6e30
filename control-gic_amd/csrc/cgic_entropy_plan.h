// cgic_entropy_plan.h -- the argument checks and the launch geometry the entropy-map entry points share (cgic_entropy_maps_f32 / _u8,
// cgic_entropy_maps_tiles, cgic_entropy_maps_ref_f32), decided before anything is enqueued.  Plain C++17 on purpose (no HIP include,
// no stream, no device pointer: `bins` is the caller's host array), so every check and every grid can be exercised without a GPU
// (tests/host/entropy_plan_main.cpp).  cgic_entropy.hip calls the checks in the order of its entry points, plans, then issues.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cgic_hip.h"

namespace cgic {

constexpr int kBins = 32;
constexpr int kEntThreads = 256;
constexpr int kEntWaves = kEntThreads / 64;      // wavefronts of a workgroup
constexpr int kEntTilesPpw = 4;      // patches a wave walks in the windowed (tiles) form
constexpr int kEntMaxTiles = 48;     // tiles per image of one shape group (EntWindow::org travels in the kernarg segment)
constexpr int64_t kEntMaxGrid = 65535;      // gridDim.y / .z

// a refusal: the call's error code and its message
struct EntropyWhy { char text[160]; };
#define CGIC_ENT_REFUSE(code, ...) do { snprintf(why->text, sizeof(why->text), __VA_ARGS__); return (code); } while (0)

inline int entropy_nbins_check(int nbins, EntropyWhy *why)
{
    if (nbins != kBins) CGIC_ENT_REFUSE(CGIC_ERR_UNSUPPORTED, "entropy: nbins=%d; the reference uses 32 (model.py:480)", nbins);
    return CGIC_OK;
}

// sigma and the bin centres.  window_words names the window whose width the sigma bound protects: "2-bin" (the kernels that evaluate
// the two bins around a pixel) or "five-bin" (the reference-arithmetic variant).
inline int entropy_setup_check(float sigma, const float *bins, const char *window_words, EntropyWhy *why)
{
    // The two-bin window drops kernel values <= exp(-0.5 ((2/31) / sigma)^2): 6.5e-9 at the bound below, 9e-10 at the
    // reference's sigma
    if (!(sigma > 0.f && sigma <= 0.0105f))
        CGIC_ENT_REFUSE(CGIC_ERR_UNSUPPORTED, "entropy: sigma=%g; the %s window assumes the reference's sigma=0.01 (model.py:481)", sigma, window_words);
    for (int i = 1; i < kBins; ++i)
        if (!(fabsf((bins[i] - bins[i - 1]) - 2.0f / 31.0f) < 1e-5f)) CGIC_ENT_REFUSE(CGIC_ERR_UNSUPPORTED, "entropy: bins are not linspace(-1, 1, 32)");
    return CGIC_OK;
}

// the image form: B images of H x W
inline int entropy_shape_check(int64_t B, int64_t H, int64_t W, EntropyWhy *why)
{
    if (!(B >= 0 && H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0))
        CGIC_ENT_REFUSE(CGIC_ERR_INVALID, "entropy: H=%lld W=%lld must be positive multiples of 16", (long long)H, (long long)W);
    if (!(B <= kEntMaxGrid && H / 16 <= kEntMaxGrid)) CGIC_ENT_REFUSE(CGIC_ERR_UNSUPPORTED, "entropy: batch/height exceed the grid limits");
    return CGIC_OK;
}

// the tiles form: T tiles of th x tw out of each of N source images of H x W
inline int entropy_shape_check(int64_t N, int64_t H, int64_t W, int T, int64_t th, int64_t tw, EntropyWhy *why)
{
    if (!(N >= 0 && H > 0 && W > 0 && H < (1 << 30) && W < (1 << 30))) CGIC_ENT_REFUSE(CGIC_ERR_INVALID, "entropy_maps_tiles: bad source shape");
    if (!(T >= 1 && T <= kEntMaxTiles))
        CGIC_ENT_REFUSE(CGIC_ERR_UNSUPPORTED, "entropy_maps_tiles: %d tiles per image in this group (1..%d): cut them with cgic_cut_tiles", T, kEntMaxTiles);
    if (!(th > 0 && tw > 0 && th % 16 == 0 && tw % 16 == 0))
        CGIC_ENT_REFUSE(CGIC_ERR_INVALID, "entropy_maps_tiles: tile %lldx%lld must be positive multiples of 16", (long long)th, (long long)tw);
    if (!(N * T <= kEntMaxGrid && th / 16 <= kEntMaxGrid)) CGIC_ENT_REFUSE(CGIC_ERR_UNSUPPORTED, "entropy: batch/height exceed the grid limits");
    return CGIC_OK;
}

// ... and its T tile origins (y0, x0).  A check of its own: the entry point looks at the origins last, and not at all when N == 0.
inline int entropy_origins_check(int T, const int *origins, EntropyWhy *why)
{
    for (int k = 0; k < 2 * T; ++k)
        if (!(origins[k] > -(1 << 29) && origins[k] < (1 << 29))) CGIC_ENT_REFUSE(CGIC_ERR_INVALID, "entropy_maps_tiles: tile origin out of range");
    return CGIC_OK;
}
#undef CGIC_ENT_REFUSE

struct EntropyPlan {
    bool nothing;               // no image or no output: the call returns without a launch
    unsigned int gx, gy, gz;    // the grid: workgroups along a row band of 16 rows, row bands, images
    float exp2_scale;
};

// `images` of H x W (multiples of 16), every wave of a workgroup walking ppw patches of its row band; has_outputs: the call writes
// at least one map or frame
inline EntropyPlan entropy_plan(int64_t H, int64_t W, int64_t images, int ppw, float sigma, bool has_outputs)
{
    EntropyPlan p;
    p.nothing = images == 0 || !has_outputs;
    const int64_t per_wg = (int64_t)kEntWaves * ppw;
    p.gx = (unsigned int)((W / 16 + per_wg - 1) / per_wg);
    p.gy = (unsigned int)(H / 16);
    p.gz = (unsigned int)images;
    // exp(-0.5 (r/sigma)^2) = exp2(c r^2), c = -0.5 log2(e) / sigma^2 (float64 on the host, rounded once)
    p.exp2_scale = (float)(-0.5 * 1.4426950408889634 / ((double)sigma * (double)sigma));
    return p;
}

}  // namespace cgic
