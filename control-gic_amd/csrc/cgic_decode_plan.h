// cgic_decode_plan.h -- which launches one cgic_decompress_streams call makes, decided before anything is enqueued.
// Plain C++17 on purpose (no HIP include, no stream, no device pointer): decode_plan() is a pure function of a DecodeShape, so
// every decision of the decode host path can be exercised without a GPU (tests/host/decode_plan_main.cpp).  cgic_decode.hip
// checks the arguments, calls decode_plan() once and issues what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cgic_hip.h"

namespace cgic {

constexpr int kDecThreads = 1024;         // workgroup of the prefix decoders and of the fused decoder + merge launch
constexpr int kSsThreadsSmall = 256;      // the self-synchronising decoder's workgroup for small streams (large ones: kDecThreads)
constexpr int kMergeThreads = 512;
constexpr int kMergeOneBandThreads = 512;       // throughput mode: one band per image (1024 until round 3: 512 measured ~0.5-1 us per step better in flight)
constexpr int kMergeBands = 4;          // row bands per image at least; more for few large images (gridDim.x)

// decoder workgroups per image (decode_split_kernel): grids up to 64x64 | beyond | beyond when the merge rides in the launch -- 16 are
// as fast as 24 per call, and the CUs they leave go to merge bands (2040x1356 chain 0.105 -> 0.104 ms; 12 falls off the fast path)
constexpr unsigned int kDecWgsSmall = 4, kDecWgsLarge = 24, kDecWgsFusedLarge = 16;
// merge bands per image are doubled while the launch has fewer than kMergeWgs workgroups and a band keeps 2 x kMergeMinRows coarse rows
constexpr int64_t kMergeWgs = 256, kMergeMinRows = 1;

constexpr size_t kLdsBudget = 150 * 1024;       // dynamic LDS a decode-side workgroup may ask for
constexpr size_t kLdsMergeStage = 64 * 1024;    // the merge stages the codebook and symbols only while its LDS stays within this
constexpr int kSplitMaxLen = 64;                // longest code of the split-stream and self-synchronising decoders
// ticket slots that one acquire_tickets request can cover: a quarter of a stream's ring (cgic_table.hip)
constexpr int64_t kTicketRequestMax = 16384 / 4;

enum DecoderPath { DECODER_FUSED, DECODER_IMAGE, DECODER_SPLIT, DECODER_SERIAL };
enum MergeForm { MERGE_BANDS, MERGE_ONE_BAND };

struct DecodeShape {
    int64_t B, h, w;            // images, latent grid
    int64_t slot;               // bytes per stream slot
    int K;                      // codebook rows
    bool has_zq;                // the call gathers codebook rows (z_q given)
    int max_len, lut_bits;      // of the table
    int dec_mode;               // CGIC_DECODE_*: the call's, or for AUTO the process default (which may be AUTO: neither promise made)
    int cus;                    // compute units of the device
    double cu_share;            // the launch group's share of them (1.0 outside a group)
    bool no_fuse;               // dev knob CGIC_NO_DECODE_MERGE
    size_t lds_decoder;         // LDS of the split-stream and serial decoders (it depends on device struct sizes: decoder_lds_bytes)
};

struct DecodePlan {
    DecoderPath decoder;
    MergeForm merge;            // of the merge launch that follows the decoder (DECODER_FUSED has its bands in the same launch)
    unsigned int ndec;          // decoder workgroups per image
    int64_t nbands;             // merge bands per image ...
    unsigned int active_bands;  // ... of which this many have rows
    int stage_cb, stage_sym;    // MergeArgs: the codebook | the image's symbols are staged in LDS
    int64_t band_syms;          // MergeArgs: u16 entries a band stages of its own when the image's symbols do not fit
    size_t lds_d, lds_m, lds_f, lds_ss;     // split-stream or serial decoder | merge | fused launch | self-synchronising decoder
    size_t stage_cap, chunk_cap;            // DECODER_IMAGE: bytes of its stream stage and of each chunk table
    int image_threads;                      // DECODER_IMAGE: its workgroup
    int64_t split_batch;                    // DECODER_SPLIT: images per launch
};

// CGIC_OK and the plan, or the error code of the call and *why
inline int decode_plan(const DecodeShape &s, DecodePlan *p, const char **why)
{
    const auto align16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const int64_t B = s.B, h = s.h, w = s.w;
    const size_t per = (size_t)((h / 4) * (w / 4) + (h / 2) * (w / 2) + h * w);      // symbols of an image's three grids
    const bool large = h * w > 64 * 64;
    *p = DecodePlan{};

    // ---- the merge's LDS: three mask bitsets per grid, then the codebook and the image's symbols while they fit ----
    const size_t wc = (size_t)(((h / 4) * (w / 4) + 31) / 32), wm = (size_t)(((h / 2) * (w / 2) + 31) / 32);
    size_t lds_m = (3 * (wc + wm) + 4) * sizeof(uint32_t);
    if (lds_m > kLdsBudget) { *why = "decompress_streams: grid too large for the mask bitsets"; return CGIC_ERR_UNSUPPORTED; }
    p->stage_cb = (s.has_zq && lds_m + (size_t)s.K * 16 <= kLdsMergeStage) ? 1 : 0;
    if (p->stage_cb) lds_m += (size_t)s.K * 16;
    p->stage_sym = (per % 2 == 0 && lds_m + per * 2 + 4 <= kLdsMergeStage) ? 1 : 0;
    if (p->stage_sym) lds_m += ((per + 1) / 2) * 4;
    // mask-stream slots must cover the word-wise staging reads
    if ((size_t)s.slot < (wm + 2) * 4) { *why = "decompress_streams: slot smaller than a mask stream"; return CGIC_ERR_CAPACITY; }

    // ---- decoder and merge as ONE launch? ----
    // Decoder and merge go out as ONE launch when every workgroup of both gets a CU of its own (B = 1 .. a few dozen images, or
    // a few tiles; inside a launch group: within the group's share of the chip)
    const int64_t cu_share = (int64_t)((double)s.cus * s.cu_share + 0.5);
    // The fused launch's merge bands SPIN on the decoder workgroups of the same launch (wait_decoded).  Alone on the chip that cannot
    // hang: the decoders sit in front of the bands in the grid and every one gets a CU at once.  With other launches of this kind in
    // flight on other queues (up to four hardware queues by default), an XCD could in principle fill up with spinning bands of
    // several launches whose decoders are queued behind each other's bands.  The chip holds two of these 1024-thread workgroups per
    // CU: as long as FOUR such launches together fit (each at most half the CUs' worth of workgroups), every workgroup of every one
    // of them is resident at once and nobody waits for a slot.  CGIC_DECODE_LATENCY is the caller's statement that this call has
    // the GPU to itself (one batch at a time): it keeps the whole chip as its budget.
    const int64_t cu_budget = s.dec_mode == CGIC_DECODE_LATENCY ? cu_share : cu_share / 2;
    const int64_t ndec_fused = large ? kDecWgsFusedLarge : kDecWgsSmall;
    // (the fused launch takes its 3 + 1 tickets per image in one request each)
    const bool may_fuse = s.dec_mode != CGIC_DECODE_THROUGHPUT && s.max_len <= kSplitMaxLen && B * 3 <= kTicketRequestMax && !s.no_fuse;
    const auto fusable = [&](int64_t nbands) { return may_fuse && B * (ndec_fused + nbands) <= cu_budget; };

    // ---- merge bands ----
    // 4 bands per image fill the GPU at B = 64; a few large tiles get more (every band re-derives the mask prefixes,
    // so not more than needed): ~256 workgroups in all, at least 2 coarse rows per band
    const int64_t h4 = h >> 2;
    int64_t nbands = kMergeBands;
    while (nbands * B < kMergeWgs && nbands * 2 <= h4 / kMergeMinRows) {
        if (fusable(nbands) && !fusable(nbands * 2)) break;        // keep a small launch fusable with its decoder
        nbands *= 2;
    }
    const int64_t rows_per = ((h4 + nbands - 1) / nbands) * 4;
    p->nbands = nbands;
    p->active_bands = (unsigned int)((h + rows_per - 1) / rows_per);
    // the image's symbols do not fit LDS: every band stages its own three rank ranges (at most 21/16 symbols per position)
    if (!p->stage_sym) {
        const int64_t need = rows_per * w * 21 / 16 + 8;
        if (lds_m + (size_t)need * 2 <= kLdsMergeStage) { p->band_syms = need; lds_m += (size_t)need * 2; }
    }
    p->lds_m = lds_m;
    p->lds_d = s.lds_decoder;
    p->lds_f = p->lds_d > lds_m ? p->lds_d : lds_m;
    // several batches in flight: one band per image (see merge_kernel)
    p->merge = s.dec_mode == CGIC_DECODE_THROUGHPUT && !large && p->stage_sym ? MERGE_ONE_BAND : MERGE_BANDS;

    // ---- which decoder ----
    if (fusable(nbands)) {
        p->decoder = DECODER_FUSED;
        p->ndec = (unsigned int)ndec_fused;
        return CGIC_OK;
    }
    if (s.max_len > kSplitMaxLen) {
        // tables with codes longer than 64 bits take the one-wave path of decode_streams_kernel: a workgroup per stream
        p->decoder = DECODER_SERIAL;
        p->ndec = 3;
        return CGIC_OK;
    }
    if (s.dec_mode == CGIC_DECODE_THROUGHPUT) {
        // The self-synchronising one-workgroup-per-image decoder when the worst case of the grid fits its LDS: bits <= symbols
        // the three grids can hold x the longest code.  (Longer inputs are an overflow on any path.)
        const size_t bits_cap = per * (size_t)s.max_len + 3 * 64;
        const size_t stage_cap = align16(bits_cap / 8 + 3 * 48), chunk_cap = align16(bits_cap / 64 + 8);
        const size_t lds_ss = sizeof(uint32_t) * ((size_t)1 << s.lut_bits) + stage_cap + 3 * chunk_cap;
        if (lds_ss <= kLdsBudget) {
            p->decoder = DECODER_IMAGE;
            p->ndec = 1;
            p->stage_cap = stage_cap; p->chunk_cap = chunk_cap; p->lds_ss = lds_ss;
            p->image_threads = large ? kDecThreads : kSsThreadsSmall;
            return CGIC_OK;
        }
    }
    // Streams are split over workgroups that exchange range functions (decode_split_kernel): 4 workgroups per image for grids
    // up to 64x64 (a 256x256 image), 24 beyond, dealt to the streams by length on the device.
    p->decoder = DECODER_SPLIT;
    p->ndec = large ? kDecWgsLarge : kDecWgsSmall;
    // one ticket request covers 3 slots per image: larger batches are cut into several launches of the same kernel
    p->split_batch = kTicketRequestMax / 3;
    return CGIC_OK;
}

}  // namespace cgic
