// cgic_coder_plan.h -- the sizes of the stream coder's buffers and the launch one cgic_compress_streams call makes, decided before
// anything is enqueued.  Plain C++17 on purpose (no HIP include, no stream, no device pointer): compress_plan() is a pure function
// of a CompressShape, so every decision of the compress host path can be exercised without a GPU (tests/host/coder_plan_main.cpp).
// cgic_coder.hip checks the arguments, calls compress_plan() once and issues what the plan says.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/cgic_hip.h"
#include "cgic_decode_plan.h"      // kTicketRequestMax

namespace cgic {

// 1024 -> 512 in round 3: with four batches in flight 36.3 -> 35.5 us per step (smaller workgroups find a CU sooner); alone +0.5 us
constexpr int kEncThreads = 512;         // x kEncItems = 4096 positions per scan round: one round per 256x256 stream
constexpr int kLdsPos = 8192;           // streams up to this many positions keep phase-A results in LDS
constexpr int kLdsPosSmall = 4096;              // ... and the small instantiation of the compress kernel (grids up to 64x64)
constexpr int kEncPartPos = 4096;         // positions per part of a split stream: measured 8192 -> 14.1 us, 4096 -> 12.2 us, 3072 -> 12.2 us (8 tiles of 768x768)
constexpr int kEncMaxParts = 7;           // descriptors of a stream fit two ticket slots: 4 words per part + the reader count
constexpr size_t kEncStageMax = 96 * 1024;      // bytes of dynamic LDS a workgroup may stage its positions in (static: 57.5 KB)

// positions of one part when a stream of npos positions is split over nparts workgroups: whole groups of four (the staging is read
// as 4-entry groups).  constexpr: the compress kernel calls it for its own range (compress_streams_body: `per`).
constexpr int64_t enc_part_positions(int64_t npos, int64_t nparts) { return (((npos + nparts - 1) / nparts) + 3) & ~(int64_t)3; }

// ---- sizes: the one statement of what the size queries of include/cgic_hip.h answer and of the workspace layout ----
constexpr size_t enc_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// bytes a stream of n symbols can take with codes of at most max_len bits
inline size_t stream_capacity(int max_len, int64_t n)
{
    const uint64_t bits = (uint64_t)max_len * (uint64_t)n;
    return enc_align16((size_t)(bits / 8 + 2) + 8);    // header + pad byte + word-store/fetch slack
}

// cgic_encode_stream's workspace: [n] end bits (u32), then [n] symbols (u16), each padded to 16 bytes
inline size_t stream_workspace_sym_offset(int64_t n) { return enc_align16((size_t)n * 4); }
inline size_t stream_workspace_bytes(int64_t n) { return n > kLdsPos ? stream_workspace_sym_offset(n) + enc_align16((size_t)n * 2) : 0; }

// one slot of cgic_compress_streams: the fine index stream at its longest, or the medium mask stream
inline size_t compress_slot_bytes(int max_len, int64_t h, int64_t w)
{
    const size_t a = stream_capacity(max_len, h * w);
    const size_t m = enc_align16((size_t)((h / 2) * (w / 2) / 8 + 2) + 8);
    return a > m ? a : m;
}

// cgic_compress_streams' workspace: [B, 3, stride] end bits (u32), then at sym_offset [B, 3, stride] symbols (u16)
struct CompressWs {
    size_t stride;          // positions reserved per (image, stream)
    size_t bytes;           // of the whole workspace; 0: grids up to kLdsPos positions need none
    size_t sym_offset;
};
inline CompressWs compress_ws(int64_t B, int64_t h, int64_t w)
{
    CompressWs ws;
    ws.stride = ((size_t)(h * w) + 7) & ~(size_t)7;
    const size_t entries = (size_t)(B > 0 ? B : 0) * 3 * ws.stride;
    ws.sym_offset = entries * sizeof(uint32_t);
    ws.bytes = h * w <= kLdsPos ? 0 : entries * (sizeof(uint32_t) + sizeof(uint16_t));
    return ws;
}

// ---- the launch ----
struct CompressShape {
    int64_t B, h, w;            // images, latent grid (check_grid has passed)
    int64_t slot;               // bytes per stream slot
    int max_len, nsym;          // of the table
    bool has_hist;              // the call wants the usage histogram
    bool has_workspace;
};

struct CompressPlan {
    int parts[3];               // workgroups per index stream (coarse, medium, fine); > 1: the stream is split
    int64_t stage_positions;    // entries of the dynamic-LDS staging buffer (0: none) ...
    size_t dyn_lds;             // ... and its bytes
    int tickets;                // ticket slots to acquire: 6 per image when a stream is split, else 0
    int combine;                // CompressArgs::combine: the short jobs of an image share one workgroup
    unsigned int jobs;          // workgroups per image; 0: nothing to do (B == 0)
    bool small;                 // the kLdsPosSmall instantiation of the kernel
    bool parts_fastest;         // grid (jobs, B) instead of (B, jobs): the parts of a stream are neighbours in dispatch order
    bool recorded;              // the launch has a grouped form (KID_COMPRESS); the small instantiation has none
    CompressWs ws;
    char why_text[96];          // the text of a refusal that names numbers
};

// CGIC_OK and the plan, or the error code of the call and *why
inline int compress_plan(const CompressShape &s, CompressPlan *p, const char **why)
{
    const int64_t B = s.B, h = s.h, w = s.w;
    *p = CompressPlan{};
    p->parts[0] = p->parts[1] = p->parts[2] = 1;
    p->ws = compress_ws(B, h, w);
    const size_t slot_need = compress_slot_bytes(s.max_len, h, w);
    if (!(s.slot % 16 == 0 && (size_t)s.slot >= slot_need)) {
        snprintf(p->why_text, sizeof(p->why_text), "compress_streams: slot=%lld, need a multiple of 16 >= %zu", (long long)s.slot, slot_need);
        *why = p->why_text;
        return CGIC_ERR_CAPACITY;
    }
    if (s.nsym > 65536) { *why = "table too large"; return CGIC_ERR_UNSUPPORTED; }
    if (!((uint64_t)s.max_len * (uint64_t)(h * w) < 0xFFFFFF00ull)) { *why = "compress_streams: a stream could exceed 2^32 bits"; return CGIC_ERR_UNSUPPORTED; }
    if (!s.has_workspace && p->ws.bytes != 0) {
        snprintf(p->why_text, sizeof(p->why_text), "compress_streams: workspace required for %lldx%lld grids", (long long)h, (long long)w);
        *why = p->why_text;
        return CGIC_ERR_INVALID;
    }
    if (B == 0) return CGIC_OK;                    // (before the histogram's bound: an empty batch asks for nothing)
    if (s.has_hist && s.nsym > kLdsPos) {
        snprintf(p->why_text, sizeof(p->why_text), "compress_streams: hist needs n <= %d", kLdsPos);
        *why = p->why_text;
        return CGIC_ERR_UNSUPPORTED;
    }
    // Streams beyond kLdsPos positions are split over workgroups of about kEncPartPos positions each, kEncMaxParts at most (a 768x768
    // tile: fine 36 864 positions -> 7 parts, medium 9216 -> 3) when the launch is small enough for one ticket request; every part
    // stages 2 bytes per position of its range in dynamic LDS.
    const bool split = B * 6 <= kTicketRequestMax;
    int64_t longest = 0;                  // positions the longest workgroup stages
    for (int g = 0; g < 3; ++g) {
        const int64_t npos = (h >> (2 - g)) * (w >> (2 - g));
        int64_t P = split && npos > kLdsPos ? (npos + kEncPartPos - 1) / kEncPartPos : 1;
        P = P > kEncMaxParts ? kEncMaxParts : P;
        p->parts[g] = (int)P;
        const int64_t per = P > 1 ? enc_part_positions(npos, P) : npos;
        if (npos > kLdsPos && per > longest) longest = per;
    }
    if (longest > 0 && (size_t)longest * 2 <= kEncStageMax) {
        p->dyn_lds = (((size_t)longest + 3) / 4 * 4 * 2 + 64 + 15) & ~(size_t)15;       // whole 4-entry groups (+ slack)
        p->stage_positions = longest;
    } else if (longest > 0) {
        p->parts[0] = p->parts[1] = p->parts[2] = 1;              // no staging room: the round-by-round form, unsplit
    }
    const int nparts = p->parts[0] + p->parts[1] + p->parts[2];
    p->tickets = nparts > 3 ? (int)(B * 6) : 0;
    p->parts_fastest = p->tickets != 0;
    // every index stream fits the static LDS arrays and nothing is split: the short jobs of an image share one workgroup
    p->combine = (!p->tickets && h * w <= kLdsPos) ? 1 : 0;
    // the kernel's jobs of an image (compress_streams_body): combined: fine | medium | coarse + both masks; else every part of the
    // three index streams and one job per mask stream; then the histogram
    p->jobs = (p->combine ? 3u : (unsigned int)nparts + 2u) + (s.has_hist ? 1u : 0u);
    p->small = p->combine && h * w <= kLdsPosSmall && (!s.has_hist || s.nsym <= kLdsPosSmall);
    p->recorded = !p->small;
    return CGIC_OK;
}

}  // namespace cgic
