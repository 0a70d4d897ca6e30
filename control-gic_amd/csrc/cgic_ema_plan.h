// cgic_ema_plan.h -- what the launches of a cgic_ema_plan do, decided when the plan is made: every check of the entries, the chunk
// table, which chunks move 16 bytes per lane, the grid and the size of the device tables.  Plain C++17 on purpose (no HIP include, no
// stream; pointers are plain addresses): ema_plan() is a pure function of the entry list, and ema_one_minus_decay() is the text the
// one-thread prologue kernel runs, so all of it can be exercised without a GPU (tests/host/ema_plan_main.cpp).  cgic_ema.hip calls
// ema_plan() once per cgic_ema_plan_create, uploads the two tables as they stand here and launches what the plan says.
//
// The work list:
//   entries  one per tensor pair: shadow, param, n and the tensor's offset in the stash of cgic_ema_copy (the element counts before
//            it, each rounded up to a multiple of 4: with a 16-byte aligned stash every tensor starts 16-byte aligned in it)
//   chunks   kEmaChunk elements of one tensor, the last one of a tensor shorter; a smaller tensor is one chunk, an empty one none.
//            Chunks of a tensor follow each other, tensors in entry order.
// A workgroup of kEmaThreads threads takes chunk blockIdx.x, blockIdx.x + grid ... ; grid = min(chunks, kEmaGridMax), 256 compute
// units x 8 workgroups (the idiom for memory-bound kernels).  A chunk begins a multiple of kEmaChunk elements into its tensor, so it
// is 16-byte aligned exactly where its tensor is: such a chunk moves len / 4 float4 and at most 3 single elements, any other chunk
// single elements.  The kernel decides that from the addresses themselves with ema_both_16 below; the plan counts with the same
// function what the kernel will decide.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/cgic_hip.h"

#if defined(__HIPCC__)
#define CGIC_EMA_HD __host__ __device__
#else
#define CGIC_EMA_HD
#endif

namespace cgic {

constexpr int kEmaThreads = 256;
constexpr int64_t kEmaChunk = 4096;         // elements: four float4 of each operand per lane
constexpr int kEmaGridMax = 2048;
constexpr size_t kEmaHeadBytes = 16;        // the plan's omd float, padded: the tables behind it stay 16-byte aligned
enum { EMA_COPY_TO = 0, EMA_STORE = 1, EMA_RESTORE = 2 };

struct EmaIn { uintptr_t shadow, param; int64_t n; };                        // (the layout of cgic_ema_entry)
struct EmaEntry { uintptr_t shadow, param; int64_t n, stash_off; };          // 32 bytes, as the kernels read it
struct EmaChunk { int32_t entry, len; int64_t off; };                        // 16 bytes
static_assert(sizeof(EmaEntry) == 32 && sizeof(EmaChunk) == 16 && sizeof(uintptr_t) == 8, "the device tables are read as these structs");

CGIC_EMA_HD inline bool ema_both_16(uintptr_t a, uintptr_t b) { return ((a | b) & 15) == 0; }

// num_updates after a call that found n there (ema.py:28-29): incremented when not negative, wrapping like an int32 tensor
CGIC_EMA_HD inline int32_t ema_next_count(int32_t n) { return n >= 0 ? (int32_t)((uint32_t)n + 1u) : n; }

// one_minus_decay of a call that found n in num_updates (ema.py:26-32; has_count false: no counter was given).  Three fp32
// operations: the division, the comparison and the subtraction.  cand < decay ? cand : decay is Python's min(decay, cand).
CGIC_EMA_HD inline float ema_one_minus_decay(float decay, int32_t n, bool has_count)
{
    if (has_count && n >= 0) {
        const uint32_t m = (uint32_t)ema_next_count(n);
        const float num = (float)(int32_t)(1u + m), den = (float)(int32_t)(10u + m);     // (int32 tensor + int: wraps)
        const float cand = num / den;
        decay = cand < decay ? cand : decay;
    }
    return 1.0f - decay;
}

struct EmaPlan {
    std::vector<EmaEntry> entries;
    std::vector<EmaChunk> chunks;
    int64_t elements;
    int64_t stash_elements;
    int64_t chunks16;               // chunks with shadow and param 16-byte aligned: update and EMA_COPY_TO
    int64_t chunks16_stash;         // chunks with param 16-byte aligned: EMA_STORE and EMA_RESTORE (the stash side always is)
    int grid;                       // 0: nothing to launch
    size_t table_bytes;             // head + entries + chunks
    size_t entries_at, chunks_at;   // byte offsets of the two tables in that allocation
    char why_text[224];
};

// CGIC_OK and the plan, or CGIC_ERR_INVALID and *why.  `in` is not read before `count` has been checked.
inline int ema_plan(const EmaIn *in, int64_t count, EmaPlan *p, const char **why)
{
    p->entries.clear(); p->chunks.clear();
    p->elements = p->stash_elements = p->chunks16 = p->chunks16_stash = 0;
    p->grid = 0; p->table_bytes = 0; p->entries_at = p->chunks_at = 0; p->why_text[0] = 0;
    const auto refuse = [&](int code) { *why = p->why_text; p->entries.clear(); p->chunks.clear(); return code; };
    if (count < 0 || count > (int64_t)INT32_MAX) {
        snprintf(p->why_text, sizeof(p->why_text), "ema_plan: %lld entries (0 .. 2^31 - 1: an entry index is an int32)", (long long)count);
        return refuse(CGIC_ERR_INVALID);
    }
    if (count > 0 && !in) {
        snprintf(p->why_text, sizeof(p->why_text), "ema_plan: NULL entry list with %lld entries", (long long)count);
        return refuse(CGIC_ERR_INVALID);
    }
    // ---- the checks and the chunk count, before anything is built
    int64_t nchunks = 0;
    for (int64_t i = 0; i < count; ++i) {
        const EmaIn &e = in[i];
        if (e.n < 0) {
            snprintf(p->why_text, sizeof(p->why_text), "ema_plan: entry %lld has %lld elements", (long long)i, (long long)e.n);
            return refuse(CGIC_ERR_INVALID);
        }
        if (e.n > 0 && (!e.shadow || !e.param)) {
            snprintf(p->why_text, sizeof(p->why_text), "ema_plan: entry %lld has a NULL %s with %lld elements", (long long)i, e.shadow ? "param" : "shadow",
                     (long long)e.n);
            return refuse(CGIC_ERR_INVALID);
        }
        if ((e.shadow | e.param) & 3) {
            snprintf(p->why_text, sizeof(p->why_text), "ema_plan: the %s of entry %lld is not aligned to its 4-byte element", e.shadow & 3 ? "shadow" : "param",
                     (long long)i);
            return refuse(CGIC_ERR_INVALID);
        }
        nchunks += e.n / kEmaChunk + (e.n % kEmaChunk != 0);          // (below 2^51 each, at most 2^31 of them: no overflow)
        if (nchunks > (int64_t)INT32_MAX) {
            snprintf(p->why_text, sizeof(p->why_text), "ema_plan: more than 2^31 - 1 chunks of %lld elements (a chunk index is an int32)", (long long)kEmaChunk);
            return refuse(CGIC_ERR_INVALID);
        }
    }
    // ---- the tables (elements <= 2^31 * kEmaChunk: no overflow)
    p->entries.reserve((size_t)count);
    p->chunks.reserve((size_t)nchunks);
    for (int64_t i = 0; i < count; ++i) {
        const EmaIn &e = in[i];
        p->entries.push_back(EmaEntry{e.shadow, e.param, e.n, p->stash_elements});
        for (int64_t off = 0; off < e.n; off += kEmaChunk) {
            const int64_t len = e.n - off < kEmaChunk ? e.n - off : kEmaChunk;
            p->chunks.push_back(EmaChunk{(int32_t)i, (int32_t)len, off});
            p->chunks16 += ema_both_16(e.shadow, e.param);
            p->chunks16_stash += ema_both_16(e.param, 0);
        }
        p->elements += e.n;
        p->stash_elements += (e.n + 3) / 4 * 4;
    }
    p->grid = (int)(nchunks < kEmaGridMax ? nchunks : kEmaGridMax);
    p->entries_at = kEmaHeadBytes;
    p->chunks_at = p->entries_at + sizeof(EmaEntry) * p->entries.size();
    p->table_bytes = p->chunks_at + sizeof(EmaChunk) * p->chunks.size();
    return CGIC_OK;
}

}  // namespace cgic
