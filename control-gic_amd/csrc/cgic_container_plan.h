// cgic_container_plan.h -- what the launches of cgic_container_pack / cgic_container_unpack look like, decided before anything is
// enqueued: header bytes, the capacity that always suffices, the workspace layout, how many stage launches carry the entry table
// and the grid of the copy.
// Plain C++17 on purpose (no HIP include, no stream; the device pointers of a group are never dereferenced here): the plans are
// pure functions of the two tables, so every limit can be exercised without a GPU (tests/host/container_plan_main.cpp).
// cgic_container.hip checks the pointers, calls the plans and issues what they say.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/cgic_hip.h"

namespace cgic {

constexpr int kContainerHeaderBytes = 12;       // "CGIC" | u16 version | u16 flags | u32 n_entries
constexpr int kContainerEntryBytes = 44;        // 5 x u32 rectangle + id | u8 mode + 3 pad | 5 x i32 length
constexpr int kContainerLensAt = 24;            // the five lengths inside an entry header
constexpr int kContainerVersion = 1;
constexpr int64_t kContainerMaxEntries = 65535;
constexpr int kContainerMaxGroups = 64;
// entries that ride in the kernel-argument block of ONE stage launch, next to the group table (both tables are host arrays: a
// launch's arguments are the one host-to-device path that a graph capture copies when it is recorded)
constexpr int kContainerStageEntries = 64;
constexpr int kContainerStageThreads = kContainerStageEntries * CGIC_NUM_STREAMS;
constexpr int kContainerScanThreads = 1024;
constexpr int kContainerCopyThreads = 256;      // one thread per 16-byte word of the destination, grid-stride
constexpr int64_t kContainerCopyMaxBlocks = 2048;

constexpr int64_t container_header_bytes(int64_t E) { return kContainerHeaderBytes + (int64_t)kContainerEntryBytes * E; }
constexpr size_t container_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// the capacity that always suffices: every stream of every entry as long as the largest slot
inline size_t container_bound(const cgic_container_group *groups, int G, int64_t E)
{
    if (E < 0 || G < 0 || (G && !groups)) return 0;
    int64_t slot = 0;
    for (int g = 0; g < G; ++g)
        if (groups[g].slot > slot) slot = groups[g].slot;
    return (size_t)container_header_bytes(E) + (size_t)E * CGIC_NUM_STREAMS * (size_t)slot;
}

// workspace: int64 off[n + 1] (blob offset of every stream; off[n] = end of the payload), int64 words[n + 1] (unpack: prefix of
// the 16-byte words each stream's slot receives), the slot address and the length word of every stream; n = 5 E
struct ContainerWorkspace {
    size_t off, words, ptr, len, bytes;
};
inline ContainerWorkspace container_workspace(int64_t E)
{
    const size_t n = (size_t)(E > 0 ? E : 0) * CGIC_NUM_STREAMS;
    ContainerWorkspace w;
    w.off = 0;
    w.words = w.off + container_align16(8 * (n + 1));
    w.ptr = w.words + container_align16(8 * (n + 1));
    w.len = w.ptr + container_align16(8 * n);
    w.bytes = w.len + container_align16(4 * n);
    return w;
}

enum ContainerWhy { CONTAINER_PLANNED, CONTAINER_ENTRIES, CONTAINER_GROUPS, CONTAINER_GROUP_SHAPE, CONTAINER_ENTRY_GROUP, CONTAINER_ENTRY_INDEX,
                    CONTAINER_CAPACITY, CONTAINER_MAGIC, CONTAINER_VERSION, CONTAINER_COUNT, CONTAINER_TRUNCATED, CONTAINER_LENGTH,
                    CONTAINER_SIZE, CONTAINER_MODE, CONTAINER_STREAM_SET, CONTAINER_SLOT };

inline const char *container_why_text(ContainerWhy w)
{
    static const char *const text[] = {
        "planned", "entries outside 0 .. 65535", "groups outside 0 .. 64 (or entries without a group)",
        "a group's B is negative, its slot no positive multiple of 16 below 2^31 or its mode outside 0 .. 6", "an entry names a group outside the table",
        "an entry's index is outside its group", "negative capacity", "not a CGIC container (magic)", "unknown container version",
        "the entry count of the header is not the entry table's", "the blob ends inside its headers", "a stream length below -1",
        "header plus stream lengths is not the blob's size", "an entry's mode is not its group's",
        "an entry's streams are not the set its mode writes", "a stream does not fit its slot (length + 8 bytes)"};
    return text[w];
}

struct ContainerPlan {
    int64_t header_bytes;       // 12 + 44 E: where the payload starts
    int64_t streams;            // 5 E
    int stage_launches;         // ceil(E / kContainerStageEntries)
    int64_t copy_words;         // pack: 16-byte words the capacity holds from the payload's first word on; unpack: slot words written
    int64_t copy_blocks;        // grid of the copy (0: no launch)
    ContainerWorkspace ws;
};

// the limits both directions share; index < B_g is part of them
inline int container_tables_check(const cgic_container_group *groups, int G, const cgic_container_entry *entries, int64_t E, ContainerWhy *why)
{
    if (E < 0 || E > kContainerMaxEntries || (E && !entries)) { *why = CONTAINER_ENTRIES; return CGIC_ERR_INVALID; }
    if (G < 0 || G > kContainerMaxGroups || (G && !groups) || (E && !G)) { *why = CONTAINER_GROUPS; return CGIC_ERR_INVALID; }
    for (int g = 0; g < G; ++g)
        if (groups[g].B < 0 || groups[g].slot <= 0 || groups[g].slot % 16 || groups[g].slot >= ((int64_t)1 << 31) || groups[g].mode < 0 || groups[g].mode > 6) {
            *why = CONTAINER_GROUP_SHAPE;
            return CGIC_ERR_INVALID;
        }
    for (int64_t e = 0; e < E; ++e) {
        if (entries[e].group < 0 || entries[e].group >= G) { *why = CONTAINER_ENTRY_GROUP; return CGIC_ERR_INVALID; }
        if (entries[e].index < 0 || entries[e].index >= groups[entries[e].group].B) { *why = CONTAINER_ENTRY_INDEX; return CGIC_ERR_INVALID; }
    }
    return CGIC_OK;
}

inline int64_t container_copy_blocks(int64_t words)
{
    const int64_t b = (words + kContainerCopyThreads - 1) / kContainerCopyThreads;
    return b < kContainerCopyMaxBlocks ? b : kContainerCopyMaxBlocks;
}

// CGIC_OK and the plan, or the error code of the call and *why
inline int container_pack_plan(const cgic_container_group *groups, int G, const cgic_container_entry *entries, int64_t E, int64_t capacity,
                               ContainerPlan *p, ContainerWhy *why)
{
    *p = ContainerPlan{};
    *why = CONTAINER_PLANNED;
    const int rc = container_tables_check(groups, G, entries, E, why);
    if (rc) return rc;
    if (capacity < 0) { *why = CONTAINER_CAPACITY; return CGIC_ERR_INVALID; }
    p->header_bytes = container_header_bytes(E);
    p->streams = E * CGIC_NUM_STREAMS;
    p->stage_launches = (int)((E + kContainerStageEntries - 1) / kContainerStageEntries);
    // the payload's words: from the word that holds its first byte to the end of the capacity (how many of them the blob really
    // has is known on the device only: the threads beyond `total` leave at once)
    const int64_t first = p->header_bytes / 16, last = (capacity + 15) / 16;
    p->copy_words = E && last > first ? last - first : 0;
    p->copy_blocks = container_copy_blocks(p->copy_words);
    p->ws = container_workspace(E);
    return CGIC_OK;
}

inline uint32_t container_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the inverse: `blob` is the HOST copy of the file, validated in full before anything is enqueued.  mode_streams[m] = the stream
// set mode m writes (bit i = stream i: cgic_mode_streams)
inline int container_unpack_plan(const uint8_t *blob, int64_t bytes, const cgic_container_group *groups, int G, const cgic_container_entry *entries,
                                 int64_t E, const int *mode_streams, ContainerPlan *p, ContainerWhy *why)
{
    *p = ContainerPlan{};
    *why = CONTAINER_PLANNED;
    const int rc = container_tables_check(groups, G, entries, E, why);
    if (rc) return rc;
    if (!blob || bytes < kContainerHeaderBytes) { *why = CONTAINER_TRUNCATED; return CGIC_ERR_INVALID; }
    if (memcmp(blob, "CGIC", 4) != 0) { *why = CONTAINER_MAGIC; return CGIC_ERR_INVALID; }
    if ((container_le32(blob + 4) & 0xFFFFu) != (uint32_t)kContainerVersion) { *why = CONTAINER_VERSION; return CGIC_ERR_UNSUPPORTED; }      // (flags: not looked at, as container.unpack)
    if ((int64_t)container_le32(blob + 8) != E) { *why = CONTAINER_COUNT; return CGIC_ERR_INVALID; }
    p->header_bytes = container_header_bytes(E);
    if (bytes < p->header_bytes) { *why = CONTAINER_TRUNCATED; return CGIC_ERR_INVALID; }
    int64_t at = p->header_bytes, words = 0;
    for (int64_t e = 0; e < E; ++e) {
        const uint8_t *h = blob + kContainerHeaderBytes + kContainerEntryBytes * e;
        const cgic_container_group &g = groups[entries[e].group];
        if ((int)h[20] != g.mode) { *why = CONTAINER_MODE; return CGIC_ERR_INVALID; }
        for (int s = 0; s < CGIC_NUM_STREAMS; ++s) {
            const int32_t len = (int32_t)container_le32(h + kContainerLensAt + 4 * s);
            if (len < -1) { *why = CONTAINER_LENGTH; return CGIC_ERR_INVALID; }
            if ((len >= 0) != ((mode_streams[g.mode] >> s & 1) != 0)) { *why = CONTAINER_STREAM_SET; return CGIC_ERR_INVALID; }
            if (len < 0) continue;
            if ((int64_t)len + 8 > g.slot) { *why = CONTAINER_SLOT; return CGIC_ERR_CAPACITY; }
            at += len;
            words += ((int64_t)len + 7) / 16 + 1;          // through the word that holds byte len + 7
        }
    }
    if (at != bytes) { *why = CONTAINER_SIZE; return CGIC_ERR_INVALID; }
    p->streams = E * CGIC_NUM_STREAMS;
    p->stage_launches = (int)((E + kContainerStageEntries - 1) / kContainerStageEntries);
    p->copy_words = words;
    p->copy_blocks = container_copy_blocks(words);
    p->ws = container_workspace(E);
    return CGIC_OK;
}

}  // namespace cgic
