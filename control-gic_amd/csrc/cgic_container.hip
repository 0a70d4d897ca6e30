// cgic_container.hip -- the container of control_gic_amd/container.py (version 1) built and taken apart on the device: G groups of
// slot buffers [B_g, 5, slot_g] <-> one contiguous blob `header | E entry headers | payload`, byte-identical to container.pack.
// Stream-ordered launches only: no workgroup waits on another, no global atomics.
//   stage   the two host tables reach the device in the kernel-argument block (kContainerStageEntries entries a launch): per stream
//           its slot address and its length word go to the workspace; pack writes the 44-byte entry headers, unpack writes nbytes
//   scan    ONE workgroup: the 5 E clamped lengths -> int64 blob offsets; pack: the 12-byte header and `total`
//   copy    pack: one thread per 16-byte word of the BLOB gathers the streams that overlap it (a word can hold many: the shortest
//           non-empty file is 2 bytes, empty and absent streams make offsets coincide) -- aligned 16-byte loads from the slots, a byte
//           funnel shift, aligned 16-byte stores inside the payload, byte stores at its two edges.  unpack: one thread per 16-byte
//           word of a SLOT, aligned loads from the blob, the same funnel, bytes past the stream's end zeroed.
#include "cgic_common.h"
#include "cgic_container_plan.h"

namespace cgic {
namespace {

struct ContainerGroupDev {
    unsigned char *data;
    int32_t *nbytes;
    uint32_t slot;
    int32_t mode;
};

struct StageArgs {
    ContainerGroupDev g[kContainerMaxGroups];
    cgic_container_entry e[kContainerStageEntries];
    unsigned char *blob;        // pack: the blob under construction; unpack: the device copy of the file
    int64_t capacity;           // pack
    int64_t *ptr;               // workspace: slot address of every stream ...
    int32_t *len;               // ... and its length word
    int base, count;            // entries [base, base + count) of the table
};
static_assert(sizeof(StageArgs) <= 4096, "the stage launch's tables must fit the kernarg segment");

struct ScanArgs {
    const int32_t *len;
    int64_t *off, *words;
    int64_t n, header_bytes, capacity, entries;
    unsigned char *blob;        // pack only
    int64_t *total;             // pack only
};

struct CopyArgs {
    const int64_t *off, *words, *ptr;
    const int32_t *len;
    unsigned char *blob;
    const int64_t *total;
    int64_t n, header_bytes, nwords, blob_words;
};

template <bool kPack>
__global__ __launch_bounds__(kContainerStageThreads) void container_stage_kernel(StageArgs a)
{
    const int t = threadIdx.x, e = t / CGIC_NUM_STREAMS, s = t - e * CGIC_NUM_STREAMS;
    if (e >= a.count) return;
    const cgic_container_entry &en = a.e[e];
    const ContainerGroupDev &g = a.g[en.group];
    const int64_t row = (int64_t)en.index * CGIC_NUM_STREAMS;
    const int64_t i = (int64_t)(a.base + e) * CGIC_NUM_STREAMS + s;
    unsigned char *head = a.blob + kContainerHeaderBytes + (int64_t)kContainerEntryBytes * (a.base + e);
    a.ptr[i] = (int64_t)(uintptr_t)(g.data + (row + s) * (int64_t)g.slot);
    if (kPack) {
        int32_t v = g.nbytes[row + s];
        if (v > (int32_t)g.slot) v = CGIC_ERR_CAPACITY - 10;       // (no coder writes that: the copy must never read past a slot)
        a.len[i] = v;
        if (s == 0 && kContainerHeaderBytes + (int64_t)kContainerEntryBytes * (a.base + e + 1) <= a.capacity) {
            uint32_t *h = reinterpret_cast<uint32_t *>(head);      // (the blob is 16-byte aligned, an entry header 4-byte)
            h[0] = en.image_id; h[1] = en.y; h[2] = en.x; h[3] = en.height; h[4] = en.width;
            h[5] = (uint32_t)g.mode & 0xFFu;
#pragma unroll
            for (int k = 0; k < CGIC_NUM_STREAMS; ++k) {
                const int32_t w = g.nbytes[row + k];
                h[6 + k] = (uint32_t)(w < -1 ? -1 : w);
            }
        }
    } else {
        int32_t v = reinterpret_cast<const int32_t *>(head + kContainerLensAt)[s];
        // (the host checked its copy of the file before the launch; a device copy that differs must still never leave a slot)
        if (v < -1 || (int64_t)v + 8 > (int64_t)g.slot) v = -1;
        a.len[i] = v;
        g.nbytes[row + s] = v;
    }
}

// words of its slot a stream of `len` bytes fills on the way in: through the word that holds byte len + 7 (the decoders' word fetches)
__device__ __forceinline__ int64_t slot_words(int32_t len) { return len < 0 ? 0 : ((int64_t)len + 7) / 16 + 1; }

template <bool kPack>
__global__ __launch_bounds__(kContainerScanThreads) void container_scan_kernel(ScanArgs a)
{
    __shared__ int64_t sm[kContainerScanThreads / kWave + 1];
    __shared__ int smin;
    const int t = threadIdx.x;
    if (t == 0) smin = 0;
    __syncthreads();
    int64_t at = a.header_bytes, wat = 0;
    int lowest = 0;
    for (int64_t base = 0; base < a.n; base += kContainerScanThreads) {
        const int64_t i = base + t;
        const int32_t v = i < a.n ? a.len[i] : -1;
        lowest = v < lowest ? v : lowest;
        int64_t tot;
        const int64_t ex = block_exclusive_scan<int64_t>(v > 0 ? v : 0, sm, &tot);
        if (i < a.n) a.off[i] = at + ex;
        at += tot;
        if (!kPack) {
            const int64_t wx = block_exclusive_scan<int64_t>(slot_words(v), sm, &tot);
            if (i < a.n) a.words[i] = wat + wx;
            wat += tot;
        }
    }
    if (lowest < -1) atomicMin(&smin, lowest);          // (LDS)
    __syncthreads();
    if (t != 0) return;
    a.off[a.n] = at;
    if (!kPack) { a.words[a.n] = wat; return; }
    if (a.capacity >= kContainerHeaderBytes) {
        uint32_t *h = reinterpret_cast<uint32_t *>(a.blob);
        h[0] = 0x43494743u;                             // "CGIC"
        h[1] = (uint32_t)kContainerVersion;             // u16 version | u16 flags = 0
        h[2] = (uint32_t)a.entries;
    }
    *a.total = smin < -1 ? (int64_t)smin : at > a.capacity ? (int64_t)(CGIC_ERR_CAPACITY - 10) : at;
}

// the 16 bytes at byte r (0 .. 15) of the 32 bytes lo | hi
__device__ __forceinline__ uint4 funnel16(const uint4 lo, const uint4 hi, unsigned int r)
{
    const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    const unsigned int q = r >> 2, sh = (r & 3u) * 8u;
    uint32_t e[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) e[j] = q == 0 ? d[j] : q == 1 ? d[j + 1] : q == 2 ? d[j + 2] : d[j + 3];
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (uint32_t)((((uint64_t)e[j + 1] << 32) | e[j]) >> sh);
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// byte mask of a dword from four byte-enable bits
__device__ __forceinline__ uint32_t spread4(unsigned int nib)
{
    return ((nib & 1u) | (nib & 2u) << 7 | (nib & 4u) << 14 | (nib & 8u) << 21) * 0xFFu;
}

__device__ __forceinline__ uint4 load16(const unsigned char *p) { return *reinterpret_cast<const uint4 *>(p); }

__global__ __launch_bounds__(kContainerCopyThreads) void container_pack_copy_kernel(CopyArgs a)
{
    const int64_t total = *a.total;
    if (total <= a.header_bytes) return;            // an error (negative), or no payload
    const int64_t first = a.header_bytes / 16, last = (total + 15) / 16;       // words [first, last) hold payload
    for (int64_t w = first + (int64_t)blockIdx.x * kContainerCopyThreads + threadIdx.x; w < last; w += (int64_t)gridDim.x * kContainerCopyThreads) {
        const int64_t W = 16 * w;
        const int64_t lo = W > a.header_bytes ? W : a.header_bytes, hi = W + 16 < total ? W + 16 : total;
        // the first stream that ends behind `lo` (off[n] = total > lo: there is one)
        int64_t l = 0, r = a.n - 1;
        while (l < r) {
            const int64_t m = (l + r) >> 1;
            if (a.off[m + 1] > lo) r = m; else l = m + 1;
        }
        uint32_t acc[4] = {0, 0, 0, 0};
        unsigned int have = 0;
        int64_t a0 = a.off[l];
        for (int64_t i = l; i < a.n && a0 < hi; ++i) {
            const int64_t b0 = a.off[i + 1];
            const int64_t sa = a0 > lo ? a0 : lo, sb = b0 < hi ? b0 : hi;
            if (sa < sb) {
                const int64_t len = b0 - a0, rel = W - a0;      // the word's byte j is the stream's byte rel + j
                const int64_t k0 = rel >> 4;                    // (floor: rel >= -15)
                const unsigned char *src = reinterpret_cast<const unsigned char *>((uintptr_t)a.ptr[i]);
                const uint4 zero = make_uint4(0, 0, 0, 0);
                const uint4 v0 = k0 >= 0 && 16 * k0 < len ? load16(src + 16 * k0) : zero;
                const uint4 v1 = 16 * (k0 + 1) < len ? load16(src + 16 * (k0 + 1)) : zero;
                const uint4 v = funnel16(v0, v1, (unsigned int)(rel & 15));
                const unsigned int en = ((1u << (unsigned int)(sb - W)) - 1u) & ~((1u << (unsigned int)(sa - W)) - 1u);
                const uint32_t in[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t m = spread4(en >> (4 * j) & 15u);
                    acc[j] = (acc[j] & ~m) | (in[j] & m);
                }
                have |= en;
            }
            a0 = b0;
        }
        if (have == 0xFFFFu) {
            *reinterpret_cast<uint4 *>(a.blob + W) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
        } else {                                    // the payload's first and last word: the headers in front, nothing behind `total`
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (have >> j & 1u) a.blob[W + j] = (unsigned char)(acc[j >> 2] >> (8 * (j & 3)));
        }
    }
}

__global__ __launch_bounds__(kContainerCopyThreads) void container_unpack_copy_kernel(CopyArgs a)
{
    for (int64_t t = (int64_t)blockIdx.x * kContainerCopyThreads + threadIdx.x; t < a.nwords; t += (int64_t)gridDim.x * kContainerCopyThreads) {
        // the stream whose slot words [words[i], words[i + 1]) hold t (absent streams have none)
        int64_t l = 0, r = a.n - 1;
        while (l < r) {
            const int64_t m = (l + r) >> 1;
            if (a.words[m + 1] > t) r = m; else l = m + 1;
        }
        const int64_t k = t - a.words[l], len = a.len[l];
        if (k < 0 || k >= slot_words((int32_t)len)) continue;      // (only if the device copy is not the file the host planned for)
        const int64_t rel = a.off[l] + 16 * k, k0 = rel >> 4;       // the slot word's byte j is the blob's byte rel + j
        const uint4 zero = make_uint4(0, 0, 0, 0);
        uint4 v = zero;
        if (16 * k < len) {
            const uint4 v0 = k0 < a.blob_words ? load16(a.blob + 16 * k0) : zero;
            const uint4 v1 = k0 + 1 < a.blob_words ? load16(a.blob + 16 * (k0 + 1)) : zero;
            v = funnel16(v0, v1, (unsigned int)(rel & 15));
            const int64_t keep = len - 16 * k;                      // bytes of the stream in this word
            if (keep < 16) {
                const unsigned int en = (1u << (unsigned int)keep) - 1u;
                v.x &= spread4(en & 15u); v.y &= spread4(en >> 4 & 15u); v.z &= spread4(en >> 8 & 15u); v.w &= spread4(en >> 12 & 15u);
            }
        }
        *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>((uintptr_t)a.ptr[l]) + 16 * k) = v;
    }
}

int fill_groups(StageArgs *a, const cgic_container_group *groups, int G, const char *what)
{
    memset((void *)a, 0, sizeof(*a));
    for (int g = 0; g < G; ++g) {
        // (a group without images has no buffers to point at)
        CGIC_REQUIRE(groups[g].B == 0 || (groups[g].data && groups[g].nbytes), CGIC_ERR_INVALID, "%s: group %d has no buffers", what, g);
        CGIC_REQUIRE((uintptr_t)groups[g].data % 16 == 0 && (uintptr_t)groups[g].nbytes % 4 == 0, CGIC_ERR_INVALID,
                     "%s: group %d: data must be 16-byte aligned, nbytes 4-byte", what, g);
        a->g[g].data = (unsigned char *)groups[g].data;
        a->g[g].nbytes = groups[g].nbytes;
        a->g[g].slot = (uint32_t)groups[g].slot;
        a->g[g].mode = groups[g].mode;
    }
    return CGIC_OK;
}

template <bool kPack>
int launch_stage(StageArgs *a, const cgic_container_entry *entries, int64_t E, const ContainerPlan &p, hipStream_t s)
{
    for (int c = 0; c < p.stage_launches; ++c) {
        a->base = c * kContainerStageEntries;
        a->count = (int)(E - a->base < kContainerStageEntries ? E - a->base : kContainerStageEntries);
        memcpy(a->e, entries + a->base, sizeof(cgic_container_entry) * (size_t)a->count);
        hipLaunchKernelGGL(container_stage_kernel<kPack>, dim3(1), dim3(kContainerStageThreads), 0, s, *a);
        const int rc = launch_check("container_stage_kernel");
        if (rc) return rc;
    }
    return CGIC_OK;
}

}  // namespace
}  // namespace cgic

using namespace cgic;

extern "C" size_t cgic_container_bound(const cgic_container_group *groups, int G, int64_t E)
{
    return container_bound(groups, G, E);
}

extern "C" size_t cgic_container_workspace_bytes(int64_t E)
{
    return E < 0 || E > kContainerMaxEntries ? 0 : container_workspace(E).bytes;
}

extern "C" int cgic_container_pack(const cgic_container_group *groups, int G, const cgic_container_entry *entries, int64_t E, uint8_t *blob,
                                   int64_t capacity, int64_t *total, void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_container_pack");
    ContainerPlan p;
    ContainerWhy why;
    const int rc0 = container_pack_plan(groups, G, entries, E, capacity, &p, &why);
    CGIC_REQUIRE(rc0 == CGIC_OK, rc0, "container_pack: %s", container_why_text(why));
    CGIC_REQUIRE(blob && total && workspace, CGIC_ERR_INVALID, "container_pack: NULL blob, total or workspace");
    CGIC_REQUIRE((uintptr_t)blob % 16 == 0 && (uintptr_t)total % 8 == 0 && (uintptr_t)workspace % 16 == 0, CGIC_ERR_INVALID,
                 "container_pack: blob and workspace must be 16-byte aligned, total 8-byte");
    StageArgs st;
    int rc = fill_groups(&st, groups, G, "container_pack");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    st.blob = blob; st.capacity = capacity;
    st.ptr = (int64_t *)(ws + p.ws.ptr); st.len = (int32_t *)(ws + p.ws.len);
    rc = launch_stage<true>(&st, entries, E, p, s);
    if (rc) return rc;
    ScanArgs sc;
    sc.len = st.len; sc.off = (int64_t *)(ws + p.ws.off); sc.words = (int64_t *)(ws + p.ws.words);
    sc.n = p.streams; sc.header_bytes = p.header_bytes; sc.capacity = capacity; sc.entries = E; sc.blob = blob; sc.total = total;
    hipLaunchKernelGGL(container_scan_kernel<true>, dim3(1), dim3(kContainerScanThreads), 0, s, sc);
    rc = launch_check("container_scan_kernel");
    if (rc || p.copy_blocks == 0) return rc;
    CopyArgs cp;
    cp.off = sc.off; cp.words = sc.words; cp.ptr = st.ptr; cp.len = st.len; cp.blob = blob; cp.total = total;
    cp.n = p.streams; cp.header_bytes = p.header_bytes; cp.nwords = p.copy_words; cp.blob_words = 0;
    hipLaunchKernelGGL(container_pack_copy_kernel, dim3((unsigned)p.copy_blocks), dim3(kContainerCopyThreads), 0, s, cp);
    return launch_check("container_pack_copy_kernel");
}

extern "C" int cgic_container_unpack(const uint8_t *host_blob, const uint8_t *blob, int64_t bytes, const cgic_container_group *groups, int G,
                                     const cgic_container_entry *entries, int64_t E, void *workspace, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_container_unpack");
    int sets[7];
    for (int m = 0; m < 7; ++m) sets[m] = cgic_mode_streams(m);
    ContainerPlan p;
    ContainerWhy why;
    const int rc0 = container_unpack_plan(host_blob, bytes, groups, G, entries, E, sets, &p, &why);
    CGIC_REQUIRE(rc0 == CGIC_OK, rc0, "container_unpack: %s", container_why_text(why));
    if (E == 0) return CGIC_OK;
    CGIC_REQUIRE(blob && workspace, CGIC_ERR_INVALID, "container_unpack: NULL device blob or workspace");
    CGIC_REQUIRE((uintptr_t)blob % 16 == 0 && (uintptr_t)workspace % 16 == 0, CGIC_ERR_INVALID,
                 "container_unpack: the device blob and the workspace must be 16-byte aligned");
    StageArgs st;
    int rc = fill_groups(&st, groups, G, "container_unpack");
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    unsigned char *ws = (unsigned char *)workspace;
    st.blob = (unsigned char *)blob; st.capacity = bytes;
    st.ptr = (int64_t *)(ws + p.ws.ptr); st.len = (int32_t *)(ws + p.ws.len);
    rc = launch_stage<false>(&st, entries, E, p, s);
    if (rc) return rc;
    ScanArgs sc;
    sc.len = st.len; sc.off = (int64_t *)(ws + p.ws.off); sc.words = (int64_t *)(ws + p.ws.words);
    sc.n = p.streams; sc.header_bytes = p.header_bytes; sc.capacity = bytes; sc.entries = E; sc.blob = nullptr; sc.total = nullptr;
    hipLaunchKernelGGL(container_scan_kernel<false>, dim3(1), dim3(kContainerScanThreads), 0, s, sc);
    rc = launch_check("container_scan_kernel");
    if (rc || p.copy_blocks == 0) return rc;
    CopyArgs cp;
    cp.off = sc.off; cp.words = sc.words; cp.ptr = st.ptr; cp.len = st.len; cp.blob = (unsigned char *)blob; cp.total = nullptr;
    cp.n = p.streams; cp.header_bytes = p.header_bytes; cp.nwords = p.copy_words; cp.blob_words = (bytes + 15) / 16;
    hipLaunchKernelGGL(container_unpack_copy_kernel, dim3((unsigned)p.copy_blocks), dim3(kContainerCopyThreads), 0, s, cp);
    return launch_check("container_unpack_copy_kernel");
}
