// cgic_ema.hip -- LitEma (CGIC/models/ema.py:25-76) over all tensors of a module in one launch: cgic_ema_plan_*, cgic_ema_update,
// cgic_ema_copy (include/cgic_hip.h, ABI 22).  The work list and every check come from cgic_ema_plan.h; this file uploads the two
// tables and launches what the plan says.  Streaming kernels: plain vector loads and stores, no LDS, no atomics; the only word two
// launches share is the plan's omd float, written by the one-thread prologue and read by every workgroup of the launch behind it.
#include <memory>
#include <new>

#include "cgic_common.h"
#include "cgic_ema_plan.h"

using namespace cgic;

struct cgic_ema_plan {
    EmaPlan plan;
    unsigned char *dev;          // [plan.table_bytes]: omd | entries | chunks
    int device;
};

namespace {

// The tables hold addresses as integers; a pointer made from one is generic, and its accesses would be flat_load / flat_store.
// These are pointers into global memory by the entry points' contract: saying so gives global_load_dwordx4 / global_store_dwordx4.
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) v4f gv4f;

// shadow - (omd * (shadow - param)): three roundings, never contracted whatever the flags
__device__ __forceinline__ float ema_step(float s, float p, float omd) { return __fsub_rn(s, __fmul_rn(omd, __fsub_rn(s, p))); }
__device__ __forceinline__ v4f ema_step4(v4f s, v4f p, float omd)
{
    v4f r;
    r.x = ema_step(s.x, p.x, omd); r.y = ema_step(s.y, p.y, omd); r.z = ema_step(s.z, p.z, omd); r.w = ema_step(s.w, p.w, omd);
    return r;
}

__global__ void ema_prologue_kernel(const float *decay, int32_t *num_updates, float *omd)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int32_t n = num_updates ? *num_updates : -1;
    if (num_updates && n >= 0) *num_updates = ema_next_count(n);
    *omd = ema_one_minus_decay(*decay, n, num_updates != nullptr);
}

constexpr int kVecPerLane = (int)(kEmaChunk / 4 / kEmaThreads);          // float4 per lane of a full chunk
static_assert(kEmaChunk % (4 * kEmaThreads) == 0, "a full chunk is a whole number of float4 per lane");

__global__ __launch_bounds__(kEmaThreads) void ema_update_kernel(const EmaEntry *entries, const EmaChunk *chunks, int nchunks, const float *omd_p)
{
    const float omd = *omd_p;
    const int t = (int)threadIdx.x;
    for (int c = (int)blockIdx.x; c < nchunks; c += (int)gridDim.x) {
        const EmaChunk ch = chunks[c];
        const EmaEntry e = entries[ch.entry];
        const uintptr_t sa = e.shadow + (uintptr_t)ch.off * sizeof(float), pa = e.param + (uintptr_t)ch.off * sizeof(float);
        gfloat *s = (gfloat *)sa;
        const gfloat *p = (const gfloat *)pa;
        const int len = ch.len;
        int done = 0;
        if (ema_both_16(sa, pa)) {
            gv4f *s4 = (gv4f *)sa;
            const gv4f *p4 = (const gv4f *)pa;
            const int n4 = len >> 2;
            if (n4 == kVecPerLane * kEmaThreads) {                          // a full chunk: every load in flight before the first store
                v4f a[kVecPerLane], b[kVecPerLane];
#pragma unroll
                for (int k = 0; k < kVecPerLane; ++k) { a[k] = s4[t + k * kEmaThreads]; b[k] = p4[t + k * kEmaThreads]; }
#pragma unroll
                for (int k = 0; k < kVecPerLane; ++k) s4[t + k * kEmaThreads] = ema_step4(a[k], b[k], omd);
            } else {
                for (int i = t; i < n4; i += kEmaThreads) s4[i] = ema_step4(s4[i], p4[i], omd);
            }
            done = n4 << 2;
        }
        for (int i = done + t; i < len; i += kEmaThreads) s[i] = ema_step(s[i], p[i], omd);
    }
}

// direction EMA_COPY_TO: param = shadow; EMA_STORE: stash = param; EMA_RESTORE: param = stash
__global__ __launch_bounds__(kEmaThreads) void ema_copy_kernel(const EmaEntry *entries, const EmaChunk *chunks, int nchunks, int direction, float *stash)
{
    const int t = (int)threadIdx.x;
    for (int c = (int)blockIdx.x; c < nchunks; c += (int)gridDim.x) {
        const EmaChunk ch = chunks[c];
        const EmaEntry e = entries[ch.entry];
        const uintptr_t param = e.param + (uintptr_t)ch.off * sizeof(float), shadow = e.shadow + (uintptr_t)ch.off * sizeof(float);
        const uintptr_t kept = (uintptr_t)stash + (uintptr_t)(e.stash_off + ch.off) * sizeof(float);
        const uintptr_t sa = direction == EMA_COPY_TO ? shadow : direction == EMA_STORE ? param : kept;
        const uintptr_t da = direction == EMA_STORE ? kept : param;
        const gfloat *src = (const gfloat *)sa;
        gfloat *dst = (gfloat *)da;
        const int len = ch.len;
        int done = 0;
        if (ema_both_16(sa, da)) {
            const gv4f *s4 = (const gv4f *)sa;
            gv4f *d4 = (gv4f *)da;
            const int n4 = len >> 2;
            if (n4 == kVecPerLane * kEmaThreads) {
                v4f a[kVecPerLane];
#pragma unroll
                for (int k = 0; k < kVecPerLane; ++k) a[k] = s4[t + k * kEmaThreads];
#pragma unroll
                for (int k = 0; k < kVecPerLane; ++k) d4[t + k * kEmaThreads] = a[k];
            } else {
                for (int i = t; i < n4; i += kEmaThreads) d4[i] = s4[i];
            }
            done = n4 << 2;
        }
        for (int i = done + t; i < len; i += kEmaThreads) dst[i] = src[i];
    }
}

}  // namespace

// the body of cgic_ema_plan_create; its containers may throw std::bad_alloc, which the entry point turns into CGIC_ERR_NOMEM
static int ema_plan_build(const cgic_ema_entry *entries, int n, std::unique_ptr<cgic_ema_plan> &p)
{
    static_assert(sizeof(cgic_ema_entry) == sizeof(EmaIn) && sizeof(float *) == sizeof(uintptr_t), "cgic_ema_entry is read as EmaIn");
    std::vector<EmaIn> in((size_t)(n > 0 && entries ? n : 0));
    for (size_t i = 0; i < in.size(); ++i) in[i] = EmaIn{(uintptr_t)entries[i].shadow, (uintptr_t)entries[i].param, entries[i].n};
    p.reset(new cgic_ema_plan{});
    const char *why = "";
    const int rc = ema_plan(entries ? in.data() : nullptr, (int64_t)n, &p->plan, &why);
    if (rc != CGIC_OK) {
        set_error("%s", why);
        return rc;
    }
    std::vector<unsigned char> host(p->plan.table_bytes, 0);
    if (!p->plan.entries.empty()) memcpy(host.data() + p->plan.entries_at, p->plan.entries.data(), sizeof(EmaEntry) * p->plan.entries.size());
    if (!p->plan.chunks.empty()) memcpy(host.data() + p->plan.chunks_at, p->plan.chunks.data(), sizeof(EmaChunk) * p->plan.chunks.size());
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc((void **)&p->dev, host.size());
    if (e == hipSuccess) e = hipMemcpy(p->dev, host.data(), host.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "cgic_ema_plan_create: upload of the tables", __FILE__, __LINE__);
    // (the host copy of the chunk table is not needed again: the launches read the device one)
    std::vector<EmaChunk>().swap(p->plan.chunks);
    return CGIC_OK;
}

extern "C" int cgic_ema_plan_create(const cgic_ema_entry *entries, int n, cgic_ema_plan **out)
{
    CGIC_NOT_IN_GROUP("cgic_ema_plan_create");
    CGIC_REQUIRE(out != nullptr, CGIC_ERR_INVALID, "cgic_ema_plan_create: NULL out");
    *out = nullptr;
    std::unique_ptr<cgic_ema_plan> p;
    int rc;
    try {
        rc = ema_plan_build(entries, n, p);
    } catch (const std::bad_alloc &) {
        set_error("cgic_ema_plan_create: out of host memory for the tables of %d entries", n);
        rc = CGIC_ERR_NOMEM;
    }
    if (rc != CGIC_OK) {
        if (p && p->dev) (void)hipFree(p->dev);
        return rc;
    }
    *out = p.release();
    return CGIC_OK;
}

extern "C" void cgic_ema_plan_destroy(cgic_ema_plan *p)
{
    if (!p) return;
    if (p->dev) (void)hipFree(p->dev);
    delete p;
}

extern "C" int cgic_ema_plan_info(const cgic_ema_plan *p, int64_t *out)
{
    CGIC_REQUIRE(p != nullptr && out != nullptr, CGIC_ERR_INVALID, "cgic_ema_plan_info: NULL argument");
    const EmaPlan &pl = p->plan;
    const int64_t nchunks = (int64_t)((pl.table_bytes - pl.chunks_at) / sizeof(EmaChunk));
    const int64_t v[8] = {(int64_t)pl.entries.size(), pl.elements, nchunks, kEmaChunk, pl.chunks16, (int64_t)pl.grid, pl.stash_elements, pl.chunks16_stash};
    memcpy(out, v, sizeof(v));
    return CGIC_OK;
}

static int ema_tables(const cgic_ema_plan *p, const char *who, const EmaEntry **entries, const EmaChunk **chunks, int *nchunks)
{
    int dev = -1;
    CGIC_HIP_TRY(hipGetDevice(&dev));
    CGIC_REQUIRE(dev == p->device, CGIC_ERR_INVALID, "%s: the plan was made on device %d, the current device is %d", who, p->device, dev);
    *entries = reinterpret_cast<const EmaEntry *>(p->dev + p->plan.entries_at);
    *chunks = reinterpret_cast<const EmaChunk *>(p->dev + p->plan.chunks_at);
    *nchunks = (int)((p->plan.table_bytes - p->plan.chunks_at) / sizeof(EmaChunk));
    return CGIC_OK;
}

extern "C" int cgic_ema_update(const cgic_ema_plan *p, const float *decay, int32_t *num_updates, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_ema_update");
    CGIC_REQUIRE(p != nullptr, CGIC_ERR_INVALID, "cgic_ema_update: NULL plan");
    CGIC_REQUIRE(decay != nullptr, CGIC_ERR_INVALID, "cgic_ema_update: NULL decay");
    CGIC_REQUIRE(((uintptr_t)decay | (uintptr_t)num_updates) % 4 == 0, CGIC_ERR_INVALID, "cgic_ema_update: decay or num_updates is not aligned to its 4-byte element");
    const EmaEntry *entries;
    const EmaChunk *chunks;
    int nchunks;
    const int rc = ema_tables(p, "cgic_ema_update", &entries, &chunks, &nchunks);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    float *omd = reinterpret_cast<float *>(p->dev);
    hipLaunchKernelGGL(ema_prologue_kernel, dim3(1), dim3(1), 0, s, decay, num_updates, omd);
    const int rc1 = launch_check("ema_prologue_kernel");
    if (rc1 || p->plan.grid == 0) return rc1;
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)p->plan.grid), dim3(kEmaThreads), 0, s, entries, chunks, nchunks, (const float *)omd);
    return launch_check("ema_update_kernel");
}

extern "C" int cgic_ema_copy(const cgic_ema_plan *p, int direction, float *stash, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_ema_copy");
    CGIC_REQUIRE(p != nullptr, CGIC_ERR_INVALID, "cgic_ema_copy: NULL plan");
    CGIC_REQUIRE(direction == EMA_COPY_TO || direction == EMA_STORE || direction == EMA_RESTORE, CGIC_ERR_INVALID,
                 "cgic_ema_copy: direction %d (0: param = shadow, 1: stash = param, 2: param = stash)", direction);
    if (direction == EMA_COPY_TO) stash = nullptr;
    else if (p->plan.grid > 0) {
        CGIC_REQUIRE(stash != nullptr, CGIC_ERR_INVALID, "cgic_ema_copy: direction %d needs the stash", direction);
        CGIC_REQUIRE((uintptr_t)stash % 16 == 0, CGIC_ERR_INVALID, "cgic_ema_copy: the stash is not 16-byte aligned");
    }
    const EmaEntry *entries;
    const EmaChunk *chunks;
    int nchunks;
    const int rc = ema_tables(p, "cgic_ema_copy", &entries, &chunks, &nchunks);
    if (rc || p->plan.grid == 0) return rc;
    hipLaunchKernelGGL(ema_copy_kernel, dim3((unsigned)p->plan.grid), dim3(kEmaThreads), 0, (hipStream_t)stream, entries, chunks, nchunks, direction, stash);
    return launch_check("ema_copy_kernel");
}
