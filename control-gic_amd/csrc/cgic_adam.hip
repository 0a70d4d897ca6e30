// cgic_adam.hip -- gradient clipping by value, torch.optim.Adam's step and LitEma's update over all tensors of a parameter group in
// ONE pass: cgic_adam_plan_*, cgic_adam_step (include/cgic_hip.h, ABI 23).  The work list, every check and the arithmetic come from
// cgic_adam_plan.h; this file uploads the tables, keeps the table of gradient addresses current and launches what the plan says:
// a one-workgroup prologue (step counts, bias corrections, the EMA groups' counters and decays) and the streaming body, which reads
// g, p, m, v, s and writes p, m, v, s -- plain vector loads and stores, no LDS, no atomics.  The words two launches share are the
// plan's scalars and omd tables, written by the prologue and read by every workgroup of the launch behind it.
#include <memory>
#include <new>

#include "cgic_common.h"
#include "cgic_adam_plan.h"

using namespace cgic;

namespace {

constexpr int kAdamSlots = 4;            // pinned staging slots of the gradient table: a changed table waits only when all are in flight
struct AdamSlot {
    void *host;
    hipEvent_t done;
    bool used;
};

}  // namespace

struct cgic_adam_plan {
    AdamPlan plan;
    unsigned char *dev;                  // [plan.table_bytes]
    int device;
    int64_t nchunks;
    std::vector<uintptr_t> last;         // the gradient table the device holds
    bool have_last;
    AdamSlot slot[kAdamSlots];
    int next_slot;
    int64_t uploads, upload_waits, steps;
};

namespace {

typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) v4f gv4f;

constexpr int kPrologueThreads = 256;

__global__ __launch_bounds__(kPrologueThreads) void adam_prologue_kernel(int nentries, int ngroups, const uintptr_t *grads, float *steps, AdamScalars *scalars,
                                                                         const AdamGroup *groups, float *omd, double lr, const float *lr_dev, double beta1,
                                                                         double beta2)
{
    if (blockIdx.x != 0) return;
    const int t = (int)threadIdx.x;
    if (lr_dev) lr = (double)*lr_dev;
    for (int i = t; i < nentries; i += kPrologueThreads) {
        if (!grads[i]) continue;                                             // no gradient this step: the count stays (torch skips grad is None)
        const float s = steps[i] + 1.0f;
        steps[i] = s;
        scalars[i] = adam_scalars(s, lr, beta1, beta2);
    }
    if (t < ngroups) {
        const AdamGroup g = groups[t];
        int32_t *count = (int32_t *)g.num_updates;
        const int32_t n = count ? *count : -1;
        if (count && n >= 0) *count = ema_next_count(n);
        omd[t] = ema_one_minus_decay(*(const float *)g.decay, n, count != nullptr);
    }
}

constexpr int kVecPerLane = (int)(kEmaChunk / 4 / kEmaThreads);          // float4 of each operand per lane of a full chunk
static_assert(kEmaChunk % (4 * kEmaThreads) == 0, "a full chunk is a whole number of float4 per lane");

template <bool S>
__device__ __forceinline__ void adam_vec(v4f g, v4f &p, v4f &m, v4f &v, v4f &s, const AdamConsts &k, AdamScalars sc, float omd)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adam_element(g[j], &pj, &mj, &vj, k, sc.step_size, sc.bc2_sqrt);
        p[j] = pj; m[j] = mj; v[j] = vj;
        if (S) s[j] = adam_shadow(s[j], pj, omd);
    }
}

// one chunk with a gradient.  S: the entry has a shadow
template <bool S>
__device__ __forceinline__ void adam_chunk(uintptr_t pa, uintptr_t ma, uintptr_t va, uintptr_t ga, uintptr_t sa, int len, int t, const AdamConsts &k,
                                           AdamScalars sc, float omd)
{
    int done = 0;
    if (adam_all_16(pa, ma, va, ga, S ? sa : 0)) {
        gv4f *p4 = (gv4f *)pa, *m4 = (gv4f *)ma, *v4 = (gv4f *)va, *s4 = (gv4f *)sa;
        const gv4f *g4 = (const gv4f *)ga;
        const int n4 = len >> 2;
        if (n4 == kVecPerLane * kEmaThreads) {                          // a full chunk: every load in flight before the first store
            v4f G[kVecPerLane], P[kVecPerLane], M[kVecPerLane], V[kVecPerLane], Sh[kVecPerLane];
#pragma unroll
            for (int j = 0; j < kVecPerLane; ++j) {
                const int i = t + j * kEmaThreads;
                G[j] = g4[i]; P[j] = p4[i]; M[j] = m4[i]; V[j] = v4[i];
                if (S) Sh[j] = s4[i];
            }
#pragma unroll
            for (int j = 0; j < kVecPerLane; ++j) {
                const int i = t + j * kEmaThreads;
                adam_vec<S>(G[j], P[j], M[j], V[j], Sh[j], k, sc, omd);
                p4[i] = P[j]; m4[i] = M[j]; v4[i] = V[j];
                if (S) s4[i] = Sh[j];
            }
        } else {
            for (int i = t; i < n4; i += kEmaThreads) {
                v4f P = p4[i], M = m4[i], V = v4[i], Sh;
                if (S) Sh = s4[i];
                adam_vec<S>(g4[i], P, M, V, Sh, k, sc, omd);
                p4[i] = P; m4[i] = M; v4[i] = V;
                if (S) s4[i] = Sh;
            }
        }
        done = n4 << 2;
    }
    gfloat *p = (gfloat *)pa, *m = (gfloat *)ma, *v = (gfloat *)va, *s = (gfloat *)sa;
    const gfloat *g = (const gfloat *)ga;
    for (int i = done + t; i < len; i += kEmaThreads) {
        float pj = p[i], mj = m[i], vj = v[i];
        adam_element(g[i], &pj, &mj, &vj, k, sc.step_size, sc.bc2_sqrt);
        p[i] = pj; m[i] = mj; v[i] = vj;
        if (S) s[i] = adam_shadow(s[i], pj, omd);
    }
}

// one chunk without a gradient but with a shadow: LitEma's update alone
__device__ __forceinline__ void adam_ema_chunk(uintptr_t pa, uintptr_t sa, int len, int t, float omd)
{
    int done = 0;
    if (adam_all_16(pa, sa, 0, 0, 0)) {
        gv4f *s4 = (gv4f *)sa;
        const gv4f *p4 = (const gv4f *)pa;
        const int n4 = len >> 2;
        for (int i = t; i < n4; i += kEmaThreads) {
            v4f s = s4[i];
            const v4f p = p4[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = adam_shadow(s[j], p[j], omd);
            s4[i] = s;
        }
        done = n4 << 2;
    }
    gfloat *s = (gfloat *)sa;
    const gfloat *p = (const gfloat *)pa;
    for (int i = done + t; i < len; i += kEmaThreads) s[i] = adam_shadow(s[i], p[i], omd);
}

__global__ __launch_bounds__(kEmaThreads) void adam_step_kernel(const AdamEntry *entries, const EmaChunk *chunks, int nchunks, const uintptr_t *grads,
                                                                const AdamScalars *scalars, const float *omds, AdamConsts k)
{
    const int t = (int)threadIdx.x;
    for (int c = (int)blockIdx.x; c < nchunks; c += (int)gridDim.x) {
        const EmaChunk ch = chunks[c];
        const AdamEntry e = entries[ch.entry];
        const uintptr_t grad = grads[ch.entry];
        const bool shadowed = e.ema_group >= 0;
        if (!grad && !shadowed) continue;                                    // neither a gradient nor a shadow: not touched
        const uintptr_t off = (uintptr_t)ch.off * sizeof(float);
        const float omd = shadowed ? omds[e.ema_group] : 0.0f;
        if (!grad) {
            adam_ema_chunk(e.param + off, e.shadow + off, ch.len, t, omd);
            continue;
        }
        const AdamScalars sc = scalars[ch.entry];
        if (shadowed) adam_chunk<true>(e.param + off, e.exp_avg + off, e.exp_avg_sq + off, grad + off, e.shadow + off, ch.len, t, k, sc, omd);
        else adam_chunk<false>(e.param + off, e.exp_avg + off, e.exp_avg_sq + off, grad + off, 0, ch.len, t, k, sc, omd);
    }
}

void adam_release(cgic_adam_plan *p)
{
    if (p->dev) (void)hipFree(p->dev);
    for (AdamSlot &s : p->slot) {
        if (s.host) (void)hipHostFree(s.host);
        if (s.done) (void)hipEventDestroy(s.done);
    }
}

}  // namespace

// the body of cgic_adam_plan_create; its containers may throw std::bad_alloc, which the entry point turns into CGIC_ERR_NOMEM
static int adam_plan_build(const cgic_adam_entry *entries, int n, const cgic_adam_ema_group *groups, int ngroups, float *steps,
                           std::unique_ptr<cgic_adam_plan> &p)
{
    static_assert(sizeof(cgic_adam_entry) == sizeof(AdamIn) && sizeof(cgic_adam_ema_group) == sizeof(AdamGroup) && sizeof(float *) == sizeof(uintptr_t),
                  "cgic_adam_entry is read as AdamIn, cgic_adam_ema_group as AdamGroup");
    std::vector<AdamIn> in((size_t)(n > 0 && entries ? n : 0));
    for (size_t i = 0; i < in.size(); ++i)
        in[i] = AdamIn{(uintptr_t)entries[i].param, (uintptr_t)entries[i].exp_avg, (uintptr_t)entries[i].exp_avg_sq, (uintptr_t)entries[i].shadow,
                       entries[i].n, entries[i].ema_group, 0};
    std::vector<AdamGroup> gr((size_t)(ngroups > 0 && ngroups <= kAdamGroupsMax && groups ? ngroups : 0));
    for (size_t i = 0; i < gr.size(); ++i) gr[i] = AdamGroup{(uintptr_t)groups[i].decay, (uintptr_t)groups[i].num_updates};
    p.reset(new cgic_adam_plan{});
    const char *why = "";
    const int rc = adam_plan(entries ? in.data() : nullptr, (int64_t)n, groups ? gr.data() : nullptr, (int64_t)ngroups, (uintptr_t)steps, &p->plan, &why);
    if (rc != CGIC_OK) {
        set_error("%s", why);
        return rc;
    }
    const AdamPlan &pl = p->plan;
    std::vector<unsigned char> host(pl.table_bytes, 0);
    if (!pl.groups.empty()) memcpy(host.data() + pl.groups_at, pl.groups.data(), sizeof(AdamGroup) * pl.groups.size());
    if (!pl.entries.empty()) memcpy(host.data() + pl.entries_at, pl.entries.data(), sizeof(AdamEntry) * pl.entries.size());
    if (!pl.chunks.empty()) memcpy(host.data() + pl.chunks_at, pl.chunks.data(), sizeof(EmaChunk) * pl.chunks.size());
    p->nchunks = (int64_t)pl.chunks.size();
    p->last.assign(pl.entries.size(), 0);                                   // (the uploaded table holds no gradient: what the zeros say)
    p->have_last = false;
    hipError_t e = hipGetDevice(&p->device);
    if (e == hipSuccess) e = hipMalloc((void **)&p->dev, host.size());
    if (e == hipSuccess) e = hipMemcpy(p->dev, host.data(), host.size(), hipMemcpyHostToDevice);
    const size_t slot_bytes = sizeof(uintptr_t) * (pl.entries.empty() ? 1 : pl.entries.size());
    for (int i = 0; i < kAdamSlots && e == hipSuccess; ++i) {
        e = hipHostMalloc(&p->slot[i].host, slot_bytes, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&p->slot[i].done, hipEventDisableTiming);
    }
    if (e != hipSuccess) return hip_fail(e, "cgic_adam_plan_create: upload of the tables", __FILE__, __LINE__);
    // (the host copy of the chunk table is not needed again: the launches read the device one)
    std::vector<EmaChunk>().swap(p->plan.chunks);
    return CGIC_OK;
}

extern "C" int cgic_adam_plan_create(const cgic_adam_entry *entries, int n, const cgic_adam_ema_group *groups, int ngroups, float *steps,
                                     cgic_adam_plan **out)
{
    CGIC_NOT_IN_GROUP("cgic_adam_plan_create");
    CGIC_REQUIRE(out != nullptr, CGIC_ERR_INVALID, "cgic_adam_plan_create: NULL out");
    *out = nullptr;
    std::unique_ptr<cgic_adam_plan> p;
    int rc;
    try {
        rc = adam_plan_build(entries, n, groups, ngroups, steps, p);
    } catch (const std::bad_alloc &) {
        set_error("cgic_adam_plan_create: out of host memory for the tables of %d entries", n);
        rc = CGIC_ERR_NOMEM;
    }
    if (rc != CGIC_OK) {
        if (p) adam_release(p.get());
        return rc;
    }
    *out = p.release();
    return CGIC_OK;
}

extern "C" void cgic_adam_plan_destroy(cgic_adam_plan *p)
{
    if (!p) return;
    adam_release(p);
    delete p;
}

extern "C" int cgic_adam_plan_info(const cgic_adam_plan *p, int64_t *out)
{
    CGIC_REQUIRE(p != nullptr && out != nullptr, CGIC_ERR_INVALID, "cgic_adam_plan_info: NULL argument");
    const AdamPlan &pl = p->plan;
    const int64_t v[12] = {(int64_t)pl.entries.size(), pl.elements, p->nchunks, kEmaChunk, pl.chunks16, (int64_t)pl.grid, (int64_t)pl.groups.size(),
                           pl.shadowed, p->uploads, p->upload_waits, (int64_t)pl.table_bytes, p->steps};
    memcpy(out, v, sizeof(v));
    return CGIC_OK;
}

// the new gradient table goes up in stream order from a pinned slot nobody reads any more
static int adam_upload_grads(cgic_adam_plan *p, const uintptr_t *table, hipStream_t s)
{
    int pick = -1;
    for (int k = 0; k < kAdamSlots && pick < 0; ++k) {
        const int i = (p->next_slot + k) % kAdamSlots;
        if (!p->slot[i].used) pick = i;
        else {
            const hipError_t q = hipEventQuery(p->slot[i].done);
            if (q == hipSuccess) pick = i;
            else if (q != hipErrorNotReady) return hip_fail(q, "cgic_adam_step: query of a staging slot", __FILE__, __LINE__);
        }
    }
    if (pick < 0) {                                                          // every slot is still in flight: wait for the oldest
        pick = p->next_slot;
        CGIC_HIP_TRY(hipEventSynchronize(p->slot[pick].done));
        ++p->upload_waits;
    }
    const size_t bytes = sizeof(uintptr_t) * p->last.size();
    memcpy(p->slot[pick].host, table, bytes);
    CGIC_HIP_TRY(hipMemcpyAsync(p->dev + p->plan.grads_at, p->slot[pick].host, bytes, hipMemcpyHostToDevice, s));
    CGIC_HIP_TRY(hipEventRecord(p->slot[pick].done, s));
    p->slot[pick].used = true;
    p->next_slot = (pick + 1) % kAdamSlots;
    ++p->uploads;
    return CGIC_OK;
}

extern "C" int cgic_adam_step(cgic_adam_plan *p, const float *const *grads, const cgic_adam_hyper *h, cgic_stream_t stream)
{
    CGIC_NOT_IN_GROUP("cgic_adam_step");
    CGIC_REQUIRE(p != nullptr, CGIC_ERR_INVALID, "cgic_adam_step: NULL plan");
    CGIC_REQUIRE(h != nullptr, CGIC_ERR_INVALID, "cgic_adam_step: NULL hyperparameters");
    const size_t n = p->plan.entries.size();
    CGIC_REQUIRE(n == 0 || grads != nullptr, CGIC_ERR_INVALID, "cgic_adam_step: NULL gradient list with %zu entries", n);
    CGIC_REQUIRE(h->lr_dev != nullptr || h->lr >= 0.0, CGIC_ERR_INVALID, "cgic_adam_step: lr %g (torch: Invalid learning rate)", h->lr);
    CGIC_REQUIRE((uintptr_t)h->lr_dev % 4 == 0, CGIC_ERR_INVALID, "cgic_adam_step: lr_dev is not aligned to its 4-byte element");
    CGIC_REQUIRE(h->beta1 >= 0.0 && h->beta1 < 1.0 && h->beta2 >= 0.0 && h->beta2 < 1.0, CGIC_ERR_INVALID,
                 "cgic_adam_step: betas (%g, %g); each must be in [0, 1)", h->beta1, h->beta2);
    CGIC_REQUIRE(h->eps >= 0.0, CGIC_ERR_INVALID, "cgic_adam_step: eps %g (torch: Invalid epsilon value)", h->eps);
    CGIC_REQUIRE(h->weight_decay >= 0.0, CGIC_ERR_INVALID, "cgic_adam_step: weight_decay %g (torch: Invalid weight_decay value)", h->weight_decay);
    CGIC_REQUIRE(!h->clip || h->clip_value >= 0.0, CGIC_ERR_INVALID, "cgic_adam_step: clip_value %g; a bound is not negative and not NaN", h->clip_value);
    int dev = -1;
    CGIC_HIP_TRY(hipGetDevice(&dev));
    CGIC_REQUIRE(dev == p->device, CGIC_ERR_INVALID, "cgic_adam_step: the plan was made on device %d, the current device is %d", p->device, dev);
    bool changed = !p->have_last;
    for (size_t i = 0; i < n; ++i) {
        const uintptr_t g = (uintptr_t)grads[i];
        CGIC_REQUIRE(g % 4 == 0, CGIC_ERR_INVALID, "cgic_adam_step: the gradient of entry %zu is not aligned to its 4-byte element", i);
        changed = changed || g != p->last[i];
    }
    hipStream_t s = (hipStream_t)stream;
    if (changed && n > 0) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        CGIC_HIP_TRY(hipStreamIsCapturing(s, &cap));
        CGIC_REQUIRE(cap == hipStreamCaptureStatusNone, CGIC_ERR_INVALID,
                     "cgic_adam_step: the gradient addresses changed while the stream is capturing (a replay would read the captured table: run one "
                     "step eagerly on the gradient buffers the capture will use)");
        const int rc = adam_upload_grads(p, reinterpret_cast<const uintptr_t *>(grads), s);
        if (rc) {
            p->have_last = false;
            return rc;
        }
        memcpy(p->last.data(), grads, sizeof(uintptr_t) * n);
    }
    p->have_last = true;
    const AdamPlan &pl = p->plan;
    const int ngroups = (int)pl.groups.size();
    if (n == 0 && ngroups == 0) return CGIC_OK;
    const uintptr_t *dgrads = reinterpret_cast<const uintptr_t *>(p->dev + pl.grads_at);
    AdamScalars *scalars = reinterpret_cast<AdamScalars *>(p->dev + pl.scalars_at);
    float *omd = reinterpret_cast<float *>(p->dev);
    hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(kPrologueThreads), 0, s, (int)n, ngroups, dgrads, (float *)pl.steps, scalars,
                       reinterpret_cast<const AdamGroup *>(p->dev + pl.groups_at), omd, h->lr, h->lr_dev, h->beta1, h->beta2);
    const int rc1 = launch_check("adam_prologue_kernel");
    ++p->steps;
    if (rc1 || pl.grid == 0) return rc1;
    const AdamConsts k = adam_consts(h->beta1, h->beta2, h->eps, h->weight_decay, h->clip_value, h->clip != 0);
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)pl.grid), dim3(kEmaThreads), 0, s, reinterpret_cast<const AdamEntry *>(p->dev + pl.entries_at),
                       reinterpret_cast<const EmaChunk *>(p->dev + pl.chunks_at), (int)p->nchunks, dgrads, (const AdamScalars *)scalars, (const float *)omd, k);
    return launch_check("adam_step_kernel");
}
