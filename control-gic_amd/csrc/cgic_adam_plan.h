// cgic_adam_plan.h -- what the two launches of a cgic_adam_plan do, decided when the plan is made, and the arithmetic they run: every
// check of the entries, the chunk table, which chunks can move 16 bytes per lane, the grid, the layout of the device tables, the
// scalar rule of the prologue (adam_scalars) and the per-element chain of the body (adam_element, adam_shadow).  Plain C++17 on
// purpose, like cgic_ema_plan.h (no HIP include, no stream; pointers are plain addresses): adam_plan() is a pure function of the
// entry list, and the two arithmetic functions are the text host and device share, so all of it can be exercised without a GPU
// (tests/host/adam_plan_main.cpp) and compared bit for bit with tests/adam_ref.py.
//
// The work list is the EMA plan's (cgic_ema_plan.h): chunks of kEmaChunk elements of one tensor, grid = min(chunks, kEmaGridMax), a
// chunk 16-byte aligned exactly where its tensor is.  An entry has up to five operands -- param, exp_avg, exp_avg_sq, the gradient
// of the step and an optional shadow --; the gradient's address is new at every step and lives in a table of its own that
// cgic_adam_step uploads when it changed, so the kernel decides the 16-byte path from the addresses it finds (adam_all_16) and the
// plan counts the chunks whose STATE side allows it.
//
// One allocation:  omd[kAdamGroupsMax] | groups | entries | chunks | scalars[entries] | grads[entries]
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "cgic_ema_plan.h"

#define CGIC_ADAM_HD CGIC_EMA_HD

namespace cgic {

constexpr int kAdamGroupsMax = 16;
constexpr size_t kAdamHeadBytes = sizeof(float) * kAdamGroupsMax;              // one omd per EMA group

struct AdamIn { uintptr_t param, exp_avg, exp_avg_sq, shadow; int64_t n; int32_t ema_group, reserved; };    // (the layout of cgic_adam_entry)
typedef AdamIn AdamEntry;                                                       // 48 bytes, as the kernels read it
struct AdamGroup { uintptr_t decay, num_updates; };                             // (the layout of cgic_adam_ema_group) 16 bytes
struct AdamScalars { float step_size, bc2_sqrt; };                              // per entry, written by the prologue
static_assert(sizeof(AdamEntry) == 48 && sizeof(AdamGroup) == 16 && sizeof(AdamScalars) == 8, "the device tables are read as these structs");

// the hyperparameters of one step as the body reads them: every one rounded to fp32 ONCE, from the doubles torch holds as Python floats
struct AdamConsts {
    float clip, wd, w1, one_minus_w1, beta2, w2, eps;
    int32_t do_clip, do_wd, lerp_low;
};

CGIC_ADAM_HD inline bool adam_all_16(uintptr_t a, uintptr_t b, uintptr_t c, uintptr_t d, uintptr_t e) { return ((a | b | c | d | e) & 15) == 0; }

// ---- the arithmetic.  No operation here may be fused with another: contraction is off for these functions whatever the flags.
#if defined(__clang__)
#define CGIC_ADAM_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CGIC_ADAM_NO_CONTRACT
#if defined(__GNUC__)
#pragma GCC push_options
#pragma GCC optimize("fp-contract=off")
#endif
#endif

inline AdamConsts adam_consts(double beta1, double beta2, double eps, double weight_decay, double clip_value, bool clip)
{
    CGIC_ADAM_NO_CONTRACT
    AdamConsts k;
    k.clip = (float)clip_value;
    k.wd = (float)weight_decay;
    k.w1 = (float)(1.0 - beta1);                        // lerp_'s weight: 1 - beta1 in double, handed over as one float
    k.one_minus_w1 = 1.0f - k.w1;                       // (the high branch of lerp: 1 - weight in fp32)
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.do_clip = clip ? 1 : 0;
    k.do_wd = weight_decay != 0.0 ? 1 : 0;
    k.lerp_low = fabsf(k.w1) < 0.5f ? 1 : 0;
    return k;
}

// the exponent of beta^step: the fp32 step count as an integer (a count is one; anything else is cut off, NaN and negatives are 0)
CGIC_ADAM_HD inline uint32_t adam_step_exponent(float step)
{
    return step >= 4294967040.0f ? 4294967040u : step >= 1.0f ? (uint32_t)step : 0u;
}

// beta^t in float64 by square-and-multiply from the lowest bit: a function of (beta, t) alone, restated in tests/adam_ref.py
CGIC_ADAM_HD inline double adam_pow(double beta, uint32_t t)
{
    CGIC_ADAM_NO_CONTRACT
    double r = 1.0, x = beta;
    while (t) {
        if (t & 1u) r = r * x;
        t >>= 1;
        if (t) x = x * x;
    }
    return r;
}

// step_size = lr / (1 - beta1^step) and sqrt(1 - beta2^step) in float64, each rounded to fp32; step: the count AFTER the increment
CGIC_ADAM_HD inline AdamScalars adam_scalars(float step, double lr, double beta1, double beta2)
{
    CGIC_ADAM_NO_CONTRACT
    const uint32_t t = adam_step_exponent(step);
    const double bc1 = 1.0 - adam_pow(beta1, t), bc2 = 1.0 - adam_pow(beta2, t);
    AdamScalars s;
    s.step_size = (float)(lr / bc1);
    s.bc2_sqrt = (float)sqrt(bc2);
    return s;
}

// one element of torch's single-tensor Adam (torch/optim/adam.py, the non-capturable branch): every operation rounds once in fp32
CGIC_ADAM_HD inline void adam_element(float g, float *p_io, float *m_io, float *v_io, const AdamConsts &k, float step_size, float bc2_sqrt)
{
    CGIC_ADAM_NO_CONTRACT
    float p = *p_io, m = *m_io, v = *v_io;
    if (k.do_clip) g = g != g ? g : g < -k.clip ? -k.clip : g > k.clip ? k.clip : g;       // clamp_: a NaN stays
    if (k.do_wd) {
        const float t = k.wd * p;
        g = g + t;
    }
    const float diff = g - m;
    if (k.lerp_low) {
        const float t = k.w1 * diff;
        m = m + t;
    } else {
        const float t = diff * k.one_minus_w1;
        m = g - t;
    }
    v = v * k.beta2;
    {
        const float t = k.w2 * g;
        const float u = t * g;
        v = v + u;
    }
    const float root = sqrtf(v);
    const float scaled = root / bc2_sqrt;
    const float denom = scaled + k.eps;
    const float q = m / denom;
    const float neg = -step_size;
    const float u = neg * q;
    p = p + u;
    *p_io = p; *m_io = m; *v_io = v;
}

// LitEma's element on the NEW parameter: shadow - (omd * (shadow - param))
CGIC_ADAM_HD inline float adam_shadow(float s, float p, float omd)
{
    CGIC_ADAM_NO_CONTRACT
    const float d = s - p;
    const float t = omd * d;
    return s - t;
}

#if !defined(__clang__) && defined(__GNUC__)
#pragma GCC pop_options
#endif

struct AdamPlan {
    std::vector<AdamEntry> entries;
    std::vector<EmaChunk> chunks;
    std::vector<AdamGroup> groups;
    uintptr_t steps;                // fp32 [entries] device buffer of step counts (the caller's)
    int64_t elements;
    int64_t chunks16;               // chunks whose param, exp_avg, exp_avg_sq (and shadow) are 16-byte aligned
    int64_t shadowed;               // entries with a shadow
    int grid;                       // 0: the body has nothing to launch
    size_t table_bytes;
    size_t groups_at, entries_at, chunks_at, scalars_at, grads_at;
    char why_text[224];
};

// CGIC_OK and the plan, or CGIC_ERR_INVALID and *why.  `in` and `groups` are not read before their counts have been checked.
inline int adam_plan(const AdamIn *in, int64_t count, const AdamGroup *groups, int64_t ngroups, uintptr_t steps, AdamPlan *p, const char **why)
{
    p->entries.clear(); p->chunks.clear(); p->groups.clear();
    p->steps = steps;
    p->elements = p->chunks16 = p->shadowed = 0;
    p->grid = 0; p->table_bytes = 0; p->groups_at = p->entries_at = p->chunks_at = p->scalars_at = p->grads_at = 0; p->why_text[0] = 0;
    const auto refuse = [&](int code) { *why = p->why_text; p->entries.clear(); p->chunks.clear(); p->groups.clear(); return code; };
#define CGIC_ADAM_REFUSE(...) do { snprintf(p->why_text, sizeof(p->why_text), __VA_ARGS__); return refuse(CGIC_ERR_INVALID); } while (0)
    if (count < 0 || count > (int64_t)INT32_MAX) CGIC_ADAM_REFUSE("adam_plan: %lld entries (0 .. 2^31 - 1: an entry index is an int32)", (long long)count);
    if (count > 0 && !in) CGIC_ADAM_REFUSE("adam_plan: NULL entry list with %lld entries", (long long)count);
    if (ngroups < 0 || ngroups > kAdamGroupsMax) CGIC_ADAM_REFUSE("adam_plan: %lld EMA groups (0 .. %d)", (long long)ngroups, kAdamGroupsMax);
    if (ngroups > 0 && !groups) CGIC_ADAM_REFUSE("adam_plan: NULL group list with %lld EMA groups", (long long)ngroups);
    if (count > 0 && !steps) CGIC_ADAM_REFUSE("adam_plan: NULL step counts with %lld entries", (long long)count);
    if (steps & 3) CGIC_ADAM_REFUSE("adam_plan: the step counts are not aligned to their 4-byte element");
    for (int64_t g = 0; g < ngroups; ++g) {
        if (!groups[g].decay) CGIC_ADAM_REFUSE("adam_plan: EMA group %lld has a NULL decay", (long long)g);
        if ((groups[g].decay | groups[g].num_updates) & 3)
            CGIC_ADAM_REFUSE("adam_plan: the %s of EMA group %lld is not aligned to its 4-byte element", groups[g].decay & 3 ? "decay" : "num_updates", (long long)g);
    }
    // ---- the checks and the chunk count, before anything is built
    int64_t nchunks = 0;
    for (int64_t i = 0; i < count; ++i) {
        const AdamIn &e = in[i];
        if (e.n < 0) CGIC_ADAM_REFUSE("adam_plan: entry %lld has %lld elements", (long long)i, (long long)e.n);
        if (e.ema_group < -1 || e.ema_group >= ngroups)
            CGIC_ADAM_REFUSE("adam_plan: entry %lld names EMA group %d of %lld (-1: no shadow)", (long long)i, (int)e.ema_group, (long long)ngroups);
        if (e.n > 0 && (!e.param || !e.exp_avg || !e.exp_avg_sq))
            CGIC_ADAM_REFUSE("adam_plan: entry %lld has a NULL %s with %lld elements", (long long)i, !e.param ? "param" : !e.exp_avg ? "exp_avg" : "exp_avg_sq",
                             (long long)e.n);
        if (e.n > 0 && e.ema_group >= 0 && !e.shadow)
            CGIC_ADAM_REFUSE("adam_plan: entry %lld has a NULL shadow with %lld elements in EMA group %d", (long long)i, (long long)e.n, (int)e.ema_group);
        if (e.ema_group < 0 && e.shadow) CGIC_ADAM_REFUSE("adam_plan: entry %lld has a shadow but no EMA group", (long long)i);
        if ((e.param | e.exp_avg | e.exp_avg_sq | e.shadow) & 3)
            CGIC_ADAM_REFUSE("adam_plan: the %s of entry %lld is not aligned to its 4-byte element",
                             e.param & 3 ? "param" : e.exp_avg & 3 ? "exp_avg" : e.exp_avg_sq & 3 ? "exp_avg_sq" : "shadow", (long long)i);
        nchunks += e.n / kEmaChunk + (e.n % kEmaChunk != 0);          // (below 2^51 each, at most 2^31 of them: no overflow)
        if (nchunks > (int64_t)INT32_MAX)
            CGIC_ADAM_REFUSE("adam_plan: more than 2^31 - 1 chunks of %lld elements (a chunk index is an int32)", (long long)kEmaChunk);
    }
#undef CGIC_ADAM_REFUSE
    // ---- the tables
    if (ngroups > 0) p->groups.assign(groups, groups + ngroups);
    p->entries.reserve((size_t)count);
    p->chunks.reserve((size_t)nchunks);
    for (int64_t i = 0; i < count; ++i) {
        AdamEntry e = in[i];
        e.reserved = 0;
        p->entries.push_back(e);
        for (int64_t off = 0; off < e.n; off += kEmaChunk) {
            const int64_t len = e.n - off < kEmaChunk ? e.n - off : kEmaChunk;
            p->chunks.push_back(EmaChunk{(int32_t)i, (int32_t)len, off});
            p->chunks16 += adam_all_16(e.param, e.exp_avg, e.exp_avg_sq, e.shadow, 0);
        }
        p->elements += e.n;
        p->shadowed += e.ema_group >= 0;
    }
    p->grid = (int)(nchunks < kEmaGridMax ? nchunks : kEmaGridMax);
    p->groups_at = kAdamHeadBytes;
    p->entries_at = p->groups_at + sizeof(AdamGroup) * kAdamGroupsMax;
    p->chunks_at = p->entries_at + sizeof(AdamEntry) * p->entries.size();
    p->scalars_at = p->chunks_at + sizeof(EmaChunk) * p->chunks.size();
    p->grads_at = p->scalars_at + sizeof(AdamScalars) * p->entries.size();
    p->table_bytes = p->grads_at + sizeof(uintptr_t) * p->entries.size();
    return CGIC_OK;
}

}  // namespace cgic
