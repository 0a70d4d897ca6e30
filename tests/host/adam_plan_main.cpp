// adam_plan_main.cpp -- prints what csrc/cgic_adam_plan.h decides and computes for the cases it is given (no GPU, no library).  One case
// per line of stdin, one line of output per case.  Floats travel as the 32 bits of the float in decimal, doubles as C99 hex floats.
//   plan K G STEPS  (param exp_avg exp_avg_sq shadow n ema_group) x K  (decay num_updates) x G
//                              the plan of K entries and G EMA groups (addresses as plain integers, 0 = NULL): its fields as
//                              name=value, the chunk table as entry:offset:length,... when it has at most 12 chunks, and covered=1
//                              when the program's own walk finds every element of every entry in exactly one chunk, the chunks of an
//                              entry in order and the entries in order; or err=<code> why=<reason>
//   count N                    adam_plan of N entries with a list of ONE entry (a refusal must come before the list is read)
//   null N                     adam_plan of N entries with no list
//   groups N                   adam_plan of no entries and N EMA groups with a list of ONE group
//   nullgroups N               adam_plan of no entries and N EMA groups with no list
//   pro STEP LR BETA1 BETA2    the prologue of one entry that found STEP: next=<bits> step_size=<bits> bc2_sqrt=<bits>
//   el G P M V STEP_SIZE BC2 BETA1 BETA2 EPS WD CLIP DO_CLIP      adam_element: p=<bits> m=<bits> v=<bits>
//   sh S P OMD                 adam_shadow: s=<bits>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_adam_plan.h"

static float f_of(unsigned long long bits)
{
    const uint32_t b = (uint32_t)bits;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

static unsigned bits_of(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return b;
}

static bool covered(const std::vector<cgic::AdamIn> &in, const cgic::AdamPlan &p)
{
    size_t c = 0;
    int64_t n16 = 0, shadowed = 0;
    if (p.entries.size() != in.size()) return false;
    for (size_t i = 0; i < in.size(); ++i) {
        const cgic::AdamEntry &e = p.entries[i];
        if (e.param != in[i].param || e.exp_avg != in[i].exp_avg || e.exp_avg_sq != in[i].exp_avg_sq || e.shadow != in[i].shadow || e.n != in[i].n ||
            e.ema_group != in[i].ema_group)
            return false;
        shadowed += in[i].ema_group >= 0;
        int64_t at = 0;
        while (at < in[i].n) {
            if (c >= p.chunks.size()) return false;
            const cgic::EmaChunk &ch = p.chunks[c++];
            const int64_t want = in[i].n - at < cgic::kEmaChunk ? in[i].n - at : cgic::kEmaChunk;
            if (ch.entry != (int32_t)i || ch.off != at || ch.len != want) return false;
            n16 += (in[i].param % 16 == 0 && in[i].exp_avg % 16 == 0 && in[i].exp_avg_sq % 16 == 0 && in[i].shadow % 16 == 0);
            at += ch.len;
        }
    }
    return c == p.chunks.size() && n16 == p.chunks16 && shadowed == p.shadowed;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        if (!(is >> cmd)) continue;
        if (cmd == "pro") {
            unsigned long long step;
            std::string lr, b1, b2;
            is >> step >> lr >> b1 >> b2;
            const float next = f_of(step) + 1.0f;
            const cgic::AdamScalars s = cgic::adam_scalars(next, strtod(lr.c_str(), nullptr), strtod(b1.c_str(), nullptr), strtod(b2.c_str(), nullptr));
            printf("next=%u step_size=%u bc2_sqrt=%u\n", bits_of(next), bits_of(s.step_size), bits_of(s.bc2_sqrt));
            continue;
        }
        if (cmd == "el") {
            unsigned long long g, p, m, v, ss, bc;
            std::string b1, b2, eps, wd, clip;
            int do_clip;
            is >> g >> p >> m >> v >> ss >> bc >> b1 >> b2 >> eps >> wd >> clip >> do_clip;
            const cgic::AdamConsts k = cgic::adam_consts(strtod(b1.c_str(), nullptr), strtod(b2.c_str(), nullptr), strtod(eps.c_str(), nullptr),
                                                         strtod(wd.c_str(), nullptr), strtod(clip.c_str(), nullptr), do_clip != 0);
            float pf = f_of(p), mf = f_of(m), vf = f_of(v);
            cgic::adam_element(f_of(g), &pf, &mf, &vf, k, f_of(ss), f_of(bc));
            printf("p=%u m=%u v=%u\n", bits_of(pf), bits_of(mf), bits_of(vf));
            continue;
        }
        if (cmd == "sh") {
            unsigned long long s, p, omd;
            is >> s >> p >> omd;
            printf("s=%u\n", bits_of(cgic::adam_shadow(f_of(s), f_of(p), f_of(omd))));
            continue;
        }
        cgic::AdamPlan p;
        const char *why = "";
        std::vector<cgic::AdamIn> in;
        std::vector<cgic::AdamGroup> gr;
        int rc;
        if (cmd == "count" || cmd == "null") {
            long long n;
            is >> n;
            in.push_back(cgic::AdamIn{4096, 8192, 12288, 0, 1, -1, 0});
            rc = cgic::adam_plan(cmd == "null" ? nullptr : in.data(), n, nullptr, 0, 1 << 20, &p, &why);
            in.clear();
        } else if (cmd == "groups" || cmd == "nullgroups") {
            long long n;
            is >> n;
            gr.push_back(cgic::AdamGroup{4096, 8192});
            rc = cgic::adam_plan(nullptr, 0, cmd == "nullgroups" ? nullptr : gr.data(), n, 0, &p, &why);
        } else if (cmd == "plan") {
            long long k, g;
            unsigned long long steps;
            is >> k >> g >> steps;
            for (long long i = 0; i < k; ++i) {
                unsigned long long a, b, c, d;
                long long n, group;
                if (!(is >> a >> b >> c >> d >> n >> group)) {
                    fprintf(stderr, "adam_plan_main: %lld entries announced, %lld given\n", k, i);
                    return 2;
                }
                in.push_back(cgic::AdamIn{(uintptr_t)a, (uintptr_t)b, (uintptr_t)c, (uintptr_t)d, (int64_t)n, (int32_t)group, 0});
            }
            for (long long i = 0; i < g; ++i) {
                unsigned long long a, b;
                if (!(is >> a >> b)) {
                    fprintf(stderr, "adam_plan_main: %lld groups announced, %lld given\n", g, i);
                    return 2;
                }
                gr.push_back(cgic::AdamGroup{(uintptr_t)a, (uintptr_t)b});
            }
            rc = cgic::adam_plan(in.data(), (int64_t)in.size(), gr.data(), (int64_t)gr.size(), (uintptr_t)steps, &p, &why);
        } else {
            fprintf(stderr, "adam_plan_main: unknown case %s\n", cmd.c_str());
            return 2;
        }
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        printf("entries=%zu elements=%lld chunks=%zu chunk=%lld chunks16=%lld grid=%d groups=%zu shadowed=%lld table_bytes=%zu covered=%d table=",
               p.entries.size(), (long long)p.elements, p.chunks.size(), (long long)cgic::kEmaChunk, (long long)p.chunks16, p.grid, p.groups.size(),
               (long long)p.shadowed, p.table_bytes, (int)covered(in, p));
        if (p.chunks.size() > 12 || p.chunks.empty()) printf("-");
        for (size_t c = 0; c < p.chunks.size() && p.chunks.size() <= 12; ++c)
            printf("%s%d:%lld:%d", c ? "," : "", (int)p.chunks[c].entry, (long long)p.chunks[c].off, (int)p.chunks[c].len);
        printf("\n");
    }
    return 0;
}
