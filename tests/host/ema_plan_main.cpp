// ema_plan_main.cpp -- prints what csrc/cgic_ema_plan.h decides for the cases it is given (no GPU, no library).  One case per line of
// stdin, one line of output per case:
//   plan K  shadow param n  (K times)     the plan of K entries (addresses as plain integers, 0 = NULL): its fields as name=value, the
//                                         chunk table as entry:offset:length,... when it has at most 12 chunks, and covered=1 when the
//                                         program's own walk finds every element of every entry in exactly one chunk, the chunks of
//                                         an entry in order and the entries in order; or err=<code> why=<reason>
//   count N                               ema_plan of N entries with a list of ONE entry (a refusal must come before the list is read)
//   null N                                ema_plan of N entries with no list
//   omd DECAY_BITS N HAS                  ema_one_minus_decay(decay, N, HAS) and ema_next_count(N): omd=<bits> next=<n>, decay and omd
//                                         as the 32 bits of the float, in decimal
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_ema_plan.h"

static bool covered(const std::vector<cgic::EmaIn> &in, const cgic::EmaPlan &p)
{
    size_t c = 0;
    int64_t n16 = 0, n16s = 0, stash = 0;
    if (p.entries.size() != in.size()) return false;
    for (size_t i = 0; i < in.size(); ++i) {
        const cgic::EmaEntry &e = p.entries[i];
        if (e.shadow != in[i].shadow || e.param != in[i].param || e.n != in[i].n || e.stash_off != stash || stash % 4) return false;
        stash += (in[i].n + 3) / 4 * 4;
        int64_t at = 0;
        while (at < in[i].n) {
            if (c >= p.chunks.size()) return false;
            const cgic::EmaChunk &ch = p.chunks[c++];
            const int64_t want = in[i].n - at < cgic::kEmaChunk ? in[i].n - at : cgic::kEmaChunk;
            if (ch.entry != (int32_t)i || ch.off != at || ch.len != want) return false;
            n16 += (in[i].shadow % 16 == 0 && in[i].param % 16 == 0);
            n16s += in[i].param % 16 == 0;
            at += ch.len;
        }
    }
    return c == p.chunks.size() && n16 == p.chunks16 && n16s == p.chunks16_stash && stash == p.stash_elements;
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        if (!(is >> cmd)) continue;
        cgic::EmaPlan p;
        const char *why = "";
        if (cmd == "omd") {
            unsigned long long bits;
            long long n;
            int has;
            is >> bits >> n >> has;
            const uint32_t b = (uint32_t)bits;
            float decay;
            memcpy(&decay, &b, 4);
            const float omd = cgic::ema_one_minus_decay(decay, (int32_t)n, has != 0);
            uint32_t ob;
            memcpy(&ob, &omd, 4);
            printf("omd=%u next=%d\n", ob, (int)cgic::ema_next_count((int32_t)n));
            continue;
        }
        std::vector<cgic::EmaIn> in;
        int rc;
        if (cmd == "count" || cmd == "null") {
            long long n;
            is >> n;
            in.push_back(cgic::EmaIn{4096, 8192, 1});
            rc = cgic::ema_plan(cmd == "null" ? nullptr : in.data(), n, &p, &why);
            in.clear();
        } else if (cmd == "plan") {
            long long k;
            is >> k;
            for (long long i = 0; i < k; ++i) {
                unsigned long long s, q;
                long long n;
                if (!(is >> s >> q >> n)) {
                    fprintf(stderr, "ema_plan_main: %lld entries announced, %lld given\n", k, i);
                    return 2;
                }
                in.push_back(cgic::EmaIn{(uintptr_t)s, (uintptr_t)q, (int64_t)n});
            }
            rc = cgic::ema_plan(in.data(), (int64_t)in.size(), &p, &why);
        } else {
            fprintf(stderr, "ema_plan_main: unknown case %s\n", cmd.c_str());
            return 2;
        }
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        printf("entries=%zu elements=%lld chunks=%zu chunk=%lld chunks16=%lld chunks16_stash=%lld grid=%d table_bytes=%zu stash=%lld covered=%d table=",
               p.entries.size(), (long long)p.elements, p.chunks.size(), (long long)cgic::kEmaChunk, (long long)p.chunks16, (long long)p.chunks16_stash,
               p.grid, p.table_bytes, (long long)p.stash_elements, (int)covered(in, p));
        if (p.chunks.size() > 12 || p.chunks.empty()) printf("-");
        for (size_t c = 0; c < p.chunks.size() && p.chunks.size() <= 12; ++c)
            printf("%s%d:%lld:%d", c ? "," : "", (int)p.chunks[c].entry, (long long)p.chunks[c].off, (int)p.chunks[c].len);
        printf("\n");
    }
    return 0;
}
