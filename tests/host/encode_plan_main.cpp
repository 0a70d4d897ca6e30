// encode_plan_main.cpp -- prints the plans of the encode host path for the cases it is given (no GPU, no library).
// A case is a letter and its numbers, from the arguments or, without arguments, from stdin:
//   R B h16 w16 c_ratio m_ratio per_image refine has_scratch scratch_bytes queues lds_budget lds_shared lds_refine
//   V N hw K conv loss perm_image cus cu_share recording router_wgs router_lds router_queues lds_filter kid_aligned kid_unaligned
//     knob_exact knob_zt knob_wgs_per_cu knob_nosplit knob_ge
// One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_encode_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    static const char *const router_why[] = {"", "segment too large", "k out of range", "does not fit the LDS", "refinement of too many patches",
                                             "exceeds LDS", "scratch too small"};
    static const char *const path[] = {"filter", "exact"};
    static const char *const variant[] = {"plain", "perm", "router", "router_perm", "router_split"};
    size_t at = 0;
    while (at < tok.size()) {
        const bool is_router = tok[at] == "R";
        const size_t n = is_router ? 13 : 20;
        if ((!is_router && tok[at] != "V") || at + 1 + n > tok.size()) {
            fprintf(stderr, "encode_plan_main: case at token %zu: expected R + 13 or V + 20 numbers\n", at);
            return 2;
        }
        ++at;
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        const auto real = [&](int i) { return strtod(tok[at + i].c_str(), nullptr); };
        if (is_router) {
            cgic::RouterShape s;
            s.B = num(0); s.h16 = num(1); s.w16 = num(2); s.c_ratio = real(3); s.m_ratio = real(4); s.per_image = num(5) != 0;
            s.refine = num(6) != 0; s.has_scratch = num(7) != 0; s.scratch_bytes = (size_t)num(8); s.queues = num(9) != 0;
            s.lds_budget = (size_t)num(10); s.lds_shared = (size_t)num(11); s.lds_refine = (size_t)num(12);
            cgic::RouterPlan p;
            cgic::RouterWhy why;
            const int rc = cgic::router_plan(s, &p, &why);
            if (rc != CGIC_OK) printf("err=%d why=%s\n", rc, router_why[why]);
            else
                printf("mode=%d k_c=%lld k_m=%lld rank_c=%u rank_m=%u mg_n8=%u mg_w8=%u mg_n4=%u mg_w4=%u refined=%d stage=%d lds=%zu bands=%d "
                       "nseg=%lld wgs=%lld nq=%u scratch_need=%zu\n",
                       p.mode, (long long)p.k_c, (long long)p.k_m, p.rank_c, p.rank_m, p.mg_n8, p.mg_w8, p.mg_n4, p.mg_w4, (int)p.refined,
                       p.stage, p.lds, p.bands, (long long)p.nseg, (long long)p.wgs, p.nq, p.scratch_need);
        } else {
            cgic::VqShape s;
            s.N = num(0); s.hw = num(1); s.K = (int)num(2); s.conv = num(3) != 0; s.loss = num(4) != 0; s.perm_image = num(5) != 0;
            s.cus = (int)num(6); s.cu_share = real(7); s.recording = num(8) != 0; s.router_wgs = num(9); s.router_lds = (size_t)num(10);
            s.router_queues = num(11) != 0; s.lds_filter = (size_t)num(12); s.kid_aligned = (int)num(13); s.kid_unaligned = (int)num(14);
            s.knob_exact = (int)num(15); s.knob_zt = (int)num(16); s.knob_wgs_per_cu = (int)num(17); s.knob_nosplit = (int)num(18);
            s.knob_ge = (int)num(19);
            cgic::VqPlan p;
            const char *why = "";
            const int rc = cgic::vq_plan(s, &p, &why);
            if (rc != CGIC_OK) printf("err=%d why=%s\n", rc, why);
            else
                printf("path=%s zt=%d aligned=%d variant=%s nblk=%lld n_early=%lld g_early=%lld g_late=%lld behind=%d grid=%lld threads=%d "
                       "lds=%zu tail_mode=%u tickets=%d kid=%d\n",
                       path[p.path], p.zt, (int)p.aligned, variant[p.variant], (long long)p.nblk, (long long)p.n_early, (long long)p.g_early,
                       (long long)p.g_late, (int)p.router_behind, (long long)p.grid, p.threads, p.lds, p.tail_mode, p.tickets, p.kid);
        }
        at += n;
    }
    return 0;
}
