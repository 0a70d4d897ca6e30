// norm_plan_main.cpp -- prints the launch plan of cgic_spatial_norm (csrc/cgic_norm_plan.h) for the cases it is given (no GPU, no
// library).  A case is 20 numbers, from the arguments or, without arguments, from stdin:
//   in_dtype out_dtype B C H W hq wq groups f zq gn_weight gn_bias wy by wb bb out workspace workspace_bytes
// (the ten addresses as plain integers, 0 = NULL).
// One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_norm_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    const size_t per_case = 20;
    if (tok.empty() || tok.size() % per_case != 0) {
        fprintf(stderr, "norm_plan_main: %zu numbers, expected a multiple of %zu\n", tok.size(), per_case);
        return 2;
    }
    for (size_t at = 0; at < tok.size(); at += per_case) {
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        cgic::NormCall c{};
        c.in_dtype = (int)num(0); c.out_dtype = (int)num(1);
        c.B = num(2); c.C = num(3); c.H = num(4); c.W = num(5); c.hq = num(6); c.wq = num(7); c.groups = num(8);
        c.f = (uintptr_t)num(9); c.zq = (uintptr_t)num(10); c.gn_weight = (uintptr_t)num(11); c.gn_bias = (uintptr_t)num(12);
        c.wy = (uintptr_t)num(13); c.by = (uintptr_t)num(14); c.wb = (uintptr_t)num(15); c.bb = (uintptr_t)num(16);
        c.out = (uintptr_t)num(17); c.workspace = (uintptr_t)num(18); c.workspace_bytes = (size_t)num(19);
        cgic::NormPlan p;
        const char *why = "";
        const int rc = cgic::norm_plan(c, &p, &why);
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        printf("form=%d unit=%d span=%lld spans=%lld chunks=%d chunk_units=%lld ymul=%d ydiv=%d xmul=%d xdiv=%d grid_one=%lld grid_stats=%lld "
               "grid_apply=%lld parts=%lld lds=%zu workspace=%zu in_place=%d threads_one=%d threads=%d mg_w=%u mg_y=%u mg_x=%u zq_vec=%d\n",
               p.form, p.unit, (long long)p.span, (long long)p.spans, p.chunks, (long long)p.chunk_units, p.ymul, p.ydiv, p.xmul, p.xdiv,
               (long long)p.grid_one, (long long)p.grid_stats, (long long)p.grid_apply, (long long)p.parts, p.lds_bytes, p.workspace_needed,
               (int)p.in_place, p.threads_one, p.threads, p.mg_w, p.mg_y, p.mg_x, (int)p.zq_vec);
    }
    return 0;
}
