// attn_bwd_plan_main.cpp -- prints the launch plan of cgic_attention_backward (csrc/cgic_attn_bwd_plan.h) for the cases it is given
// (no GPU, no library).  A case is 21 numbers, from the arguments or, without arguments, from stdin:
//   in_dtype grad_dtype B C N go_batch_stride q_batch_stride k_batch_stride v_batch_stride scale_x1e6
//   go q k v out lse dq dk dv workspace workspace_bytes
// (the ten addresses as plain integers, 0 = NULL; the scale in millionths, so that every field is an integer; workspace_bytes -1:
// what the plan asks for).  One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_attn_bwd_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    const size_t per_case = 21;
    if (tok.empty() || tok.size() % per_case != 0) {
        fprintf(stderr, "attn_bwd_plan_main: %zu numbers, expected a multiple of %zu\n", tok.size(), per_case);
        return 2;
    }
    for (size_t at = 0; at < tok.size(); at += per_case) {
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        cgic::AttnBwdCall c{};
        c.in_dtype = (int)num(0); c.grad_dtype = (int)num(1);
        c.B = num(2); c.C = num(3); c.N = num(4);
        c.go_batch_stride = num(5); c.q_batch_stride = num(6); c.k_batch_stride = num(7); c.v_batch_stride = num(8);
        c.scale = (double)num(9) * 1e-6;
        c.go = (uintptr_t)num(10); c.q = (uintptr_t)num(11); c.k = (uintptr_t)num(12); c.v = (uintptr_t)num(13); c.out = (uintptr_t)num(14);
        c.lse = (uintptr_t)num(15); c.dq = (uintptr_t)num(16); c.dk = (uintptr_t)num(17); c.dv = (uintptr_t)num(18);
        c.workspace = (uintptr_t)num(19);
        cgic::AttnBwdPlan p;
        const char *why = "";
        if (num(20) < 0) {
            const int rc = cgic::attn_bwd_form(c.in_dtype, c.grad_dtype, c.B, c.C, c.N, &p, &why);
            c.workspace_bytes = rc == CGIC_OK ? p.workspace_needed : 0;
        } else {
            c.workspace_bytes = (size_t)num(20);
        }
        const int rc = cgic::attn_bwd_plan(c, &p, &why);
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        printf("form=%d pre_run=%d pre_threads=%d pre_grid=%lld dq_run=%d dq_threads=%d dq_tiles=%lld dq_grid=%lld dq_lds=%zu dkdv_run=%d "
               "dkdv_threads=%d dkdv_tiles=%lld dkdv_grid=%lld dkdv_lds=%zu dq_vec=%d dkdv_vec=%d workspace=%zu\n",
               p.form, (int)p.pre.run, p.pre.threads, (long long)p.pre.grid, (int)p.dq.run, p.dq.threads, (long long)p.dq.tiles, (long long)p.dq.grid,
               p.dq.lds_bytes, (int)p.dkdv.run, p.dkdv.threads, (long long)p.dkdv.tiles, (long long)p.dkdv.grid, p.dkdv.lds_bytes, (int)p.dq_vec,
               (int)p.dkdv_vec, p.workspace_needed);
    }
    return 0;
}
