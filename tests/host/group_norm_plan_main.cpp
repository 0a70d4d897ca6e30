// group_norm_plan_main.cpp -- prints the launch plans of cgic_group_norm, cgic_group_norm_train and cgic_group_norm_backward: the
// plans of csrc/cgic_norm_plan.h and csrc/cgic_norm_bwd_plan.h with their `plain` flag, which this program takes as a number so
// that the same case can be planned both ways (no GPU, no library).  Numbers from the arguments or, without arguments, from stdin;
// a case begins with its kind:
//   0 plain in_dtype out_dtype B C H W hq wq groups f zq gn_weight gn_bias wy by wb bb out workspace workspace_bytes stats
//     (the forward: 22 numbers; stats 0: cgic_group_norm / cgic_spatial_norm, else the training forward)
//   1 plain in_dtype go_dtype df_dtype B C H W hq wq groups  f go zq stats gn_weight gn_bias wy by wb bb
//     df dzq dgn_weight dgn_bias dwy dby dwb dbb  workspace workspace_bytes                                   (the backward: 31 numbers)
// (addresses as plain integers, 0 = NULL).  One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_norm_bwd_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    size_t at = 0;
    while (at < tok.size()) {
        const long long kind = strtoll(tok[at].c_str(), nullptr, 10);
        const size_t per_case = kind == 0 ? 23 : 32;
        if ((kind != 0 && kind != 1) || at + per_case > tok.size()) {
            fprintf(stderr, "group_norm_plan_main: case of kind %lld at number %zu of %zu\n", kind, at, tok.size());
            return 2;
        }
        const auto num = [&](int i) { return strtoll(tok[at + 1 + i].c_str(), nullptr, 10); };
        const char *why = "";
        if (kind == 0) {
            cgic::NormCall c{};
            c.plain = num(0) != 0;
            c.in_dtype = (int)num(1); c.out_dtype = (int)num(2);
            c.B = num(3); c.C = num(4); c.H = num(5); c.W = num(6); c.hq = num(7); c.wq = num(8); c.groups = num(9);
            c.f = (uintptr_t)num(10); c.zq = (uintptr_t)num(11); c.gn_weight = (uintptr_t)num(12); c.gn_bias = (uintptr_t)num(13);
            c.wy = (uintptr_t)num(14); c.by = (uintptr_t)num(15); c.wb = (uintptr_t)num(16); c.bb = (uintptr_t)num(17);
            c.out = (uintptr_t)num(18); c.workspace = (uintptr_t)num(19); c.workspace_bytes = (size_t)num(20);
            const uintptr_t stats = (uintptr_t)num(21);
            cgic::NormPlan p;
            const int rc = stats ? cgic::norm_train_plan(c, stats, &p, &why) : cgic::norm_plan(c, &p, &why);
            if (rc != CGIC_OK)
                printf("err=%d why=%s\n", rc, why);
            else
                printf("form=%d unit=%d span=%lld spans=%lld chunks=%d chunk_units=%lld ymul=%d ydiv=%d xmul=%d xdiv=%d grid_one=%lld "
                       "grid_stats=%lld grid_apply=%lld parts=%lld lds=%zu workspace=%zu in_place=%d mg_w=%u mg_y=%u mg_x=%u zq_vec=%d\n",
                       p.form, p.unit, (long long)p.span, (long long)p.spans, p.chunks, (long long)p.chunk_units, p.ymul, p.ydiv, p.xmul, p.xdiv,
                       (long long)p.grid_one, (long long)p.grid_stats, (long long)p.grid_apply, (long long)p.parts, p.lds_bytes,
                       p.workspace_needed, (int)p.in_place, p.mg_w, p.mg_y, p.mg_x, (int)p.zq_vec);
            at += per_case;
            continue;
        }
        cgic::NormBwdCall c{};
        c.plain = num(0) != 0;
        c.in_dtype = (int)num(1); c.go_dtype = (int)num(2); c.df_dtype = (int)num(3);
        c.B = num(4); c.C = num(5); c.H = num(6); c.W = num(7); c.hq = num(8); c.wq = num(9); c.groups = num(10);
        c.f = (uintptr_t)num(11); c.go = (uintptr_t)num(12); c.zq = (uintptr_t)num(13); c.stats = (uintptr_t)num(14);
        c.gn_weight = (uintptr_t)num(15); c.gn_bias = (uintptr_t)num(16); c.wy = (uintptr_t)num(17); c.by = (uintptr_t)num(18);
        c.wb = (uintptr_t)num(19); c.bb = (uintptr_t)num(20);
        c.df = (uintptr_t)num(21); c.dzq = (uintptr_t)num(22); c.dgn_weight = (uintptr_t)num(23); c.dgn_bias = (uintptr_t)num(24);
        c.dwy = (uintptr_t)num(25); c.dby = (uintptr_t)num(26); c.dwb = (uintptr_t)num(27); c.dbb = (uintptr_t)num(28);
        c.workspace = (uintptr_t)num(29); c.workspace_bytes = (size_t)num(30);
        cgic::NormBwdPlan p;
        const int rc = cgic::norm_bwd_plan(c, &p, &why);
        if (rc != CGIC_OK)
            printf("err=%d why=%s\n", rc, why);
        else
            printf("unit=%d span=%lld spans=%lld chan_block=%d chan_blocks=%lld threads_reduce=%d tiles=%lld tiles_max=%lld grid_reduce=%lld "
                   "grid_sums=%lld grid_dzq=%lld grid_apply=%lld parts=%lld need_dz=%d need_conv=%d need_df=%d in_place=%d sums=%d off_sums=%zu "
                   "off_span=%zu off_dz=%zu workspace=%zu zq_vec=%d\n",
                   p.unit, (long long)p.span, (long long)p.spans, p.chan_block, (long long)p.chan_blocks, p.threads_reduce, (long long)p.tiles,
                   (long long)p.tiles_max, (long long)p.grid_reduce, (long long)p.grid_sums, (long long)p.grid_dzq, (long long)p.grid_apply,
                   (long long)p.parts, (int)p.need_dz, (int)p.need_conv, (int)p.need_df, (int)p.in_place, p.sums, p.off_sums, p.off_span, p.off_dz,
                   p.workspace_needed, (int)p.zq_vec);
        at += per_case;
    }
    return 0;
}
