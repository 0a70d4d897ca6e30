// rate_plan_main.cpp -- prints the plans of the rate-control family (csrc/cgic_rate_plan.h) and the router's rank arithmetic
// (csrc/cgic_encode_plan.h: router_ranks) for the cases it is given (no GPU, no library).  A case is 72 integers, from the arguments
// or, without arguments, from stdin:
//   what  table nsym max_len  B h16 w16 ratio  R  T N S M tile_nbytes_given  C inputs
//   ind_c ind_m ind_f e16 e8 nbytes tiles_dev image_nbytes ranks_dev budget_dev mask_c mask_m mask_f ind choice_dev workspace
//   count_given count[5]  tiles_given  3 x (h16 w16 k_c shape image reserved off_c off_m off_f off_e16 off_e8)
// what: 0 / 1 / 2 curve_plan of cgic_rate_curve / cgic_rate_curve_tiles / cgic_route_to_budget; 3 rate_table_plan; 4 / 5 / 6 the size
// query of entry what - 4; 7 the rate table's size query; 8 router_ranks(mode of (ratio, ratio2), n16 = B) with ratio2 in the place
// of R.  ratio (and ratio2) are the bit patterns of float64 values, so that every field is an integer and a NaN can be asked for;
// the sixteen addresses are plain integers, 0 = NULL.  Descriptors past the third are zeros (a tile without a shape).
// One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_rate_plan.h"
#include "../../include/cgic_hip.h"

static double as_double(long long bits)
{
    double d;
    memcpy(&d, &bits, sizeof d);
    return d;
}

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    const size_t per_case = 72;
    if (tok.empty() || tok.size() % per_case != 0) {
        fprintf(stderr, "rate_plan_main: %zu numbers, expected a multiple of %zu\n", tok.size(), per_case);
        return 2;
    }
    for (size_t at = 0; at < tok.size(); at += per_case) {
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        const int what = (int)num(0);
        const char *why = "";
        if (what == 8) {
            const double c = as_double(num(7)), m = as_double(num(8));
            double k_c, k_m;
            const int mode = cgic::router_mode(c, m);
            const bool ok = cgic::router_ranks(mode, num(4), c, m, &k_c, &k_m);
            printf("ok=%d mode=%d k_c=%.0f k_m=%.0f\n", (int)ok, mode, k_c, k_m);
            continue;
        }
        if (what == 3 || what == 7) {
            cgic::RateTableCall c{};
            c.table = num(1) != 0; c.nsym = (int)num(2); c.max_len = (int)num(3);
            c.B = num(4); c.h16 = num(5); c.w16 = num(6); c.C = (int)num(14);
            c.inputs = num(15) != 0;
            c.workspace = (uintptr_t)num(31);
            cgic::RateTablePlan p;
            if (what == 7) {
                printf("bytes=%zu\n", cgic::rate_table_form(c.B, c.h16, c.w16, c.C, &p, &why) == CGIC_OK ? p.workspace_needed : (size_t)0);
                continue;
            }
            const int rc = cgic::rate_table_plan(c, &p, &why);
            if (rc != CGIC_OK) { printf("err=%d why=%s\n", rc, why); continue; }
            printf("nothing=%d stride_c=%lld stride_m=%lld stride_f=%lld off_c=%zu off_m=%zu off_f=%zu workspace=%zu grid_x=%lld grid_y=%lld lds=%zu\n",
                   (int)p.nothing_to_do, (long long)p.stride_c, (long long)p.stride_m, (long long)p.stride_f, p.off_c, p.off_m, p.off_f,
                   p.workspace_needed, (long long)p.grid_x, (long long)p.grid_y, p.lds_bytes);
            continue;
        }
        cgic::CurveCall c{};
        cgic::CurveShape &s = c.shape;
        s.entry = (cgic::CurveEntry)(what % 4);
        c.table = num(1) != 0; c.nsym = (int)num(2); c.max_len = (int)num(3);
        s.B = num(4); s.h16 = num(5); s.w16 = num(6);
        c.coarse_ratio = as_double(num(7));
        s.R = num(8); s.T = num(9); s.N = num(10); s.S = num(11); s.M = num(12); s.tile_nbytes_given = num(13) != 0;
        if (what >= 4) {
            printf("bytes=%zu\n", cgic::curve_workspace_bytes(s));
            continue;
        }
        uintptr_t *const addr[16] = {&c.ind_c, &c.ind_m, &c.ind_f, &c.e16, &c.e8, &c.nbytes, &c.tiles_dev, &c.image_nbytes, &c.ranks_dev,
                                     &c.budget_dev, &c.mask_c, &c.mask_m, &c.mask_f, &c.ind, &c.choice_dev, &c.workspace};
        for (int i = 0; i < 16; ++i) *addr[i] = (uintptr_t)num(16 + i);
        int64_t count[5];
        for (int i = 0; i < 5; ++i) count[i] = num(33 + i);
        c.count = num(32) ? count : nullptr;
        // (as many descriptors as the call says it has, so that the plan never reads past them)
        std::vector<cgic_rate_tile> tiles((size_t)(s.T > 3 && s.T <= 65536 ? s.T : 3), cgic_rate_tile{});
        for (int k = 0; k < 3; ++k) {
            const int o = 39 + 11 * k;
            cgic_rate_tile &d = tiles[k];
            d.h16 = (int32_t)num(o); d.w16 = (int32_t)num(o + 1); d.k_c = (int32_t)num(o + 2); d.shape = (int32_t)num(o + 3);
            d.image = (int32_t)num(o + 4); d.reserved = (int32_t)num(o + 5);
            d.off_c = num(o + 6); d.off_m = num(o + 7); d.off_f = num(o + 8); d.off_e16 = num(o + 9); d.off_e8 = num(o + 10);
        }
        c.tiles = num(38) ? tiles.data() : nullptr;
        cgic::CurvePlan p;
        const int rc = cgic::curve_plan(c, &p, &why);
        if (rc != CGIC_OK) { printf("err=%d why=%s\n", rc, why); continue; }
        printf("nothing=%d mode=%d k_c=%lld n8_max=%lld grid=%lld threads=%d lds=%zu staged=%d opt_in=%d workspace=%zu off_summary=%zu off_total=%zu "
               "off_tkey=%zu off_tile_nbytes=%zu fold_x=%lld fold_y=%lld pick_grid=%lld apply_grid=%lld\n",
               (int)p.nothing_to_do, p.mode, (long long)p.k_c, (long long)p.n8_max, (long long)p.grid, p.threads, p.lds_bytes, (int)p.staged,
               (int)p.lds_opt_in, p.workspace_needed, p.off_summary, p.off_total, p.off_tkey, p.off_tile_nbytes, (long long)p.fold_grid_x,
               (long long)p.fold_grid_y, (long long)p.pick_grid, (long long)p.apply_grid);
    }
    return 0;
}
