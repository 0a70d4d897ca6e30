// decode_plan_main.cpp -- prints the launch plan of cgic_decompress_streams for the cases it is given (no GPU, no library).
// A case is 13 numbers, from the arguments or, without arguments, from stdin:
//   B h w slot K has_zq max_len lut_bits dec_mode cus cu_share no_fuse lds_decoder
// One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_decode_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    const size_t per_case = 13;
    if (tok.empty() || tok.size() % per_case != 0) {
        fprintf(stderr, "decode_plan_main: %zu numbers, expected a multiple of %zu\n", tok.size(), per_case);
        return 2;
    }
    static const char *const decoder[] = {"fused", "image", "split", "serial"};
    static const char *const merge[] = {"bands", "one_band"};
    for (size_t at = 0; at < tok.size(); at += per_case) {
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        cgic::DecodeShape s;
        s.B = num(0); s.h = num(1); s.w = num(2); s.slot = num(3); s.K = (int)num(4); s.has_zq = num(5) != 0;
        s.max_len = (int)num(6); s.lut_bits = (int)num(7); s.dec_mode = (int)num(8); s.cus = (int)num(9);
        s.cu_share = strtod(tok[at + 10].c_str(), nullptr); s.no_fuse = num(11) != 0; s.lds_decoder = (size_t)num(12);
        cgic::DecodePlan p;
        const char *why = "";
        const int rc = cgic::decode_plan(s, &p, &why);
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        printf("decoder=%s merge=%s ndec=%u nbands=%lld active=%u stage_cb=%d stage_sym=%d band_syms=%lld lds_d=%zu lds_m=%zu lds_f=%zu "
               "lds_ss=%zu stage_cap=%zu chunk_cap=%zu image_threads=%d split_batch=%lld\n",
               decoder[p.decoder], merge[p.merge], p.ndec, (long long)p.nbands, p.active_bands, p.stage_cb, p.stage_sym,
               (long long)p.band_syms, p.lds_d, p.lds_m, p.lds_f, p.lds_ss, p.stage_cap, p.chunk_cap, p.image_threads,
               (long long)p.split_batch);
    }
    return 0;
}
