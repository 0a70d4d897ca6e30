// coder_plan_main.cpp -- prints the launch plan of cgic_compress_streams for the cases it is given (no GPU, no library).
// A case is 8 numbers, from the arguments or, without arguments, from stdin:
//   B h w slot max_len nsym has_hist has_workspace
// One line per case: the plan's fields as name=value (with the sizes the size queries answer for the shape), or err=<code> and the
// reason.  per_c / per_m / per_f: enc_part_positions of each index stream for its planned parts.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_coder_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    const size_t per_case = 8;
    if (tok.empty() || tok.size() % per_case != 0) {
        fprintf(stderr, "coder_plan_main: %zu numbers, expected a multiple of %zu\n", tok.size(), per_case);
        return 2;
    }
    for (size_t at = 0; at < tok.size(); at += per_case) {
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        cgic::CompressShape s;
        s.B = num(0); s.h = num(1); s.w = num(2); s.slot = num(3); s.max_len = (int)num(4); s.nsym = (int)num(5);
        s.has_hist = num(6) != 0; s.has_workspace = num(7) != 0;
        cgic::CompressPlan p;
        const char *why = "";
        const int rc = cgic::compress_plan(s, &p, &why);
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        long long per[3];
        for (int g = 0; g < 3; ++g) per[g] = (long long)cgic::enc_part_positions((s.h >> (2 - g)) * (s.w >> (2 - g)), p.parts[g]);
        printf("parts_c=%d parts_m=%d parts_f=%d stage=%lld dyn_lds=%zu tickets=%d combine=%d jobs=%u small=%d parts_fastest=%d "
               "recorded=%d ws_stride=%zu ws_bytes=%zu ws_sym_offset=%zu slot_need=%zu capacity=%zu stream_ws=%zu per_c=%lld per_m=%lld "
               "per_f=%lld\n",
               p.parts[0], p.parts[1], p.parts[2], (long long)p.stage_positions, p.dyn_lds, p.tickets, p.combine, p.jobs, (int)p.small,
               (int)p.parts_fastest, (int)p.recorded, p.ws.stride, p.ws.bytes, p.ws.sym_offset,
               cgic::compress_slot_bytes(s.max_len, s.h, s.w), cgic::stream_capacity(s.max_len, s.h * s.w),
               cgic::stream_workspace_bytes(s.h * s.w), per[0], per[1], per[2]);
    }
    return 0;
}
