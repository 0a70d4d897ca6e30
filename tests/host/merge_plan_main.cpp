// merge_plan_main.cpp -- prints the launch plan of the merge / pool / blend calls (csrc/cgic_merge_plan.h) for the cases it is
// given (no GPU, no library).  A case is 16 numbers, from the arguments or, without arguments, from stdin:
//   op in_dtype out_dtype B C h w k feat0 feat1 feat2 mask0 mask1 mask2 out entry
// (op: 0 merge, 1 pool, 2 medium blend, 3 fine blend; the seven addresses as plain integers, 0 = NULL; entry: 0 the _h call,
// 1 the _f32 call).
// One line per case: the plan's fields as name=value, or err=<code> and the reason.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_merge_plan.h"
#include "../../include/cgic_hip.h"

int main(int argc, char **argv)
{
    std::vector<std::string> tok;
    for (int i = 1; i < argc; ++i) tok.push_back(argv[i]);
    if (argc == 1) {
        char buf[64];
        while (scanf("%63s", buf) == 1) tok.push_back(buf);
    }
    const size_t per_case = 16;
    if (tok.empty() || tok.size() % per_case != 0) {
        fprintf(stderr, "merge_plan_main: %zu numbers, expected a multiple of %zu\n", tok.size(), per_case);
        return 2;
    }
    for (size_t at = 0; at < tok.size(); at += per_case) {
        const auto num = [&](int i) { return strtoll(tok[at + i].c_str(), nullptr, 10); };
        cgic::MergeCall c{};
        c.op = (int)num(0); c.in_dtype = (int)num(1); c.out_dtype = (int)num(2);
        c.B = num(3); c.C = (int)num(4); c.h = num(5); c.w = num(6); c.k = (int)num(7);
        for (int i = 0; i < 3; ++i) { c.feat[i] = (uintptr_t)num(8 + i); c.mask[i] = (uintptr_t)num(11 + i); }
        c.out = (uintptr_t)num(14); c.entry = (int)num(15);
        cgic::MergePlan p;
        const char *why = "";
        const int rc = cgic::merge_plan(c, &p, &why);
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, why);
            continue;
        }
        printf("unit=%d threads=%d grid=%d total=%lld in_place=%d ntensors=%d\n", p.unit, p.threads, p.grid, (long long)p.total,
               (int)p.in_place, p.ntensors);
    }
    return 0;
}
