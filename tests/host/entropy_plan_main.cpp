// entropy_plan_main.cpp -- runs the argument checks and the launch geometry of the entropy-map entry points (cgic_entropy_plan.h)
// over the cases it is given (no GPU, no library).  One case per line, from stdin or, as one case, from the arguments:
//   setup  nbins sigma window bins[32]          window: 2 = "2-bin", 5 = "five-bin"; the nbins check, then sigma and the bin centres
//   image  B H W                                the image form's shape check
//   tiles  N H W T th tw [origins: 2 T numbers] the tiles form's shape check, then the origins if they are given
//   plan   H W images ppw sigma has_outputs     the grid and the exp2 scale (as the bit pattern of the float)
// One line per case: ok, name=value fields, or err=<code> and the message.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_entropy_plan.h"
#include "../../include/cgic_hip.h"

static int fail(int rc, const cgic::EntropyWhy &why)
{
    printf("err=%d why=%s\n", rc, why.text);
    return rc;
}

static int run(const std::vector<std::string> &t)
{
    const auto num = [&](size_t i) { return strtoll(t[i].c_str(), nullptr, 10); };
    const auto flt = [&](size_t i) { return strtof(t[i].c_str(), nullptr); };
    cgic::EntropyWhy why;
    int rc;
    if (t[0] == "setup" && t.size() == 4 + (size_t)cgic::kBins) {
        float bins[cgic::kBins];
        for (int i = 0; i < cgic::kBins; ++i) bins[i] = flt(4 + i);
        if ((rc = cgic::entropy_nbins_check((int)num(1), &why))) return fail(rc, why);
        if ((rc = cgic::entropy_setup_check(flt(2), bins, num(3) == 5 ? "five-bin" : "2-bin", &why))) return fail(rc, why);
    } else if (t[0] == "image" && t.size() == 4) {
        if ((rc = cgic::entropy_shape_check(num(1), num(2), num(3), &why))) return fail(rc, why);
    } else if (t[0] == "tiles" && t.size() >= 7) {
        const int T = (int)num(4);
        if ((rc = cgic::entropy_shape_check(num(1), num(2), num(3), T, num(5), num(6), &why))) return fail(rc, why);
        if (t.size() > 7) {
            if (t.size() != 7 + 2 * (size_t)T) return 2;
            std::vector<int> org;
            for (size_t i = 7; i < t.size(); ++i) org.push_back((int)num(i));
            if ((rc = cgic::entropy_origins_check(T, org.data(), &why))) return fail(rc, why);
        }
    } else if (t[0] == "plan" && t.size() == 7) {
        const cgic::EntropyPlan p = cgic::entropy_plan(num(1), num(2), num(3), (int)num(4), flt(5), num(6) != 0);
        unsigned int bits;
        memcpy(&bits, &p.exp2_scale, sizeof(bits));
        printf("nothing=%d gx=%u gy=%u gz=%u exp2_scale_bits=%u\n", (int)p.nothing, p.gx, p.gy, p.gz, bits);
        return 0;
    } else {
        return 2;
    }
    printf("ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    std::vector<std::vector<std::string>> cases;
    if (argc > 1) {
        cases.emplace_back(argv + 1, argv + argc);
    } else {
        char line[4096];
        while (fgets(line, sizeof(line), stdin)) {
            std::istringstream in(line);
            std::vector<std::string> t;
            for (std::string w; in >> w;) t.push_back(w);
            if (!t.empty()) cases.push_back(t);
        }
    }
    for (const auto &t : cases)
        if (run(t) == 2) {
            fprintf(stderr, "entropy_plan_main: cannot read the case that starts with '%s' (%zu words)\n", t[0].c_str(), t.size());
            return 2;
        }
    return cases.empty() ? 2 : 0;
}
