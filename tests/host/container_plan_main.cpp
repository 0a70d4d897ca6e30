// container_plan_main.cpp -- runs the launch plan of cgic_container_pack / _unpack (csrc/cgic_container_plan.h) for the cases it is
// given on stdin (no GPU, no library).  One case per line, one output line per case:
//   H E                                     -> header=<12 + 44 E> residue=<header % 16>
//   B G E  slot_0 .. slot_G-1               -> bound=<cgic_container_bound>
//   W E                                     -> ws=<bytes> off=.. words=.. ptr=.. len=..
//   P G E capacity  (B slot mode) x G  (group index) x E
//                                           -> header=.. streams=.. stage=.. words=.. blocks=..   or  err=<code> why=<text>
//   U G E  (B slot mode) x G  (group index) x E  <hex of the blob, or ->
//                                           -> the same fields
#include <stdio.h>
#include <stdlib.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_container_plan.h"

static const int kModeStreams[7] = {0x1F, 0x16, 0x0D, 0x0B, 0x01, 0x02, 0x04};

int main()
{
    // (the stream sets of the seven modes, model.py:225-260, bit i = stream i: what cgic_mode_streams returns; restated here
    // because this program links nothing)
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string kind;
        if (!(in >> kind)) continue;
        if (kind == "H") {
            long long E;
            in >> E;
            printf("header=%lld residue=%lld\n", (long long)cgic::container_header_bytes(E), (long long)(cgic::container_header_bytes(E) % 16));
            continue;
        }
        if (kind == "W") {
            long long E;
            in >> E;
            const cgic::ContainerWorkspace w = cgic::container_workspace(E);
            printf("ws=%zu off=%zu words=%zu ptr=%zu len=%zu\n", w.bytes, w.off, w.words, w.ptr, w.len);
            continue;
        }
        long long G, E;
        in >> G >> E;
        if (kind == "B") {
            std::vector<cgic_container_group> g((size_t)(G > 0 ? G : 0));
            for (auto &x : g) { long long s; in >> s; x = cgic_container_group{nullptr, nullptr, 1, s, 0}; }
            printf("bound=%zu\n", cgic::container_bound(g.data(), (int)G, E));
            continue;
        }
        long long capacity = 0;
        if (kind == "P") in >> capacity;
        // (tables as long as the case says, so that a count over the limit is refused by the plan and not by this program)
        std::vector<cgic_container_group> g((size_t)(G > 0 ? G : 0));
        for (auto &x : g) { long long b, s, m; in >> b >> s >> m; x = cgic_container_group{nullptr, nullptr, b, s, (int)m}; }
        std::vector<cgic_container_entry> e((size_t)(E > 0 ? E : 0));
        for (auto &x : e) {
            long long gi = 0, ix = 0;
            if (!(in >> gi >> ix)) { gi = 0; ix = 0; }          // (a long table may be left out: all entries (0, 0))
            x = cgic_container_entry{0, 0, 0, 0, 0, (int32_t)gi, (int32_t)ix};
        }
        cgic::ContainerPlan p;
        cgic::ContainerWhy why;
        int rc;
        if (kind == "P") {
            rc = cgic::container_pack_plan(g.data(), (int)G, e.data(), E, capacity, &p, &why);
        } else {
            std::string hex;
            in >> hex;
            std::vector<uint8_t> blob;
            if (hex != "-")
                for (size_t i = 0; i + 1 < hex.size(); i += 2) blob.push_back((uint8_t)strtol(hex.substr(i, 2).c_str(), nullptr, 16));
            // an exact-size heap copy: the address sanitizer then sees any read past the file
            uint8_t *exact = blob.empty() ? nullptr : (uint8_t *)malloc(blob.size());
            if (exact) memcpy(exact, blob.data(), blob.size());
            rc = cgic::container_unpack_plan(exact, (int64_t)blob.size(), g.data(), (int)G, e.data(), E, kModeStreams, &p, &why);
            free(exact);
        }
        if (rc != CGIC_OK) {
            printf("err=%d why=%s\n", rc, cgic::container_why_text(why));
            continue;
        }
        printf("header=%lld streams=%lld stage=%d words=%lld blocks=%lld ws=%zu\n", (long long)p.header_bytes, (long long)p.streams, p.stage_launches,
               (long long)p.copy_words, (long long)p.copy_blocks, p.ws.bytes);
    }
    return 0;
}
