// tiles_plan_main.cpp -- runs the launch plans of cgic_cut_tiles / cgic_paste_tiles / cgic_partition_map (csrc/cgic_tiles_plan.h) for
// the cases it is given on stdin (no GPU, no library).  One case per line, one output line per case:
//   K y0 x0 th tw H W                        -> clip=y0,y1,x0,x1 empty=<0|1>
//   D H W n  (y0 x0 th tw) x n               -> apart=1   or   apart=0 j=.. k=..
//   C u8 N H W n  (y0 x0 th tw) x n          -> total=.. blocks=.. gy=.. first=a,b,..                    or  err=<code> why=<NAME> j=.. k=..
//   P N H W n  (y0 x0 th tw stride w) x n    -> most=.. blocks=.. gy=.. gz=.. stride4=a,b,..             or  err=.. why=.. j=.. k=..
//                                               w: 0 = no weights, 1 = wx and wy, 2 = wx only, 3 = wy only
//   M u8 N H W alias n  (form y0 x0 th tw gh gw) x n
//                                            -> masks=<0|1> most=.. blocks=.. gy=.. gz=.. grid=ghxgw,..  or  err=.. why=.. j=.. k=..
//                                               form: m = the three masks, i = the indices, b = both, n = neither
//                                               alias: 0 = three images apart, 1 = out_f32 is src, 2 = out_f32 16 bytes into src,
//                                                      3 = out_u8 is src (another layout unless u8), 4 = out_u8 64 bytes into out_f32
// A tile left out of a long table repeats the last one given, 16 pixels further right.  The addresses are made-up aligned numbers: the
// plans never dereference them.
#include <stdio.h>

#include <sstream>
#include <string>
#include <vector>

#include "../../control-gic_amd/csrc/cgic_tiles_plan.h"

using namespace cgic;

struct Rect { int y0 = 0, x0 = 0, th = 16, tw = 16; };

static bool rect(std::istringstream &in, Rect *r)
{
    Rect t;
    if (in >> t.y0 >> t.x0 >> t.th >> t.tw) { *r = t; return true; }
    in.clear();
    r->x0 += 16;
    return false;
}

template <class V>
static void list(const char *key, const V *v, int n)
{
    printf(" %s=", key);
    for (int k = 0; k < n; ++k) printf(k ? ",%u" : "%u", (unsigned)v[k]);
}

static int refused(int rc, const TilesFault &f)
{
    if (rc != CGIC_OK) printf("err=%d why=%s j=%d k=%d\n", rc, tiles_why_name(f.why), f.j, f.k);
    return rc;
}

int main()
{
    static char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string kind;
        if (!(in >> kind)) continue;
        long long N = 1, H = 0, W = 0;
        int n = 0, u8 = 0;
        TilesFault f;
        if (kind == "K") {
            Rect r;
            in >> r.y0 >> r.x0 >> r.th >> r.tw >> H >> W;
            const TileClip c = tile_clip(r.y0, r.x0, r.th, r.tw, H, W);
            printf("clip=%lld,%lld,%lld,%lld empty=%d\n", (long long)c.y0, (long long)c.y1, (long long)c.x0, (long long)c.x1, (int)c.empty);
        } else if (kind == "D") {
            in >> H >> W >> n;
            std::vector<TileClip> c;                       // (exact size: the address sanitizer sees a read past the table)
            Rect r;
            for (int k = 0; k < n; ++k) { rect(in, &r); c.push_back(tile_clip(r.y0, r.x0, r.th, r.tw, H, W)); }
            int j = -1, k = -1;
            if (tiles_disjoint(c.data(), n, &j, &k)) printf("apart=1\n");
            else printf("apart=0 j=%d k=%d\n", j, k);
        } else if (kind == "C") {
            in >> u8 >> N >> H >> W >> n;
            std::vector<cgic_tile> t;
            Rect r;
            for (int k = 0; k < n; ++k) {
                rect(in, &r);
                t.push_back(cgic_tile{(void *)(uintptr_t)0x100000, 3LL * r.th * r.tw, r.y0, r.x0, r.th, r.tw});
            }
            CutPlan p;
            if (refused(cut_plan(u8, N, H, W, n, t.data(), &p, &f), f)) continue;
            printf("total=%u blocks=%u gy=%lld", p.total, p.blocks, N);
            list("first", p.first, n);
            printf("\n");
        } else if (kind == "P") {
            in >> N >> H >> W >> n;
            std::vector<cgic_paste_tile> t;
            Rect r;
            long long stride = 768, w = 1;
            for (int k = 0; k < n; ++k) {
                if (rect(in, &r)) in >> stride >> w;
                t.push_back(cgic_paste_tile{(const float *)(uintptr_t)0x100000, stride, (const double *)(uintptr_t)(w == 1 || w == 2 ? 0x200000 : 0),
                                            (const double *)(uintptr_t)(w == 1 || w == 3 ? 0x300000 : 0), r.y0, r.x0, r.th, r.tw});
            }
            PastePlan p;
            if (refused(paste_plan(N, H, W, n, t.data(), &p, &f), f)) continue;
            printf("most=%u blocks=%u gy=%d gz=%lld", p.most, p.blocks, n, N);
            list("stride4", p.stride4, n);
            printf("\n");
        } else if (kind == "M") {
            int alias = 0;
            in >> u8 >> N >> H >> W >> alias >> n;
            std::vector<cgic_partition_tile> t;
            Rect r;
            std::string form = "m";
            int gh = 0, gw = 0;
            for (int k = 0; k < n; ++k) {
                std::string fm;
                if (in >> fm) { form = fm; rect(in, &r); in >> gh >> gw; }
                else { in.clear(); r.x0 += 16; }
                const bool m = form == "m" || form == "b", i = form == "i" || form == "b";
                t.push_back(cgic_partition_tile{(const int32_t *)(uintptr_t)(m ? 0x400000 : 0), (const int32_t *)(uintptr_t)(m ? 0x410000 : 0),
                                                (const int32_t *)(uintptr_t)(m ? 0x420000 : 0), (const int64_t *)(uintptr_t)(i ? 0x430000 : 0), 1,
                                                r.y0, r.x0, r.th, r.tw, gh, gw});
            }
            const uintptr_t src = 0x10000000, far = 0x40000000;
            const float *o32 = (const float *)(alias == 1 ? src : alias == 2 ? src + 16 : alias == 3 ? 0 : far);
            const unsigned char *o8 = (const unsigned char *)(alias == 3 ? src : alias == 4 ? far + 64 : (uintptr_t)0);
            PartitionPlan p;
            if (refused(partition_plan((const void *)src, u8, N, H, W, n, t.data(), o32, o8, &p, &f), f)) continue;
            printf("masks=%d most=%u blocks=%u gy=%d gz=%lld grid=", (int)p.masks_form, p.most, p.blocks, n, N);
            for (int k = 0; k < n; ++k) printf(k ? ",%ux%u" : "%ux%u", (unsigned)p.gh[k], (unsigned)p.gw[k]);
            printf("\n");
        } else {
            printf("err=0 why=unknown-case j=0 k=0\n");
        }
    }
    return 0;
}
