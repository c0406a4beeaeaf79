// The pixel-filter host unit (csrc/pixel_filter.cpp) and the tile planner's halo overload
// (csrc/tile_plan.cpp) on the CPU: plain C++, no libmpss, no HIP runtime, no GPU. Reads one command per
// line from the file named on the command line and answers each with one JSON line. Floats travel as
// their 32-bit patterns (decimal), so nothing is lost in text.
//   defaults kind                         -> [kind, xwidth, ywidth, a, b, is_default]
//   invalid kind xw yw a b                -> "" or the reason
//   table kind xw yw a b                  -> 256 weights
//   extent kind xw yw a b W H             -> [xs, xe, ys, ye, rx, ry]
//   ranges w res n X...                   -> per X: [lo, hi, idx(lo), ..., idx(hi)]
//   keys kind xw yw a b W H               -> per pixel of the sample extent, row-major: its key; then
//                                            1 when every key maps back to its pixel
//   plan kind xw yw a b W H spp max_batch filtered nrects rects...   (filtered 1: planned with the filter's
//                                            halo, filter_plan_halo; 0: plan_tiles without a halo)
//                                         -> pieces [x0, x1, y0, y1, ex0, ey0, ew, eh, nsamples, rect, out_off]
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "pixel_filter.h"
#include "tile_plan.h"

using namespace mpss;

static float f_of(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static uint32_t u_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
static PixelFilter read_filter(std::istream &in) {
    PixelFilter f;
    uint32_t xw, yw, a, b;
    in >> f.kind >> xw >> yw >> a >> b;
    f.xwidth = f_of(xw);
    f.ywidth = f_of(yw);
    f.a = f_of(a);
    f.b = f_of(b);
    return f;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream file(argv[1]);
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "defaults") {
            int kind;
            in >> kind;
            const PixelFilter f = filter_defaults(kind);
            printf("[%d, %u, %u, %u, %u, %d]\n", f.kind, u_of(f.xwidth), u_of(f.ywidth), u_of(f.a), u_of(f.b),
                   (int)f.is_default());
        } else if (cmd == "invalid") {
            const PixelFilter f = read_filter(in);
            const char *why = filter_invalid(f);
            printf("\"%s\"\n", why ? why : "");
        } else if (cmd == "table") {
            const PixelFilter f = read_filter(in);
            float t[kFilterTableSize * kFilterTableSize];
            filter_table(f, t);
            printf("[");
            for (int i = 0; i < kFilterTableSize * kFilterTableSize; ++i) printf("%s%u", i ? ", " : "", u_of(t[i]));
            printf("]\n");
        } else if (cmd == "extent") {
            const PixelFilter f = read_filter(in);
            int W, H;
            in >> W >> H;
            const SampleExtent e = filter_sample_extent(f, W, H);
            const FilmFilter ff = film_filter(f, W, H);
            if (ff.g.xs != e.xs || ff.g.xe != e.xe || ff.g.ys != e.ys || ff.g.ye != e.ye) return 3;
            printf("[%d, %d, %d, %d, %d, %d]\n", e.xs, e.xe, e.ys, e.ye, filter_halo(f.xwidth), filter_halo(f.ywidth));
        } else if (cmd == "ranges") {
            uint32_t wb;
            int res, n;
            in >> wb >> res >> n;
            const float w = f_of(wb), inv = 1.f / w;
            printf("[");
            for (int i = 0; i < n; ++i) {
                uint32_t xb;
                in >> xb;
                const float X = f_of(xb);
                int lo, hi;
                filter_range(X, w, res, lo, hi);
                printf("%s[%d, %d", i ? ", " : "", lo, hi);
                for (int x = lo; x <= hi; ++x) printf(", %d", filter_index(x, X - 0.5f, inv));
                printf("]");
            }
            printf("]\n");
        } else if (cmd == "keys") {
            const PixelFilter f = read_filter(in);
            int W, H;
            in >> W >> H;
            const FilmFilter ff = film_filter(f, W, H);
            int back = 1;
            printf("[");
            for (int y = ff.g.ys; y < ff.g.ye; ++y)
                for (int x = ff.g.xs; x < ff.g.xe; ++x) {
                    const uint32_t key = filter_pixel_key(ff.g, W, H, x, y);
                    int bx, by;
                    filter_key_pixel(ff.g, W, H, key, bx, by);
                    back &= bx == x && by == y;
                    printf("%u, ", key);
                }
            printf("%d]\n", back);
        } else if (cmd == "plan") {
            const PixelFilter f = read_filter(in);
            int W, H, spp, filtered, n;
            long long max_batch;
            in >> W >> H >> spp >> max_batch >> filtered >> n;
            std::vector<int32_t> rects(4 * (size_t)n);
            for (int32_t &v : rects) in >> v;
            const TilePlan plan = filtered ? plan_tiles(W, H, spp, 7u, n, rects.data(), max_batch, false, 0, 0,
                                                        filter_plan_halo(f, W, H))
                                           : plan_tiles(W, H, spp, 7u, n, rects.data(), max_batch, false, 0, 0);
            printf("[");
            for (size_t i = 0; i < plan.pieces.size(); ++i) {
                const PlanPiece &p = plan.pieces[i];
                printf("%s[%d, %d, %d, %d, %d, %d, %d, %d, %lld, %d, %zu]", i ? ", " : "", p.tb.x0, p.tb.x1, p.tb.y0,
                       p.tb.y1, p.tb.ex0, p.tb.ey0, p.tb.ew, p.tb.eh, (long long)p.tb.nsamples, p.rect, p.out_off);
            }
            printf("]\n");
        } else if (!cmd.empty()) {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
