// The render_tiles planner on the CPU (tests/test_tile_plan.py builds this with csrc/tile_plan.cpp alone, under
// ASan + UBSan). Reads cases from the file named on the command line, one per line:
//   W H spp seed max_batch replay replay_k window_limit n  x0 x1 y0 y1 (n times)
// and prints each case's plan as one JSON line:
//   pieces   [x0, x1, y0, y1, ex0, ey0, ew, eh, spp, seed, nsamples, rect, out_off]
//   batches  [first, end, total, bx0, bx1, by0, by1, new_window, wx0, wx1, wy0, wy1]
//   launches per batch [primary groups, film groups], a group = [first, n, [block0 x (n + 1)], [off x n],
//            [out_stride x n]]
// With "rects" before the file name, the lines are  W H x0 x1 y0 y1  and the output is tile_rect_ok of each, 0 or 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tile_plan.h"

using namespace mpss;

static void print_groups(const TilePlan &plan, const PlanBatch &b, bool film) {
    const std::vector<LaunchGroup> groups = launch_groups(plan, b, film);
    printf("[");
    for (size_t g = 0; g < groups.size(); ++g) {
        const LaunchGroup &lg = groups[g];
        if (lg.blocks != lg.block0[lg.n]) {
            fprintf(stderr, "group %zu: blocks %d != block0[n] %d\n", g, lg.blocks, lg.block0[lg.n]);
            exit(2);
        }
        printf("%s[%zu,%d,[", g ? "," : "", lg.first, lg.n);
        for (int j = 0; j <= lg.n; ++j) printf("%s%d", j ? "," : "", lg.block0[j]);
        printf("],[");
        for (int j = 0; j < lg.n; ++j) printf("%s%lld", j ? "," : "", (long long)lg.off[j]);
        printf("],[");
        for (int j = 0; j < lg.n; ++j) printf("%s%d", j ? "," : "", lg.out_stride[j]);
        printf("]]");
    }
    printf("]");
}

int main(int argc, char **argv) {
    const bool rects_only = argc == 3 && !strcmp(argv[1], "rects");
    if (argc != 2 && !rects_only) {
        fprintf(stderr, "usage: tile_plan_host [rects] CASES\n");
        return 2;
    }
    FILE *f = fopen(argv[argc - 1], "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[argc - 1]);
        return 2;
    }
    if (rects_only) {
        int W, H;
        int32_t r[4];
        while (fscanf(f, "%d %d %d %d %d %d", &W, &H, &r[0], &r[1], &r[2], &r[3]) == 6)
            printf("%d\n", tile_rect_ok(r, W, H) ? 1 : 0);
        fclose(f);
        return 0;
    }
    int W, H, spp, n, replay, replay_k;
    unsigned seed;
    long long max_batch, window_limit;
    while (fscanf(f, "%d %d %d %u %lld %d %d %lld %d", &W, &H, &spp, &seed, &max_batch, &replay, &replay_k,
                  &window_limit, &n) == 9) {
        std::vector<int32_t> rects(4 * (size_t)n);
        for (int32_t &v : rects)
            if (fscanf(f, "%d", &v) != 1) {
                fprintf(stderr, "short case\n");
                return 2;
            }
        const TilePlan plan =
            plan_tiles(W, H, spp, seed, n, rects.data(), max_batch, replay != 0, replay_k, window_limit);
        printf("{\"pieces\":[");
        for (size_t k = 0; k < plan.pieces.size(); ++k) {
            const PlanPiece &p = plan.pieces[k];
            const TileBatch &t = p.tb;
            printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%u,%lld,%d,%zu]", k ? "," : "", t.x0, t.x1, t.y0, t.y1, t.ex0, t.ey0,
                   t.ew, t.eh, t.spp, t.seed, (long long)t.nsamples, p.rect, p.out_off);
        }
        printf("],\"batches\":[");
        for (size_t k = 0; k < plan.batches.size(); ++k) {
            const PlanBatch &b = plan.batches[k];
            printf("%s[%zu,%zu,%lld,%d,%d,%d,%d,%d,%d,%d,%d,%d]", k ? "," : "", b.first, b.end, (long long)b.total,
                   b.bx0, b.bx1, b.by0, b.by1, b.new_window ? 1 : 0, b.wx0, b.wx1, b.wy0, b.wy1);
        }
        printf("],\"launches\":[");
        for (size_t k = 0; k < plan.batches.size(); ++k) {
            printf("%s[", k ? "," : "");
            print_groups(plan, plan.batches[k], false);
            printf(",");
            print_groups(plan, plan.batches[k], true);
            printf("]");
        }
        printf("]}\n");
    }
    fclose(f);
    return 0;
}
