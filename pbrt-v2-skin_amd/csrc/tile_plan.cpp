// tile_plan.cpp -- the host planner of render_tiles (tile_plan.h).
#include "tile_plan.h"

#include <algorithm>

namespace mpss {

bool tile_rect_ok(const int32_t *r, int W, int H) {
    return !(r[0] < 0 || r[2] < 0 || r[1] > W || r[3] > H || r[0] >= r[1] || r[2] >= r[3]);
}

TilePlan plan_tiles(int W, int H, int spp, uint32_t seed, int n, const int32_t *rects, int64_t max_batch,
                    bool replay, int replay_k, int64_t window_limit) {
    return plan_tiles(W, H, spp, seed, n, rects, max_batch, replay, replay_k, window_limit, PlanHalo{1, 1, 0, W, 0, H});
}

TilePlan plan_tiles(int W, int H, int spp, uint32_t seed, int n, const int32_t *rects, int64_t max_batch,
                    bool replay, int replay_k, int64_t window_limit, const PlanHalo &halo) {
    TilePlan plan;
    std::vector<PlanPiece> &pieces = plan.pieces;
    // replay: rectangles in row order, so that consecutive batches continue the task streams
    // (replay_window) and a batch's window stays compact
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    if (replay)
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
            return rects[4 * a + 2] != rects[4 * b + 2] ? rects[4 * a + 2] < rects[4 * b + 2]
                                                        : rects[4 * a] < rects[4 * b];
        });
    // cut rectangles into pieces of <= max_batch samples
    for (int i : order) {
        const int x0 = rects[4 * i], x1 = rects[4 * i + 1], y0 = rects[4 * i + 2], y1 = rects[4 * i + 3];
        const int tw = x1 - x0;
        const int ex0 = std::max(x0 - halo.rx, halo.xs);
        const int ew = std::min(x1 + halo.rx, halo.xe) - ex0;
        const int rows = (int)std::max<int64_t>(1, max_batch / ((int64_t)ew * spp) - 2 * halo.ry);
        for (int yb = y0; yb < y1; yb += rows) {
            const int ye = std::min(y1, yb + rows);
            PlanPiece p;
            p.tb.x0 = x0;
            p.tb.x1 = x1;
            p.tb.y0 = yb;
            p.tb.y1 = ye;
            p.tb.ex0 = ex0;
            p.tb.ey0 = std::max(yb - halo.ry, halo.ys);
            p.tb.ew = ew;
            p.tb.eh = std::min(ye + halo.ry, halo.ye) - p.tb.ey0;
            p.tb.spp = spp;
            p.tb.seed = seed;
            p.tb.nsamples = (int64_t)p.tb.ew * p.tb.eh * spp;
            p.rect = i;
            p.out_off = (size_t)(yb - y0) * tw * 4;
            pieces.push_back(p);
        }
    }
    size_t pi = 0;
    // replay: the current generated window (it may span several batches: one generation over
    // more tasks keeps more waves in flight, replay_gen.hip)
    bool have_win = false;
    int wx0 = 0, wx1 = 0, wy0 = 0, wy1 = 0;
    while (pi < pieces.size()) {
        // pack pieces into one batch
        size_t pe = pi;
        int64_t total = 0;
        // replay: the batch's window (the pieces' bounding box) holds spp x replay_k floats per
        // pixel; kept to <= window_limit
        int bx0 = INT32_MAX, bx1 = 0, by0 = INT32_MAX, by1 = 0;
        auto fits = [&](const TileBatch &tb) {
            if (!replay) return true;
            const int64_t w = std::max(bx1, tb.ex0 + tb.ew) - std::min(bx0, tb.ex0);
            const int64_t h = std::max(by1, tb.ey0 + tb.eh) - std::min(by0, tb.ey0);
            return w * h * spp * replay_k <= window_limit;
        };
        while (pe < pieces.size() &&
               (pe == pi || (total + pieces[pe].tb.nsamples <= max_batch && fits(pieces[pe].tb)))) {
            const TileBatch &tb = pieces[pe].tb;
            bx0 = std::min(bx0, tb.ex0);
            bx1 = std::max(bx1, tb.ex0 + tb.ew);
            by0 = std::min(by0, tb.ey0);
            by1 = std::max(by1, tb.ey0 + tb.eh);
            total += pieces[pe++].tb.nsamples;
        }
        bool new_window = false;
        if (replay && (!have_win || bx0 < wx0 || bx1 > wx1 || by0 < wy0 || by1 > wy1)) {
            // the reference sampler's values over a new window: this batch's pieces and the
            // following ones, as far as the window table allows (window_limit)
            int gx0 = bx0, gx1 = bx1, gy0 = by0, gy1 = by1;
            for (size_t k = pe; k < pieces.size(); ++k) {
                const TileBatch &tb = pieces[k].tb;
                const int nx0 = std::min(gx0, tb.ex0), nx1 = std::max(gx1, tb.ex0 + tb.ew);
                const int ny0 = std::min(gy0, tb.ey0), ny1 = std::max(gy1, tb.ey0 + tb.eh);
                if ((int64_t)(nx1 - nx0) * (ny1 - ny0) * spp * replay_k > window_limit) break;
                gx0 = nx0;
                gx1 = nx1;
                gy0 = ny0;
                gy1 = ny1;
            }
            new_window = have_win = true;
            wx0 = gx0;
            wx1 = gx1;
            wy0 = gy0;
            wy1 = gy1;
        }
        plan.batches.push_back(PlanBatch{pi, pe, total, bx0, bx1, by0, by1, new_window, wx0, wx1, wy0, wy1});
        pi = pe;
    }
    return plan;
}

std::vector<LaunchGroup> launch_groups(const TilePlan &plan, const PlanBatch &b, bool film, int film_tile) {
    std::vector<LaunchGroup> groups;
    int64_t off = 0;
    for (size_t k0 = b.first; k0 < b.end; k0 += kMaxPieces) {
        LaunchGroup g{};
        g.first = k0;
        int blocks = 0;
        for (size_t k = k0; k < b.end && k < k0 + kMaxPieces; ++k) {
            const TileBatch &tb = plan.pieces[k].tb;
            const int j = g.n++;
            const int tw = tb.x1 - tb.x0;
            const int64_t items = film ? (int64_t)tw * (tb.y1 - tb.y0) : tb.nsamples;
            g.block0[j] = blocks;
            g.off[j] = off;
            g.out_stride[j] = tw;
            if (film && film_tile > 0)
                blocks += ((tw + film_tile - 1) / film_tile) * ((tb.y1 - tb.y0 + film_tile - 1) / film_tile);
            else
                blocks += (int)((items + 255) / 256);
            off += tb.nsamples;
        }
        g.block0[g.n] = g.blocks = blocks;
        groups.push_back(g);
    }
    return groups;
}

}  // namespace mpss
