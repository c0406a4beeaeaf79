// poisson_accept.cpp -- PoissonAccept::consume (poisson_accept.h): plain C++, linked alone by
// tests/poisson_accept_host.
#include "poisson_accept.h"

#include <cmath>

namespace mpss {

PoissonAccept::State PoissonAccept::consume(const SurfacePoint *cand, const int *cnt, int batch,
                                            int batches, int stride) {
    auto cell = [&](float x) { return (int64_t)std::floor((double)x / (double)md); };
    auto key = [](int64_t x, int64_t y, int64_t z) {
        return ((uint64_t)(x & 0x1fffff) << 42) | ((uint64_t)(y & 0x1fffff) << 21) | (uint64_t)(z & 0x1fffff);
    };
    bool done = false;
    for (int b = 0; b < batches && !done; ++b) {
        total_paths += batch;
        for (int i = b * batch; i < (b + 1) * batch && !done; ++i)
            for (int j = 0; j < cnt[i] && !done; ++j) {
                SurfacePoint sp = cand[(size_t)i * stride + j];
                const int64_t cx = cell(sp.p[0]), cy = cell(sp.p[1]), cz = cell(sp.p[2]);
                bool fail = false;
                for (int dz = -1; dz <= 1 && !fail; ++dz)
                    for (int dy = -1; dy <= 1 && !fail; ++dy)
                        for (int dx = -1; dx <= 1 && !fail; ++dx) {
                            auto it = grid.find(key(cx + dx, cy + dy, cz + dz));
                            if (it == grid.end()) continue;
                            for (uint32_t q : it->second) {
                                const SurfacePoint &o = points[q];
                                const float ex = o.p[0] - sp.p[0], ey = o.p[1] - sp.p[1], ez = o.p[2] - sp.p[2];
                                if (ex * ex + ey * ey + ez * ez < md2) {
                                    fail = true;
                                    break;
                                }
                            }
                        }
                if (fail) {
                    if (++repeated_fails >= max_fails) done = true;
                } else {
                    repeated_fails = 0;
                    sp.area = area;
                    grid[key(cx, cy, cz)].push_back((uint32_t)points.size());
                    points.push_back(sp);
                }
            }
        // Warning + return, as FindPoissonPointDistribution (surfacepoints.cpp:277-281)
        if (!done && total_paths > 50000 && points.empty()) return State::GaveUp;
    }
    return done ? State::Done : State::GoOn;
}

}  // namespace mpss
