// poisson_accept.h -- the host half of FindPoissonPointDistribution (renderers/surfacepoints.cpp:175-284,
// one SurfacePointTask): candidates in path order are accepted unless an accepted point lies within
// minDist (PoissonCheck: DistanceSquared < minDist^2; the reference's octree lookup finds exactly
// those), until maxFails candidates in a row fail. Plain C++ (no HIP, no device pointers), so a CPU
// program can link poisson_accept.cpp alone (tests/poisson_accept_host); find_poisson_points
// (preprocess_host.hip) traces the candidates on the GPU and feeds them here launch by launch.
#pragma once
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "scene_plain.h"

namespace mpss {

struct PoissonAccept {
    enum class State {
        GoOn,   // feed the next launch
        Done,   // max_fails candidates in a row failed
        GaveUp  // more than 50000 paths and not one point: the caller warns and returns
    };
    // area: what an accepted point's SurfacePoint::area becomes (pi (minDist / 2)^2 in the caller's float)
    PoissonAccept(float min_dist, int max_fails, float area)
        : md(min_dist), md2(min_dist * min_dist), area(area), max_fails(max_fails) {}
    // One launch's candidates: `batches` batches of `batch` paths; path i's candidates are
    // cand[i * stride ... + cnt[i]). Batches are taken in order, and Done cuts off at the candidate
    // that reached max_fails: nothing after it is looked at.
    State consume(const SurfacePoint *cand, const int *cnt, int batch, int batches, int stride);

    std::vector<SurfacePoint> points;  // accepted, in order
    int repeated_fails = 0;
    int64_t total_paths = 0;

private:
    const float md, md2, area;
    const int max_fails;
    // accepted points, bucketed by minDist cells
    std::unordered_map<uint64_t, std::vector<uint32_t>> grid;
};

}  // namespace mpss
