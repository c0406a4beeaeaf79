// scene_plain.h -- the records of scene.h that plain C++ reads (no HIP runtime, no device pointers):
// BvhNode with thread_bvh, and SurfacePoint. scene.h includes it; a CPU program can link scene_plain.cpp
// and poisson_accept.cpp alone (tests/thread_bvh_host, tests/poisson_accept_host).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mpss {

// Linear BVH node (accelerators/bvh.cpp:113-123 layout): 32 B.
struct alignas(16) BvhNode {
    float bmin[3];
    int32_t offset;  // leaf: first primitive; interior: second child index
    float bmax[3];
    uint16_t nprims;  // 0 for interior
    uint16_t axis;
};
static_assert(sizeof(BvhNode) == 32, "BvhNode is 32 B");

// The threaded copy for stackless any-hit walks (bvh_trace.h): the nodes are in pre-order (a node's
// subtree is [i, end_i)), so an interior node's offset becomes end_i -- where a walk continues after
// missing it; a leaf's end is i + 1, and leaves are copied as they are.
std::vector<BvhNode> thread_bvh(const std::vector<BvhNode> &bvh);

// SurfacePoint (renderers/surfacepoints.h:45-55): p, n, u, v, materialId, area, rayEpsilon.
struct SurfacePoint {
    float p[3], n[3], u, v;
    uint32_t material;
    float area, ray_eps;
};
static_assert(sizeof(SurfacePoint) == 44, "SurfacePoint matches the reference's 44-B pointsfile record");

}  // namespace mpss
