// device_octree.h -- the device copy of the irradiance-point octree (octree.h) and its group-major
// band layouts, as every Mo() gather reads them (device_octree.hip; built on the device by octree_gpu.hip).
#pragma once
#include <memory>
#include <vector>

#include "common.h"
#include "common_grid_types.h"
#include "octree.h"

namespace mpss {

// The group-major copy of the octree's E/Et rows for one band grouping (mo_band.h): et[g][node],
// e[g][point] = the 4 bands of group g as a float4.
struct BandLayout {
    BandGroups groups{};
    DevBuf<float4> et, e;
    DevBuf<float4> ew;  // e scaled by each point's area (the common-grid gather's products, mo_band.h)
};

struct DeviceOctree {
    DevBuf<NodeHdr> nodes;
    DevBuf<float> node_et;
    DevBuf<float4> pt_hdr;
    DevBuf<float> pt_e;
    DevBuf<int> pt_index;  // original point index of every point slot
    int n_nodes = 0, n_points = 0, max_depth = 0;
    float bmin[3] = {0.f, 0.f, 0.f}, bmax[3] = {0.f, 0.f, 0.f};  // root bounds (query sort keys)
    // one group-major layout per distinct band grouping in use; built eagerly and synchronously
    // (Context::set_irradiance_points / add material) so launches only read them
    std::vector<std::unique_ptr<BandLayout>> layouts;
    // per node: for a leaf, the square of a radius around its centroid that holds every point of the
    // leaf as seen from any query that opens it under max_error (DiffusionOctree Mo(): d^2 <= sumArea /
    // maxError, or the query inside the leaf's box): max(sqrt(sumArea / maxError), diag) + diag,
    // squared, rounded up; +inf for interior nodes and leaves without a finite centroid. Lets the
    // sharded gather prove a leaf's point lookups lie in its LDS near field. Valid for
    // leaf_r2_error == the gather's max_error. The gather reads it as a 16-bit code in the node's
    // header (NodeHdr::pad's high half, rounded up; ensure_leaf_r2 writes both).
    DevBuf<float> leaf_r2;
    float leaf_r2_error = -1.f;
    void ensure_leaf_r2(float max_error);  // synchronous
    void upload(const FlatOctree &t);      // the tree in device order (octree.h device_order)
    const BandLayout *find_layout(const BandGroups &g) const;
    // builds the layout if it is missing (synchronizes the device); the caller serializes calls
    const BandLayout &ensure_layout(const BandGroups &g);
};

// SubsurfaceOctreeNode::Insert + InitHierarchy on the device (octree_gpu.hip): the tree of the host
// build (octree.cpp) + DeviceOctree::upload, bit for bit. P, N: n x 3, E: n x NB, A: n device floats;
// bmin / bmax: the points' bounds (Union of the points in index order). Synchronous.
void build_octree_device(int n, const float *P, const float *N, const float *E, const float *A, const float bmin[3],
                         const float bmax[3], DeviceOctree &t);

}  // namespace mpss
