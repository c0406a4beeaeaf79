// device_octree.hip -- DeviceOctree (device_octree.h): the upload of the host build in device order, the
// leaves' near-field bounds with their codes in the headers, and the group-major band layouts.
#include "device_octree.h"

#include <cmath>

namespace mpss {

void DeviceOctree::upload(const FlatOctree &t) {
    const DeviceOrder d = device_order(t);
    layouts.clear();
    leaf_r2_error = -1.f;
    nodes.upload(d.hdr.data(), d.hdr.size());
    node_et.upload(t.node_et.data(), t.node_et.size());
    pt_hdr.upload(reinterpret_cast<const float4 *>(d.pt_hdr.data()), d.pt_hdr.size() / 4);
    pt_e.upload(d.pt_e.data(), d.pt_e.size());
    pt_index.upload(d.pt_index.data(), d.pt_index.size());
    n_nodes = (int)t.hdr.size();
    n_points = (int)t.pt_index.size();
    max_depth = t.max_depth;
    for (int k = 0; k < 3; ++k) {
        bmin[k] = t.bmin[k];
        bmax[k] = t.bmax[k];
    }
}

namespace {
// Also writes the bound's leaf code into NodeHdr::pad's high half (its low half is the live point count):
// the bound's high 16 bits rounded up, so code < (lim's high 16 bits) => bound < lim -- the sharded
// gather's LDS-only leaf test is then one scalar compare on the header it has loaded anyway.
__global__ void leaf_r2_kernel(NodeHdr *__restrict__ nodes, int n, float max_error, float *__restrict__ r2) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const NodeHdr h = nodes[i];
    float out = INFINITY;
    if (h.leaf_first >= 0 && h.sum_area > 0.f && max_error > 0.f && isfinite(h.px) && isfinite(h.py) &&
        isfinite(h.pz)) {
        // A query opens the leaf only if |q - c| <= open (dw >= max_error) or q lies in the box. Every point
        // lies in the box, so |q - p_i| <= open + (c's farthest box corner) or <= diag. The centroid c is
        // luminance-weighted and need not lie in the box (mixed-sign E, or a zero weight sum leaving c at
        // the origin), hence the farthest corner from c rather than the diagonal.
        const double dx = (double)h.bmaxx - h.bminx, dy = (double)h.bmaxy - h.bminy, dz = (double)h.bmaxz - h.bminz;
        const double diag = sqrt(dx * dx + dy * dy + dz * dz);
        const double fx = fmax(fabs((double)h.px - h.bminx), fabs((double)h.px - h.bmaxx));
        const double fy = fmax(fabs((double)h.py - h.bminy), fabs((double)h.py - h.bmaxy));
        const double fz = fmax(fabs((double)h.pz - h.bminz), fabs((double)h.pz - h.bmaxz));
        const double corner = sqrt(fx * fx + fy * fy + fz * fz);
        const double open = sqrt((double)h.sum_area / (double)max_error) * (1.0 + 1e-6);
        const double R = (open + corner > diag ? open + corner : diag);
        out = (float)(R * R * (1.0 + 1e-6));
    }
    r2[i] = out;
    const uint32_t code = (__float_as_uint(out) + 0xffffu) >> 16;  // (out > 0; INF -> 0x7f80)
    nodes[i].pad = (h.pad & 0xffffu) | (code << 16);
}

// area: null, or the points' headers -- then each value is scaled by the point's area (|w|: its sign
// bit marks a black E), the common-grid gather's E * area (mo_band.h cg_combine)
__global__ void band_permute_kernel(const float *__restrict__ rows, int n, BandGroups g, const float4 *__restrict__ area,
                                    float4 *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * kGroups) return;
    const int grp = (int)(i / n), r = (int)(i % n);
    const float *row = rows + (size_t)r * ROW;
    const float w = area ? fabsf(area[r].w) : 1.f;
    float v[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) v[s] = g.band[grp][s] >= 0 ? (area ? row[g.band[grp][s]] * w : row[g.band[grp][s]]) : 0.f;
    out[i] = make_float4(v[0], v[1], v[2], v[3]);
}
}  // namespace

void DeviceOctree::ensure_leaf_r2(float max_error) {
    if (leaf_r2.ptr && leaf_r2_error == max_error) return;
    leaf_r2.alloc((size_t)(n_nodes > 0 ? n_nodes : 1));
    if (n_nodes > 0)
        hipLaunchKernelGGL(leaf_r2_kernel, dim3((unsigned)((n_nodes + 255) / 256)), dim3(256), 0, 0, nodes.ptr, n_nodes,
                           max_error, leaf_r2.ptr);
    MPSS_HIP(hipGetLastError());
    MPSS_HIP(hipDeviceSynchronize());
    leaf_r2_error = max_error;
}

const BandLayout *DeviceOctree::find_layout(const BandGroups &g) const {
    for (const auto &l : layouts)
        if (same_groups(l->groups, g)) return l.get();
    return nullptr;
}

const BandLayout &DeviceOctree::ensure_layout(const BandGroups &g) {
    if (const BandLayout *l = find_layout(g)) return *l;
    auto lay = std::make_unique<BandLayout>();
    lay->groups = g;
    lay->et.alloc((size_t)(n_nodes > 0 ? n_nodes : 1) * kGroups);
    lay->e.alloc((size_t)(n_points > 0 ? n_points : 1) * kGroups);
    lay->ew.alloc((size_t)(n_points > 0 ? n_points : 1) * kGroups);
    const int64_t tn = (int64_t)n_nodes * kGroups, tp = (int64_t)n_points * kGroups;
    if (tn) hipLaunchKernelGGL(band_permute_kernel, dim3((unsigned)((tn + 255) / 256)), dim3(256), 0, 0, node_et.ptr,
                               n_nodes, g, nullptr, lay->et.ptr);
    if (tp) {
        hipLaunchKernelGGL(band_permute_kernel, dim3((unsigned)((tp + 255) / 256)), dim3(256), 0, 0, pt_e.ptr,
                           n_points, g, nullptr, lay->e.ptr);
        hipLaunchKernelGGL(band_permute_kernel, dim3((unsigned)((tp + 255) / 256)), dim3(256), 0, 0, pt_e.ptr,
                           n_points, g, pt_hdr.ptr, lay->ew.ptr);
    }
    MPSS_HIP(hipGetLastError());
    // synchronous: every stream that launches a gather later sees a complete layout
    MPSS_HIP(hipDeviceSynchronize());
    layouts.push_back(std::move(lay));
    return *layouts.back();
}

}  // namespace mpss
