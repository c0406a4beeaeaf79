// mo_kernel.hip -- the host side of the production Mo() gather, the spectrally sharded one (mo_band.h,
// mo_wave.h) on CDNA4 (gfx950): the query sort, the kernel arguments and the launch; and
// launch_mo_gather, which dispatches mpss_mo_batch's modes to it and to the two checking paths
// (mo_exact.hip: the reference's summation order; mo_packet.hip).
//
// Computes, for each query point p, SubsurfaceOctreeNode::Mo(octreeBounds, p, ...)
// (reference src/integrators/diffusionutil.h:175-210) with the multipole profile
// Rd(d^2) of MultipoleProfileData::reflectance (src/core/multipole.cpp:60-113).
#include "mo_kernel.h"
#include "mo_wave.h"
#include "spectral.h"

#include <algorithm>
#include <cmath>

namespace mpss {

namespace {

// 30-bit Morton code of a point in [lo, lo + 1/inv) per axis (10 bits per axis, clamped).
__device__ __forceinline__ uint32_t morton_expand10(uint32_t v) {
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
__device__ __forceinline__ uint32_t morton30(float x, float y, float z, const float lo[3], const float inv[3]) {
    const float q[3] = {(x - lo[0]) * inv[0], (y - lo[1]) * inv[1], (z - lo[2]) * inv[2]};
    uint32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (uint32_t)fminf(fmaxf(q[k], 0.f), 1023.f);
    return (morton_expand10(c[0]) << 2) | (morton_expand10(c[1]) << 1) | morton_expand10(c[2]);
}

// Step 1: each 1024-query chunk sorted by the Morton key of its live queries, written as a
// permutation: perm[base + i] = the i-th query
// of the chunk in key order, -1 past the live ones. Chunks at or past the query count write nothing.
__global__ __launch_bounds__(1024) void mo_sort_kernel(BandArgs a) {
    __shared__ unsigned long long keys[1024];
    const int tid = (int)threadIdx.x;
    const int nq = a.count ? *a.count : a.nq;
    const int base = (int)blockIdx.x * 1024;
    if (base >= nq) return;  // uniform over the block
    float px = 0.f, py = 0.f, pz = 0.f;
    const bool in = base + tid < nq && band_query(a, base + tid, px, py, pz);
    const uint32_t key = in ? morton30(px, py, pz, a.klo, a.kinv) : 0xffffffffu;  // dead last
    keys[tid] = ((unsigned long long)key << 32) | (unsigned)tid;
    __syncthreads();
    for (int k = 2; k <= 1024; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            const int ixj = tid ^ j;
            if (ixj > tid) {
                const unsigned long long x = keys[tid], y = keys[ixj];
                if ((x > y) == ((tid & k) == 0)) {
                    keys[tid] = y;
                    keys[ixj] = x;
                }
            }
            __syncthreads();
        }
    const unsigned long long mine = keys[tid];
    a.perm[base + tid] = (mine >> 32) != 0xffffffffull ? base + (int)(mine & 0xffffffffull) : -1;
}

void launch_band(BandArgs a, int nq_max, const DeviceOctree &t, bool count, const GatherOpts &opts,
                 hipStream_t stream) {
    if (nq_max <= 0) return;
    if (!a.perm) throw Error(-2, "launch_band: the sharded gather needs its permutation scratch");
    if (opts.near_field != 10236 && opts.near_field != 5088)
        throw Error(-1, "mo_near_field must be 10236 or 5088");
    for (int k = 0; k < 3; ++k) {
        const float ext = t.bmax[k] - t.bmin[k];
        a.klo[k] = t.bmin[k];
        a.kinv[k] = ext > 0.f ? 1023.99f / ext : 0.f;
    }
    MPSS_HIP(hipMemsetAsync(a.work, 0, sizeof(int) * kGroups, stream));
    if (count && opts.count_noprune) a.t.prune_f = INFINITY;
    const int chunks = (nq_max + 1023) / 1024;
    hipLaunchKernelGGL(mo_sort_kernel, dim3((unsigned)chunks), dim3(1024), 0, stream, a);
    const bool wide = opts.near_field == 10236;
    const int cap = wide ? 32 : 64;  // resident workgroups per group: 1 or 2 per CU of an XCD
    const dim3 grid((unsigned)((chunks < cap ? chunks : cap) * kGroups));
    if (!wide) a.t.cg = a.t.cg_half;  // the grid built for the 5088 layout's LDS split
    const bool cg = opts.common_grid && a.t.cg.on && a.t.cg.tab;
    if (a.t.rgb_refl && cg)  // rgbprofile: three lookups per record, FromRGB into the group's bands
        launch_wave_rgb_cg(a, grid, count, wide, opts.steal, stream);
    else if (a.t.rgb_refl)
        launch_wave_rgb(a, grid, count, wide, opts.steal, stream);
    else if (cg)
        launch_wave_cg(a, grid, count, wide, opts.steal, stream);
    else
        launch_wave_plain(a, grid, count, wide, opts.steal, stream);
    MPSS_HIP(hipGetLastError());
}

BandTree band_tree(const DeviceOctree &t, const BandLayout &l, const DeviceProfile &p, float max_error) {
    if (!same_groups(l.groups, p.groups)) throw Error(-2, "band layout does not match the profile's band groups");
    BandTree bt;
    bt.nodes = t.nodes.ptr;
    bt.band_et = l.et.ptr;
    bt.pt_hdr = t.pt_hdr.ptr;
    bt.band_e = l.e.ptr;
    bt.band_ew = l.ew.ptr;
    bt.table = p.table.ptr;
    bt.groups = p.groups;
    for (int g = 0; g < kGroups; ++g) {
        bt.grcp_max[g] = 0.f;
        for (int s = 0; s < 4; ++s) {
            bt.grcp[g][s] = p.groups.band[g][s] >= 0 ? p.host_rcp[p.groups.band[g][s]] : 0.f;
            bt.grcp_max[g] = bt.grcp[g][s] > bt.grcp_max[g] ? bt.grcp[g][s] : bt.grcp_max[g];
        }
    }
    bt.leaf_r2 = (t.leaf_r2.ptr && t.leaf_r2_error == max_error) ? t.leaf_r2.ptr : nullptr;
    bt.cg = p.cg;
    bt.cg_half = p.cg_half;
    for (int g = 0; g < kGroups; ++g)
        for (int s2 = 0; s2 < 4; ++s2) bt.lband[g][s2] = p.groups.band[g][s2];
    bt.rgb_refl = nullptr;
    if (p.rgb_refl.ptr) {  // rgbprofile: rows 0..2 (R, G, B) in every group, one reach for all
        float rmin = INFINITY, rmax = 0.f;
        for (int k = 0; k < 3; ++k) {
            rmin = std::min(rmin, p.host_rcp[k]);
            rmax = std::max(rmax, p.host_rcp[k]);
        }
        for (int g = 0; g < kGroups; ++g) {
            for (int s2 = 0; s2 < 4; ++s2) {
                bt.lband[g][s2] = s2 < 3 ? s2 : -1;
                bt.grcp[g][s2] = s2 < 3 ? p.host_rcp[s2] : 0.f;
            }
            bt.grcp_max[g] = rmax;
            bt.groups.rcp_min[g] = rmin;
        }
        bt.rgb_refl = p.rgb_refl.ptr;  // (p.cg: the grid of the three profiles, set_rgb)
        // the groups' FromRGB weights: rgbRefl2Spect{White, Cyan, Magenta, Yellow, Red, Green, Blue}
        for (int g = 0; g < kGroups; ++g)
            for (int s2 = 0; s2 < 4; ++s2) {
                const int c = p.groups.band[g][s2];
                auto at = [&](int t) { return c >= 0 ? rgb_refl2spect(t)[c] : 0.f; };
                bt.rgb_k[g].w[s2] = at(0);
                for (int t = 0; t < 3; ++t) {
                    bt.rgb_k[g].x[t][s2] = at(1 + t);  // Cyan, Magenta, Yellow
                    bt.rgb_k[g].y[t][s2] = at(4 + t);  // Red, Green, Blue
                }
            }
    }
    if (!bt.leaf_r2)
        for (int g = 0; g < kGroups; ++g) bt.cg.lds_r2[g] = bt.cg_half.lds_r2[g] = 0.f;
    bt.L = p.L;
    bt.n_nodes = t.n_nodes;
    bt.n_points = t.n_points;
    bt.max_error = max_error;
    const PruneLimit pl = prune_limit(p.L, p.rcp_min);
    bt.prune_f = pl.prune_f;
    if (!(pl.rcp_min > 0.f))
        for (int g = 0; g < kGroups; ++g) bt.groups.rcp_min[g] = 0.f;  // rcp <= 0: no pruning
    return bt;
}

}  // namespace

void launch_mo_band(const DeviceOctree &t, const BandLayout &layout, const DeviceProfile &p, float max_error,
                    int nq_max, const float4 *queries4, const int *count_dev, float4 *out4, const uint32_t *hit_s,
                    int mat, unsigned long long *counts, int *work, int *perm, const GatherOpts &opts,
                    hipStream_t stream) {
    if (nq_max <= 0 || t.n_nodes <= 0) return;
    BandArgs a{};
    a.t = band_tree(t, layout, p, max_error);
    a.queries4 = queries4;
    a.count = count_dev;
    a.hit_s = hit_s;
    a.mat = mat;
    a.nq = nq_max;
    a.out4 = out4;
    a.counts = counts;
    a.work = work;
    a.perm = perm;
    launch_band(a, nq_max, t, counts != nullptr, opts, stream);
}

void launch_mo_gather(const DeviceOctree &t, const BandLayout *layout, const DeviceProfile &p, float max_error, int nq,
                      const float *queries, float *out, int out_stride, int32_t *counters, int *work, int *perm,
                      int mode, const GatherOpts &opts, hipStream_t stream, unsigned long long *counts) {
    if (nq <= 0) return;
    if (counts && mode != 0) throw Error(-1, "launch_mo_gather: path statistics come from the sharded gather only");
    if (t.n_nodes <= 0) throw Error(-1, "launch_mo_gather: octree is empty");
    if (p.L < 2) throw Error(-1, "launch_mo_gather: profile table has fewer than 2 entries");
    if (mode == 1) return launch_mo_exact(t, p, max_error, nq, queries, out, out_stride, counters, stream);
    if (mode != 0) return launch_mo_packet(t, p, max_error, nq, queries, out, out_stride, counters, stream);
    const bool count = counters != nullptr || counts != nullptr;
    if (!layout || !work) throw Error(-2, "launch_mo_gather: the sharded gather needs a band layout and work counters");
    if (counters) MPSS_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t) * 4 * (size_t)nq, stream));
    BandArgs b{};
    b.t = band_tree(t, *layout, p, max_error);
    b.queries3 = queries;
    b.nq = nq;
    b.out = out;
    b.out_stride = out_stride;
    b.counters = counters;
    b.counts = counts;
    b.work = work;
    b.perm = perm;
    launch_band(b, nq, t, count, opts, stream);
}

}  // namespace mpss
