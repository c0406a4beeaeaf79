// mo_kernel.h -- the device-resident profile and the Mo() gather launchers (the device-resident octree:
// device_octree.h).
#pragma once
#include "common.h"
#include "device_octree.h"
#include "mo_band.h"

namespace mpss {

// (upload, set_rgb and build_common: device_profile.cpp)
struct DeviceProfile {
    DevBuf<float> table;  // [NB][L] channel-major + 2 trailing zeros
    DevBuf<float> rcp;    // [NB]
    float rcp_min = 0.f;  // min over bands (exact subtree pruning, mo_band.h prune_limit)
    int L = 0;
    float host_rcp[NB];
    BandGroups groups{};   // band -> XCD group assignment for this profile
    // The common grid of each band group (common_grid_types.h CommonGrid), built by upload() for each LDS layout
    // (the 10236-entry near field: cg; the 5088-entry one, the default: cg_half): ctab / ctab_half hold
    // the groups' pair rows (two float4 per row); on = 1 when some group has an accurate row range.
    DevBuf<float4> ctab, ctab_half;
    CommonGrid cg{}, cg_half{};  // for the 10236 and 5088 LDS layouts
    // per band and layout: max |R - T| / |T| over its knots read from the group rows, and the sum of
    // |R - T| over those knots / the sum of |T| over the table ([0]: 10236 layout, [1]: 5088)
    float cg_rel_err[2][NB] = {};
    float cg_l1_err[2][NB] = {};
    // snake: deal the bands to groups in snake rounds instead of runs of adjacent reach (common_grid_types.h)
    // grid_host: the common grids' per-knot scan on the host (common_grid.h build_common_grid alone) instead
    // of the GPU (scan_common_grid_gpu); the same grids bit for bit
    void upload(const float *table, int L, const float *rcp, bool snake = false, bool grid_host = true);
    bool grid_on_host = true;
    // (upload calls it with groups, set_rgb with rows 0..2 in every group; host table [NB][L])
    // lds_reserve: floats at the end of the LDS near field the grid's split leaves free
    // rgb: the slots are the rgbprofile's R, G, B (common_grid.h build_common_grid)
    void build_common(const float *table, const BandGroups &slots, int lds_reserve, bool rgb);
    // rgbprofile material: rows 0..2 of the table are its R, G, B profiles; the sharded gather looks
    // up those three for every group and converts them with FromRGB (rgb_refl: the device copy of
    // the rgbRefl2Spect tables, [7][NB]; set_rgb after upload)
    DevBuf<float> rgb_refl;
    void set_rgb(const float *table);
};

// Choices of the sharded gather (mpss_config.mo_near_field / mo_work_stealing; count_noprune =
// mpss_config.count_traversal == 2, instrumented passes only).
struct GatherOpts {
    int near_field = 10236;
    bool steal = true;
    bool count_noprune = false;
    bool common_grid = true;  // mpss_config.mo_common_grid (the layout's grid: cg for 10236, cg_half for 5088)
};

// queries/out/counters are device pointers. out[q * out_stride + c], c < 30.
// counters (nullable, q*4 int32): per query {reference-traversal nodes entered, points evaluated,
// pruned-kernel nodes entered, points evaluated}. The packet kernel reports only
// the last two (the first two are 0); mode 1 follows the reference summation order.
// counts (mode 0 only, nullable): the instrumented pass's statistics, kStatStride * kGroups, added to.
// mode: 0 spectrally sharded (default; needs `layout` for p.groups), 1 exact reference order, 2 packet.
// work: kGroups ints of device scratch for mode 0 (the persistent grid's chunk counters); perm:
// >= nq rounded up to 1024 ints of device scratch for mode 0 (the sorted query permutation).
void launch_mo_gather(const DeviceOctree &t, const BandLayout *layout, const DeviceProfile &p, float max_error, int nq,
                      const float *queries, float *out, int out_stride, int32_t *counters, int *work, int *perm,
                      int mode, const GatherOpts &opts, hipStream_t stream, unsigned long long *counts = nullptr);

// launch_mo_gather's mode 1 (mo_exact.hip) and mode 2 (mo_packet.hip), behind its argument checks
void launch_mo_exact(const DeviceOctree &t, const DeviceProfile &p, float max_error, int nq, const float *queries,
                     float *out, int out_stride, int32_t *counters, hipStream_t stream);
void launch_mo_packet(const DeviceOctree &t, const DeviceProfile &p, float max_error, int nq, const float *queries,
                      float *out, int out_stride, int32_t *counters, hipStream_t stream);

// Mo with the closed-form single dipole (dipole.h) as Rd, in the reference summation order.
// dipole_dev: [4][NB] device floats zpos, zneg, sigma_tr, k. Nothing is pruned.
void launch_mo_dipole(const DeviceOctree &t, const float *dipole_dev, float max_error, int nq, const float *queries,
                      float *out, int out_stride, int32_t *counters, hipStream_t stream);

// Mo with an rgbprofile material (multipole.cpp:85-107): table3 [3][L] R, G, B profiles (device),
// rcp3 their rcpDsqSpacing (device and host copies), in the reference summation order. Queries
// either queries (q x 3) or the render path's queries4 / count_dev / hit_s + mat (see
// launch_mo_band); out[i * out_stride + c].
void launch_mo_rgb(const DeviceOctree &t, const float *table3, const float *rcp3_dev, const float rcp3[3], int L,
                   float max_error, int nq, const float *queries, const float4 *queries4, const int *count_dev,
                   const uint32_t *hit_s, int mat, float *out, int out_stride, int32_t *counters, hipStream_t stream);

// Traversal statistics of the sharded gather (count variant): per group g, counts[kStatStride*g + k]
// for k = 0 node visits, 1 point visits (summed over queries), 2 wave node iterations, 3 wave
// point iterations (summed over waves; 64 x these / the visits = 1 / lane efficiency), 4 table
// lookups inside the profile (lane x band), 5..7 those at entries < 4096, 8192, 16384; common grid
// only: 8 lane-records read from the group rows (two 16-byte loads each), 9 from the LDS near field,
// 10 from the bands' own tables (four 8-byte loads); 11..16 the L2 footprint of the row and own-table
// fetches (mo_band.h kHist 7..12: distinct 32-B sectors, 128-B lines, wave fetches); 17 lane-records of
// flagged row cells; 18 lane-opens of leaves that qualify for the LDS-only pair loop, 19 of leaves with an
// odd live count; 20 lane-visits pruned by the reach test, 21 of black nodes, 22 inside the box of a
// node other than the root (mo_band.h kHist 13..18).
constexpr int kStatStride = 4 + 19;

// Spectrally sharded gather for the render path: queries4[i] = {p, *}, i < *count_dev (<= nq_max);
// out4[i * 8 + g] = the 4 bands of group g (BandGroups::pos gives a band's float offset).
// hit_s / mat (hit_s nullable): only queries whose hit_s material field equals mat are evaluated
// (scenes with several BSSRDF materials run one launch per material). counts: see kStatStride.
// work: kGroups ints of device scratch (the chunk counters of the persistent grid); perm: >= nq_max
// rounded up to 1024 ints of device scratch.
void launch_mo_band(const DeviceOctree &t, const BandLayout &layout, const DeviceProfile &p, float max_error,
                    int nq_max, const float4 *queries4, const int *count_dev, float4 *out4,
                    const uint32_t *hit_s, int mat, unsigned long long *counts, int *work, int *perm,
                    const GatherOpts &opts, hipStream_t stream);

}  // namespace mpss
