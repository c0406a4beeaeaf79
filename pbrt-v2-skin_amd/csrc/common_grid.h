// common_grid.h -- the builder of the common grid (common_grid_types.h CommonGrid): the resampled pair-row
// table the sharded Mo() gather reads past its LDS near field. Host only (common_grid.cpp, plain C++, no
// HIP runtime), with the part that scales with 3 x L x bands optionally done on the GPU
// (common_grid_gpu.hip); both go through common_grid_math.h and build the same grid bit for bit.
#pragma once
#include <cstdint>
#include <vector>

#include "common_grid_math.h"
#include "common_grid_types.h"

namespace mpss {

// The per-knot scan's results, when the GPU made them (scan_common_grid_gpu) instead of build_common_grid
struct CgScan {
    std::vector<uint8_t> bad[kGroups][3];  // per group and row spacing H = 1, 2, 4: cells with a knot off by more than the bound
    double peak[kGroups][4];               // each slot's largest |T|
};

// The grid of one LDS layout from the host band tables: the layout (cg, without tab), the pair rows h (two
// float4 per row, group by group from cg.row0) and the per-band errors; true (cg.on) when some group
// has rows. rgb: the slots are the rgbprofile's R, G, B, whose knots' errors are relative to the
// largest of the three at that distance (the scale of FromRGB's outputs) instead of their own value.
// lds_reserve: floats at the end of the LDS near field the split leaves free.
// pre: the per-knot scan's results from the GPU (below) instead of scanning here; the rest is the same code.
bool build_common_grid(const float *tab, int L, const float *rcp, const BandGroups &groups, CommonGrid &cg,
                       std::vector<float4> &h, float rel_err[NB], float l1_err[NB], int near_field = 10236,
                       int lds_reserve = 0, bool rgb = false, const CgScan *pre = nullptr);

// The part of build_common_grid that scales with 3 x L x bands, on the GPU (common_grid_gpu.hip): each
// slot's peak |T| and the per-knot error test at H = 1, 2, 4 into the bad-cell maps, for both LDS layouts
// (out[0]: 10236, out[1]: 5088) and all groups in one launch per stage. dev_tab: the [NB][L] table on the
// device. False when no grid can be built (build_common_grid then declines by itself). Synchronous.
bool scan_common_grid_gpu(const float *dev_tab, int L, const float *host_rcp, const BandGroups &slots,
                          int lds_reserve, bool rgb, CgScan out[2]);

}  // namespace mpss
