// common_grid_gpu.hip -- the per-knot scan of the common-grid build (common_grid.cpp build_common_grid)
// on the GPU, from the profile table where DeviceProfile::upload has just put it.
//
// What runs here is the work that scales with 3 x L x bands: each slot's peak |T|, and for every band
// knot past the near field the error of the group rows at H = 1, 2, 4 against the band's own value
// (common_grid_math.h cg_knot_err under cg_knot_bound), into the three bad-cell maps -- for both LDS
// layouts (10236, 5088) and all eight groups in one launch per stage. The host keeps the rest
// (profile-end flags, the sequential prefix scores, the choice of range, the row emission and the error
// sums), from these maps, in build_common_grid itself: one code path for both builders.
//
// Bit identity with the host scan is the contract (tests/test_common_grid_gpu.py):
//   * the arithmetic is the host's: both sides call the functions of common_grid_math.h (double, without
//     contraction, max as the host library defines it), and the host decides the split with cg_split;
//   * a peak is a maximum, the same bits in any order (atomic max on the bit pattern of a
//     non-negative double, NaNs skipped as std::max skips them);
//   * a map cell is only ever set to 1: the threads' order cannot show. The host derives the list
//     of bad fine knots from the H = 1 map in ascending order, so nothing here is order-dependent.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "common_grid.h"

#pragma clang fp contract(off)

namespace mpss {

namespace {

constexpr int kCombos = 2 * kGroups * 4;  // (layout, group, slot)

struct ScanCombo {
    int band[4];          // the group's slots (-1 empty); this combo scans slot j
    double r[4];          // rcp_j / rg
    int j;                // -1: nothing to scan
    int kstart;           // first knot past the near field
    uint32_t off[3];      // the group's three maps in the byte pool
    uint32_t size[3];
    int peak;             // index of this combo's peak in the peak pool
};

// each slot's largest |T| (blockIdx.y: combo; layouts share bands but keep their own slot, for simplicity)
__global__ __launch_bounds__(256) void cg_peak_kernel(const float *__restrict__ tab, int L, const ScanCombo *__restrict__ P,
                                                      unsigned long long *__restrict__ peaks) {
    const ScanCombo &c = P[blockIdx.y];
    if (c.j < 0) return;
    const float *T = tab + (size_t)c.band[c.j] * L;
    double m = 0.0;
    for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < L; k += (int)(gridDim.x * blockDim.x)) {
        const double x = fabs((double)T[k]);
        m = cg_max(m, x);  // (a NaN is never taken, as on the host)
    }
    // m >= 0 and not NaN: its bit pattern orders as the value does
    if (m > 0.0) atomicMax(&peaks[c.peak], (unsigned long long)__double_as_longlong(m));
}

// one thread per (layout, group, slot, knot), all three H: the table reads of a wave are coalesced
__global__ __launch_bounds__(256) void cg_scan_kernel(const float *__restrict__ tab, int L, const ScanCombo *__restrict__ P, int rgb,
                                                      const unsigned long long *__restrict__ peaks,
                                                      unsigned char *__restrict__ maps) {
    const ScanCombo &c = P[blockIdx.y];
    if (c.j < 0) return;
    const int j = c.j;
    const int k = c.kstart + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (k >= L - 1) return;
    const double u = (double)k / c.r[j];
    const double peak = __longlong_as_double((long long)peaks[c.peak]);
    const double bound = cg_knot_bound(tab, L, c.band, c.r, j, k, rgb != 0, peak);
    for (int hi = 0; hi < 3; ++hi) {
        const int H = 1 << hi;
        if (cg_knot_err(tab, L, c.band[j], c.r[j], k, H, bound) == INFINITY) {
            const unsigned long long cell = (unsigned long long)floor(u / H);
            if (cell < c.size[hi]) maps[c.off[hi] + cell] = 1;
        }
    }
}

}  // namespace

bool scan_common_grid_gpu(const float *dev_tab, int L, const float *host_rcp, const BandGroups &slots,
                          int lds_reserve, bool rgb, CgScan out[2]) {
    if (!cg_can_build(L, host_rcp, slots)) return false;
    const bool same = cg_same_slots(slots, rgb);  // (the host then builds group 0 only)
    const int ncell = L + 2;
    std::vector<ScanCombo> P(kCombos);
    uint32_t pool = 0;
    int kmin = L;
    static const int kNear[2] = {10236, 5088};
    for (int lay = 0; lay < 2; ++lay) {
        const int kLdsFloats = 4 * (kNear[lay] + 3) - lds_reserve;
        for (int g = 0; g < kGroups; ++g) {
            // the knots to scan and where they fall: from the group's near-field split
            const CgSplit sp = cg_split(host_rcp, slots.band[g], L, kLdsFloats);
            const bool skip = sp.nfull == 0 || !sp.fit || (same && g > 0);  // (no fit: the host declines the grid)
            uint32_t off[3], size[3];
            for (int hi = 0; hi < 3; ++hi) {
                size[hi] = skip ? 0u : (uint32_t)((size_t)ncell / (1 << hi) + 2);
                off[hi] = pool;
                pool += size[hi];
                out[lay].bad[g][hi].assign(size[hi], 0);
            }
            for (int j = 0; j < 4; ++j) {
                ScanCombo &c = P[(lay * kGroups + g) * 4 + j];
                for (int q = 0; q < 4; ++q) {
                    c.band[q] = slots.band[g][q];
                    c.r[q] = sp.r[q];
                }
                c.j = (skip || slots.band[g][j] < 0) ? -1 : j;
                c.kstart = c.j < 0 ? L : cg_first_knot((double)sp.u0f, sp.r[j]);
                for (int hi = 0; hi < 3; ++hi) {
                    c.off[hi] = off[hi];
                    c.size[hi] = size[hi];
                }
                c.peak = (lay * kGroups + g) * 4 + j;
                kmin = std::min(kmin, c.kstart);
                out[lay].peak[g][j] = 0.0;
            }
        }
    }
    DevBuf<ScanCombo> dP;
    dP.upload(P.data(), P.size());
    DevBuf<unsigned long long> peaks;
    DevBuf<unsigned char> maps;
    peaks.alloc(kCombos);
    maps.alloc(pool ? pool : 1);
    MPSS_HIP(hipMemset(peaks.ptr, 0, sizeof(unsigned long long) * kCombos));
    MPSS_HIP(hipMemset(maps.ptr, 0, pool ? pool : 1));
    const unsigned pb = (unsigned)std::min(64, (L + 255) / 256);
    hipLaunchKernelGGL(cg_peak_kernel, dim3(pb, kCombos), dim3(256), 0, 0, dev_tab, L, (const ScanCombo *)dP.ptr, peaks.ptr);
    const int span = L - 1 - kmin;  // knots kstart .. L - 2 of the combo that starts first
    if (span > 0)
        hipLaunchKernelGGL(cg_scan_kernel, dim3((unsigned)((span + 255) / 256), kCombos), dim3(256), 0, 0, dev_tab, L,
                           (const ScanCombo *)dP.ptr, rgb ? 1 : 0, (const unsigned long long *)peaks.ptr, maps.ptr);
    MPSS_HIP(hipGetLastError());
    std::vector<unsigned char> hm(pool ? pool : 1);
    unsigned long long hp[kCombos];
    MPSS_HIP(hipMemcpy(hm.data(), maps.ptr, hm.size(), hipMemcpyDeviceToHost));
    MPSS_HIP(hipMemcpy(hp, peaks.ptr, sizeof(hp), hipMemcpyDeviceToHost));
    for (int lay = 0; lay < 2; ++lay)
        for (int g = 0; g < kGroups; ++g) {
            for (int j = 0; j < 4; ++j) {
                const ScanCombo &c = P[(lay * kGroups + g) * 4 + j];
                if (c.j >= 0) memcpy(&out[lay].peak[g][j], &hp[c.peak], sizeof(double));
            }
            const ScanCombo &c0 = P[(lay * kGroups + g) * 4];
            for (int hi = 0; hi < 3; ++hi)
                if (c0.size[hi]) memcpy(out[lay].bad[g][hi].data(), hm.data() + c0.off[hi], c0.size[hi]);
        }
    return true;
}

}  // namespace mpss
