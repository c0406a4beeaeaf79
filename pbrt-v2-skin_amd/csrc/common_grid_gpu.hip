// common_grid_gpu.hip -- the per-knot scan of the common-grid build (mo_kernel.hip build_common_grid)
// on the GPU, from the profile table where DeviceProfile::upload has just put it.
//
// What runs here is the work that scales with 3 x L x bands: each slot's peak |T|, and for every band
// knot past the near field the error of the group rows at H = 1, 2, 4 against the band's own value
// (knot_err, with scale() for the rgbprofile), into the three bad-cell maps -- for both LDS layouts
// (10236, 5088) and all eight groups in one launch per stage. The host keeps the rest (profile-end
// flags, the sequential prefix scores, the choice of range, the row emission and the error sums), from
// these maps, in build_common_grid itself: one code path for both builders.
//
// Bit identity with the host scan is the contract (tests/test_common_grid_gpu.py):
//   * the arithmetic is the host's, operation for operation, in double, without contraction (the
//     library is compiled with -ffp-contract=off; the pragma below says so again where it matters);
//     IEEE division, floor and float<->double conversions are exact on both sides;
//   * std::max(a, b) is written as the host library defines it, (a < b) ? b : a, so NaNs fall the
//     same way;
//   * a peak is a maximum, the same bits in any order (atomic max on the bit pattern of a
//     non-negative double, NaNs skipped as std::max skips them);
//   * a map cell is only ever set to 1: the threads' order cannot show. The host derives the list
//     of bad fine knots from the H = 1 map in ascending order, so nothing here is order-dependent.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mo_kernel.h"

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

__device__ inline double dmax(double a, double b) { return (a < b) ? b : a; }  // std::max

// R_j(u) of build_common_grid: band c on the group grid (double lerp, rounded once)
__device__ inline float grid_R(const float *__restrict__ tab, int L, int c, double rj, long long u) {
    if (c < 0 || u >= (long long)L) return 0.f;
    const double f = (double)u * rj;
    if (f - rj > (double)(L - 1)) return 0.f;
    const int fl = (int)floor(f);
    const int sidx = fl < L - 2 ? fl : L - 2;
    const double t = f - sidx;
    const float *T = tab + (size_t)c * L;
    return (float)((1.0 - t) * (double)T[sidx] + t * (double)T[sidx + 1]);
}

// each slot's largest |T| (blockIdx.y: combo; layouts share bands but keep their own slot, for simplicity)
__global__ __launch_bounds__(256) void cg_peak_kernel(const float *__restrict__ tab, int L, const ScanCombo *__restrict__ P,
                                                      unsigned long long *__restrict__ peaks) {
    const ScanCombo &c = P[blockIdx.y];
    if (c.j < 0) return;
    const float *T = tab + (size_t)c.band[c.j] * L;
    double m = 0.0;
    for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < L; k += (int)(gridDim.x * blockDim.x)) {
        const double x = fabs((double)T[k]);
        m = dmax(m, x);  // (a NaN is never taken, as on the host)
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
    const float *T = tab + (size_t)c.band[j] * L;
    const double rj = c.r[j];
    const double u = (double)k / rj;
    // scale(j, k)
    double sc = fabs((double)T[k]);
    if (rgb) {
        for (int q = 0; q < 4; ++q) {
            const int cq = c.band[q];
            if (cq < 0 || q == j) continue;
            const double f = u * c.r[q];
            if (f > (double)(L - 1)) continue;
            const int fl = (int)floor(f);
            const int sidx = fl < L - 2 ? fl : L - 2;
            const double t = f - sidx;
            const float *Tq = tab + (size_t)cq * L;
            sc = dmax(sc, fabs((1.0 - t) * (double)Tq[sidx] + t * (double)Tq[sidx + 1]));
        }
    }
    const double peak = __longlong_as_double((long long)peaks[c.peak]);
    const double bound = dmax(kCgRelTol * sc, kCgAbsTol * peak);
    for (int hi = 0; hi < 3; ++hi) {
        const int H = 1 << hi;
        // knot_err(j, k, H)
        const long long m = (long long)floor(u / H);
        const double t = (u - (double)(H * m)) / H;
        const double approx =
            (1.0 - t) * grid_R(tab, L, c.band[j], rj, H * m) + t * grid_R(tab, L, c.band[j], rj, H * (m + 1));
        const double err = fabs(approx - (double)T[k]);
        if (err > bound || err == INFINITY) {
            const unsigned long long cell = (unsigned long long)floor(u / H);
            if (cell < c.size[hi]) maps[c.off[hi] + cell] = 1;
        }
    }
}

}  // namespace

bool scan_common_grid_gpu(const float *dev_tab, int L, const float *host_rcp, const BandGroups &slots,
                          int lds_reserve, bool rgb, CgScan out[2]) {
    if (L < 4) return false;
    for (int g = 0; g < kGroups; ++g)
        for (int j = 0; j < 4; ++j) {
            const int c = slots.band[g][j];
            if (c >= 0 && (!(host_rcp[c] > 0.f) || !std::isfinite(host_rcp[c]))) return false;
        }
    bool same = rgb;  // (rgb: every group's slots are the same three profiles; the host builds group 0 only)
    for (int g = 1; g < kGroups && same; ++g)
        for (int j = 0; j < 4; ++j) same = same && slots.band[g][j] == slots.band[0][j];
    const int ncell = L + 2;
    std::vector<ScanCombo> P(kCombos);
    uint32_t pool = 0;
    int kmin = L;
    static const int kNear[2] = {10236, 5088};
    for (int lay = 0; lay < 2; ++lay) {
        const int kLdsFloats = 4 * (kNear[lay] + 3) - lds_reserve;
        for (int g = 0; g < kGroups; ++g) {
            // the group's near-field split, as build_common_grid's build_group makes it (the same
            // expressions: u0f and r decide which knots are scanned and where they fall)
            float rg = INFINITY;
            int nfull = 0;
            for (int j = 0; j < 4; ++j)
                if (slots.band[g][j] >= 0) {
                    rg = std::min(rg, host_rcp[slots.band[g][j]]);
                    ++nfull;
                }
            double r[4] = {0.0, 0.0, 0.0, 0.0}, rsum = 0.0;
            for (int j = 0; j < 4; ++j)
                if (slots.band[g][j] >= 0) {
                    r[j] = (double)host_rcp[slots.band[g][j]] / (double)rg;
                    rsum += r[j];
                }
            bool skip = nfull == 0 || (same && g > 0);
            int klim[4] = {1, 1, 1, 1}, total = 0;
            if (!skip) {
                int K0 = (int)std::floor((kLdsFloats - 3.0 * nfull - 2.0 * (4 - nfull) - 8.0) / rsum);
                for (;;) {
                    total = 0;
                    for (int j = 0; j < 4; ++j) {
                        if (slots.band[g][j] < 0) {
                            klim[j] = 1;
                        } else {
                            const double want = std::ceil((double)K0 * r[j] * (1.0 + 1e-6)) + 1.0;
                            klim[j] = (int)std::min<double>(want, (double)(L - 2));
                        }
                        total += klim[j] + 1;
                    }
                    if (total <= kLdsFloats || K0 <= 1) break;
                    --K0;
                }
                if (total > kLdsFloats) skip = true;  // (the host build fails this group, and with it the grid)
            }
            double u0 = INFINITY;
            for (int j = 0; j < 4; ++j)
                if (slots.band[g][j] >= 0) u0 = std::min(u0, (double)klim[j] / r[j] * (1.0 - 0x1p-18));
            float u0f = (float)u0;
            if ((double)u0f > u0) u0f = std::nextafter(u0f, 0.f);
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
                    c.r[q] = r[q];
                }
                c.j = (skip || slots.band[g][j] < 0) ? -1 : j;
                c.kstart = c.j < 0 ? L : std::max(0, (int)std::floor((double)u0f * r[j]) - 1);
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
                           (const ScanCombo *)dP.ptr,                           rgb ? 1 : 0, (const unsigned long long *)peaks.ptr, maps.ptr);
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
