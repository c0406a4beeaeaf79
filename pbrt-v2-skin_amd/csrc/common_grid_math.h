// common_grid_math.h -- the one copy of everything the two common-grid builders both compute: the host
// builder (common_grid.cpp) and the GPU's per-knot scan (common_grid_gpu.hip) build the same grid bit for
// bit (tests/test_common_grid_gpu.py) because they call these functions, not restatements of them.
//
// What keeps host and device results identical:
//   * every function is double arithmetic without contraction (the library is compiled with
//     -ffp-contract=off; the pragma below says so again for whatever includes this file); IEEE
//     division, floor and float<->double conversions are exact on both sides;
//   * max is written as the host library defines std::max, (a < b) ? b : a, so NaNs fall the same way.
#pragma once
#include <cmath>
#include <cstddef>

#include "common_grid_types.h"

#pragma clang fp contract(off)

#if defined(__HIPCC__)
#define MPSS_CG_HD __host__ __device__ inline
#else
#define MPSS_CG_HD inline
#endif

namespace mpss {

// The common grid's bound on the resampling error of a lookup: kCgRelTol of the band's own value
// there, or kCgAbsTol of the band's peak where that is larger (the far tails, whose values fall to
// 1e-11 of the peak and carry under 1 % of a band's mass on C2's profile: there the bound is
// absolute). A group row (cell) holding a knot off by more is flagged and
// its lanes read the exact tables. The floor is chosen on the full C2 frame against the oracle, same
// box (profiles/r06_grid_ab.txt, rows H steps apart with flagged cells): 1e-13: gather 43.4 ms,
// unfloored image error 3.3e-5; 1e-14: 43.9 ms, 1.5e-6; 1e-15: 45.1 ms, 1.1e-6 -- the worst values at
// 1e-16 of the frame's peak, far below the film's resolution (round 4, one stretch of rows per group,
// profiles/r04p_abstol.txt: none 60.4 ms, 1.1e-6; 1e-13 48.6 ms, 4.3e-6; 1e-10 47.1 ms, 9.0e-5).
constexpr double kCgRelTol = 2e-6;
#ifndef MPSS_CG_ABS_TOL  // (A/B builds of the floor only)
#define MPSS_CG_ABS_TOL 1e-14
#endif
constexpr double kCgAbsTol = MPSS_CG_ABS_TOL;

MPSS_CG_HD double cg_max(double a, double b) { return (a < b) ? b : a; }  // std::max

// Can a grid be built at all: four rows to lerp between, and a positive finite spacing for every band
// in a slot (otherwise there is no uniform grid to resample).
inline bool cg_can_build(int L, const float *rcp, const BandGroups &slots) {
    if (L < 4) return false;
    for (int g = 0; g < kGroups; ++g)
        for (int j = 0; j < 4; ++j) {
            const int c = slots.band[g][j];
            if (c >= 0 && (!(rcp[c] > 0.f) || !std::isfinite(rcp[c]))) return false;
        }
    return true;
}

// The rgbprofile's slots are the same three profiles in every group: one group is built, the rest copy it.
inline bool cg_same_slots(const BandGroups &slots, bool rgb) {
    bool same = rgb;
    for (int g = 1; g < kGroups && same; ++g)
        for (int j = 0; j < 4; ++j) same = same && slots.band[g][j] == slots.band[0][j];
    return same;
}

// A group's near-field split: the LDS budget (lds_floats) is divided so that every slot's exact near
// field ends at the same distance: klim_j ~ K0 * rcp_j / rg, sum_j (klim_j + 1) <= lds_floats (empty
// slots: 2 zero floats), and u0f = min_j klim_j rg / rcp_j (less a 2^-18 margin, rounded down) guarantees
// s_j = fl(d2 rcp_j) < klim_j for every lane with u < u0f.
struct CgSplit {
    int nfull;    // occupied slots (0: an unused group, no wave ever walks it)
    bool fit;     // false: no split fits the LDS (the grid is declined)
    float rg;     // the group's grid: its smallest rcp
    double r[4];  // rcp_j / rg (0: an empty slot)
    int klim[4];  // slot j's near field holds entries 0..klim_j
    float u0f;
};
inline CgSplit cg_split(const float *rcp, const int band[4], int L, int lds_floats) {
    CgSplit s{};
    s.rg = INFINITY;
    for (int j = 0; j < 4; ++j)
        if (band[j] >= 0) {
            s.rg = std::min(s.rg, rcp[band[j]]);
            ++s.nfull;
        }
    if (s.nfull == 0) return s;
    double rsum = 0.0;
    for (int j = 0; j < 4; ++j)
        if (band[j] >= 0) {
            s.r[j] = (double)rcp[band[j]] / (double)s.rg;
            rsum += s.r[j];
        }
    int K0 = (int)std::floor((lds_floats - 3.0 * s.nfull - 2.0 * (4 - s.nfull) - 8.0) / rsum);
    int total;
    for (;;) {
        total = 0;
        for (int j = 0; j < 4; ++j) {
            if (band[j] < 0) {
                s.klim[j] = 1;
            } else {
                const double want = std::ceil((double)K0 * s.r[j] * (1.0 + 1e-6)) + 1.0;
                s.klim[j] = (int)std::min<double>(want, (double)(L - 2));
            }
            total += s.klim[j] + 1;
        }
        if (total <= lds_floats || K0 <= 1) break;
        --K0;
    }
    s.fit = total <= lds_floats;
    if (!s.fit) return s;
    double u0 = INFINITY;
    for (int j = 0; j < 4; ++j)
        if (band[j] >= 0) u0 = std::min(u0, (double)s.klim[j] / s.r[j] * (1.0 - 0x1p-18));
    s.u0f = (float)u0;
    if ((double)s.u0f > u0) s.u0f = std::nextafter(s.u0f, 0.f);
    return s;
}

// The first knot of a band (relative spacing rj) that is compared for rows beginning at u
inline int cg_first_knot(double u, double rj) {
    const int k = (int)std::floor(u * rj) - 1;
    return k < 0 ? 0 : k;
}

// A band's lerp at fractional index f in double, its last segment continued past the end
MPSS_CG_HD double cg_lerp(const float *T, int L, double f) {
    const int fl = (int)floor(f);
    const int sidx = fl < L - 2 ? fl : L - 2;
    const double t = f - sidx;
    return (1.0 - t) * (double)T[sidx] + t * (double)T[sidx + 1];
}

// R_j(u): band c (relative spacing rj = rcp_c / rg) on the group grid, rounded once; its last segment
// continued one row past its end, 0 after
MPSS_CG_HD float cg_R(const float *tab, int L, int c, double rj, long long u) {
    if (c < 0 || u >= (long long)L) return 0.f;
    const double f = (double)u * rj;
    if (f - rj > (double)(L - 1)) return 0.f;  // past the row after the band's end
    return (float)cg_lerp(tab + (size_t)c * L, L, f);
}

// The value the error at slot j's knot k is relative to: the band's own |T[k]|; for the rgbprofile's R,
// G, B (rgb) the largest of the three at that distance -- FromRGB's outputs are sums of the three with
// weights of order one, so each component's error counts against their scale, not its own (B, ~15x
// shorter reach, falls orders of magnitude under R and G soon past the near field)
MPSS_CG_HD double cg_scale(const float *tab, int L, const int band[4], const double r[4], int j, int k, bool rgb) {
    double v = fabs((double)tab[(size_t)band[j] * L + k]);
    if (!rgb) return v;
    const double u = (double)k / r[j];
    for (int q = 0; q < 4; ++q) {
        if (band[q] < 0 || q == j) continue;
        const double f = u * r[q];
        if (f > (double)(L - 1)) continue;
        v = cg_max(v, fabs(cg_lerp(tab + (size_t)band[q] * L, L, f)));
    }
    return v;
}

// The bound on the rows' error at slot j's knot k (peak: the band's largest |T|)
MPSS_CG_HD double cg_knot_bound(const float *tab, int L, const int band[4], const double r[4], int j, int k, bool rgb,
                                double peak) {
    return cg_max(kCgRelTol * cg_scale(tab, L, band, r, j, k, rgb), kCgAbsTol * peak);
}

// The per-knot test: |rows - T| at band c's knot k on rows H grid steps apart (cells [H m, H (m + 1))),
// +inf when it exceeds the bound (the knot is bad). The knot lies at u = k / rj, in cell floor(u / H).
MPSS_CG_HD double cg_knot_err(const float *tab, int L, int c, double rj, int k, int H, double bound) {
    const double u = (double)k / rj;
    const long long m = (long long)floor(u / H);
    const double t = (u - (double)(H * m)) / H;
    const double approx = (1.0 - t) * cg_R(tab, L, c, rj, H * m) + t * cg_R(tab, L, c, rj, H * (m + 1));
    const double err = fabs(approx - (double)tab[(size_t)c * L + k]);
    return err > bound ? INFINITY : err;
}

}  // namespace mpss
