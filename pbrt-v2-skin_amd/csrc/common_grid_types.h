// common_grid_types.h -- the plain layout types the sharded gather's kernels (mo_band.h) and the host-only
// common-grid builder (common_grid.cpp) share: the band groups and each group's common grid. No HIP
// runtime: float4 comes from the header-only vector types.
#pragma once
#include <hip/hip_vector_types.h>

#include <cmath>
#include <cstdint>

namespace mpss {

constexpr int NB = 30;      // nSpectralSamples (reference src/core/spectrum.h:46)
constexpr int ROW = 32;     // padded spectral row: 30 bands + 2 pad lanes, 128 B per row

constexpr int kGroups = 8;

// Band -> (group, slot) assignment and per-group pruning scale.
struct BandGroups {
    int band[kGroups][4];    // band index, or -1 for an empty slot
    float rcp_min[kGroups];  // min rcpDsqSpacing over the group's bands
    int pos[NB];             // band c lives at float pos[c] of a group-major row (4 * g + slot)
};

// Deal bands to groups: bands sorted by decreasing profile reach (L-1)/rcp, then either runs of
// adjacent reach (default: group g's bands share one prune radius, so few of its lookups fall
// past a band's profile end) or, with `snake` (mpss_config.mo_band_dealing = 1), snake rounds
// (0..7, 7..0, ...: every group gets one of the 8 longest-reaching bands, equal work per group).
inline BandGroups make_band_groups(const float *rcp, bool snake = false) {
    int order[NB];
    for (int c = 0; c < NB; ++c) order[c] = c;
    for (int i = 1; i < NB; ++i)  // insertion sort by increasing rcp (= decreasing reach)
        for (int j = i; j > 0 && rcp[order[j]] < rcp[order[j - 1]]; --j) {
            const int t = order[j];
            order[j] = order[j - 1];
            order[j - 1] = t;
        }
    BandGroups g;
    int fill[kGroups] = {0};
    for (int i = 0; i < kGroups; ++i) {
        g.rcp_min[i] = INFINITY;
        for (int s = 0; s < 4; ++s) g.band[i][s] = -1;
    }
    // Groups of adjacent reach (6 x 4 + 2 x 3 bands, by decreasing reach): each group's prune radius
    // fits all of its bands, 29 % fewer record visits than dealing the bands in snake rounds; the
    // groups' unequal work is evened out by the gather's work stealing (C2: 41.1 -> 37.3 ms per
    // frame, profiles/r02j_variants.txt r02bf).
    const bool contig = !snake;
    for (int r = 0; r < NB; ++r) {
        const int round = r / kGroups, k = r % kGroups;
        const int grp = contig ? (r < 24 ? r / 4 : 6 + (r - 24) / 3) : ((round & 1) ? kGroups - 1 - k : k);
        const int c = order[r];
        g.band[grp][fill[grp]] = c;
        g.pos[c] = 4 * grp + fill[grp];
        ++fill[grp];
        g.rcp_min[grp] = rcp[c] < g.rcp_min[grp] ? rcp[c] : g.rcp_min[grp];
    }
    return g;
}

inline bool same_groups(const BandGroups &a, const BandGroups &b) {
    for (int g = 0; g < kGroups; ++g)
        for (int s = 0; s < 4; ++s)
            if (a.band[g][s] != b.band[g][s]) return false;
    return true;
}

// The common grid of a band group (mpss_config.mo_common_grid; common_grid.cpp builds it,
// DeviceProfile::build_common uploads it): a
// lookup of all <= 4 bands of the group past their LDS near fields from ONE interleaved table. The
// group's tables are resampled onto the grid of its longest-reach band (rg = its rcpDsqSpacing, for
// which the resampling is the identity), u = d2 * rg, and stored as 32-byte pair rows
// {R_0(u_k), R_0(u_k+1), R_1(u_k), R_1(u_k+1)}, {R_2(u_k), ...}: a lookup is two 16-byte loads from one
// 32-byte-aligned sector per lane instead of four 8-byte lerp pairs from four unrelated offsets (the
// gather is bound by the L2 request rate of these per-lane loads). Row k sits at u_k = k
// below ua and at ua + H (k - ua) above it (H = 1, 2 or 4 per group): the lane's row coordinate is
// v = min(u, fma(u, hinv, hc)), hc = ua (1 - hinv), its row floor(v) and its lerp parameter fract(v), so
// a group's rows can reach its profile end inside kCgMaxRows (common_grid.cpp) where the tables are
// smooth enough for the coarser steps. Each lane takes one of three paths by u:
//   u < u0lim          every band's exact pair from its LDS near field (as the per-band gather);
//   u0lim <= u < u1lim the group rows -- accurate wherever they are read: the builder measures the
//                      error at every band's own knots, and a cell (row) holding a knot off by more
//                      than the bound carries a NaN in its first value: its lanes read the bands' own
//                      tables instead (cg_fix). So does a cell within a step of a band's profile end
//                      (sampleProfile's exact cutoff, multipole.cpp:65-66, is the own path's) and one
//                      before the stretch the rows serve (u1start). The range is the one serving the
//                      most records from good cells (the far tails of the longest-reach bands carry
//                      the MPC resampler's float noise, which no coarser grid follows: every cell bad);
//   otherwise          every band's exact pair from its own table in HBM/L2 (as the per-band gather),
//                      a band past its profile end from the table's trailing zero pair.
struct CommonGrid {
    const float4 *tab;          // pair rows, two float4 each; group g's row for u at 2 * (row0[g] + u - ubase[g])
    uint32_t row0[kGroups];     // group g's first pair row
    uint32_t ubase[kGroups];    // the v (row coordinate) of that row
    float rg[kGroups];          // the group's grid: u = d2 * rg (its smallest rcp)
    float u0lim[kGroups];       // u < u0lim => every band's pair (s, s + 1) lies in its LDS near field
    float u1lim[kGroups];       // u0lim <= u < u1lim: the pair rows (u1lim = u0lim: none)
    float u1start[kGroups];     // the rows' cells below it are flagged (bands the rows cannot serve)
    float ua[kGroups];          // rows one grid step apart below ua, H steps apart above (L: none)
    float hinv[kGroups];        // 1 / H
    float hc[kGroups];          // ua (1 - 1 / H): v = min(u, fma(u, hinv, hc)) (exact: ua a multiple of 64)
    float tau[kGroups][4];      // d2 >= tau <=> fl(d2 * rcp) >= L - 1: the band is past its profile end
    uint32_t lrow[kGroups][4];  // float offset of slot j's near-field row in LDS (entries 0..klim_j)
    int lcnt[kGroups][4];       // its length, klim_j + 1 floats (2 zeros for an empty slot)
    float lds_r2[kGroups];      // a leaf with leaf_r2 below this is read from LDS only (0: never)
    int on;                     // 1: some group has a non-empty row range (the three-path gather runs)
};

}  // namespace mpss
