// common_grid.cpp -- the common grid (common_grid_types.h CommonGrid) on the host, from the band tables.
// Plain C++: no device buffers, no HIP runtime (tests/cg_host links this file alone, under sanitizers).
//
//   * group g's grid is its longest-reach band's own (rg = the smallest rcp), u = d2 * rg;
//   * the LDS budget of the gather's near field is split so that every slot's exact near field ends at
//     the same distance (common_grid_math.h cg_split);
//   * R_j(u) = band j's lerp at f = u * rcp_j / rg in double (its last segment continued one row past
//     its end, 0 after); on the group rows a lane computes (1 - t) R_j(u0) + t R_j(u0 + 1);
//   * the row range: the far path reads R where the band gather reads T, both piecewise linear, so the
//     largest error lies on a knot of one of the two grids, and at the group grid's knots R is T's own
//     lerp; every band knot s >= u0lim rcp_j / rg - 1 is compared (R's lerp at u = s rg / rcp_j against
//     T[s]) against max(kCgRelTol scale, kCgAbsTol peak), scale = |T[s]| (unfloored: a zero or a sign
//     change is bad), for the rgbprofile's R, G, B (rgb) the largest of the three at that distance;
//   * at most kCgMaxRows rows per group (32 B each: a group's rows stay well inside its XCD's 4 MB L2);
//   * tau_j = the smallest float d2 with fl(d2 * rcp_j) >= L - 1 (sampleProfile's range test).
//
// The row layout. Rows are indexed by v, a piecewise-linear map of u: v = u below ua (one row per grid
// step), v = ua + (u - ua) / H above it (one row per H steps, H = 1, 2 or 4) -- on the lane
// v = min(u, fma(u, hinv, hc)), hc = ua (1 - hinv). A cell (rows k, k + 1) is "bad" when some band knot in
// it is off by more than the bound on the rows (the error of two piecewise-linear functions peaks at a knot
// of one or the other, and at the row positions R is the band's own lerp, rounded once); a bad cell's row
// carries a NaN in slot 0's first value and its lanes read the bands' own tables instead (cg_fix), so
// every served value is within the bound. The range [u1start, u1lim), ua and H are chosen to maximise the
// record weight served by good cells (records per unit u fall off as 1 / u past the near field: the
// octree's aggregated nodes grow with distance), a bad cell counting against it, within kCgMaxRows rows
// (+ one pad row).
//
// Each group is built in stages over a GroupGrid (build_group): split and tau -> bad maps (scanned here,
// or taken from the GPU's scan) -> profile-end flags -> prefix scores -> range choice -> row emission ->
// error sums.
#include "common_grid.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

namespace mpss {

namespace {

#ifndef MPSS_CG_MAX_ROWS_DEFAULT  // (A/B builds of the cap only)
#define MPSS_CG_MAX_ROWS_DEFAULT 49152
#endif
constexpr int kCgMaxRows = MPSS_CG_MAX_ROWS_DEFAULT;
// The range choice tries at most 64 starts per group: the near field's end and the cells just
// past the first 63 distinct bad fine knots. A table whose first accurate stretch begins after more
// bad knots than that (a rough table, tests/test_common_grid.py) gets the best range among those 64
// starts only -- still within the error bound (every served cell is checked), possibly shorter than
// the best one; each start costs O(L / 64) lookups per row spacing.
constexpr size_t kCgMaxStarts = 64;
// (a diagnostic build, -DMPSS_DIAGNOSTICS, lets MPSS_CG_MAX_ROWS override the cap: row-cap experiments)
int cg_max_rows() {
#ifdef MPSS_DIAGNOSTICS
    const char *e = getenv("MPSS_CG_MAX_ROWS");
    if (e && atoi(e) > 0) return atoi(e);
#endif
    return kCgMaxRows;
}

constexpr int kH[3] = {1, 2, 4};  // the row spacings a group may use past ua

struct GridIn {
    const float *tab;  // [NB][L]
    int L;
    const float *rcp;
    int lds_floats;  // the near field's LDS budget
    bool rgb;
    int64_t cap;     // cg_max_rows()
};

// One group's grid as the stages build it
struct GroupGrid {
    int band[4];
    CgSplit s;
    // the group's entries of CommonGrid (as an unused or declined group leaves them)
    float rg = 0.f, u0lim = 0.f, u1lim = 0.f, u1start = 0.f, ua = 0.f, hinv = 1.f, hc = 0.f, lds_r2 = 0.f;
    float tau[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t ubase = 0, lrow[4] = {0, 0, 0, 0};
    int lcnt[4] = {0, 0, 0, 0};
    // the scan: each slot's largest |T|, and per row spacing the cells holding a knot off by more than the
    // bound (later also those the profile ends flag); cells of the fine grid: u < L + 2, coarse: / H
    double peak[4] = {0.0, 0.0, 0.0, 0.0};
    std::vector<uint8_t> bad[3];
    std::vector<double> starts;  // candidate range starts: the near field's end, then just past bad fine knots
    int64_t c0 = 0, vbase = 0;   // the near field's last cell; the first row (the row below c0 is never read)
    // the chosen range: rows serve [start, u1), fine below row_ua, H = kH[hi] steps apart above
    double score = 0.0, start = 0.0;
    int64_t row_ua = 0, u1 = 0;
    int hi = 0;
    std::vector<float4> rows;
    float rel[4] = {0.f, 0.f, 0.f, 0.f}, l1[4] = {0.f, 0.f, 0.f, 0.f};
    bool any = false, fail = false;

    int H() const { return kH[hi]; }
    int64_t upos(int64_t v) const { return v <= row_ua ? v : row_ua + (int64_t)H() * (v - row_ua); }
    bool cell_bad(int64_t v) const {
        const int64_t u = upos(v);
        if (u < (int64_t)std::floor(start) && u >= c0) return true;  // before the stretch the rows serve
        return v < row_ua ? bad[0][(size_t)u] != 0 : bad[hi][(size_t)(u / H())] != 0;
    }
};

// Stage 1: the LDS split and each slot's tau. False: nothing more to build (unused group, or no split fits).
bool split_and_tau(const GridIn &in, GroupGrid &G) {
    const int L = in.L;
    G.s = cg_split(in.rcp, G.band, L, in.lds_floats);
    if (G.s.nfull == 0) {  // an unused group: no wave ever walks it
        for (int j = 0; j < 4; ++j) {
            G.lrow[j] = (uint32_t)(2 * j);
            G.lcnt[j] = 2;
        }
        return false;
    }
    if (!G.s.fit) {
        G.fail = true;
        return false;
    }
    uint32_t off = 0;
    for (int j = 0; j < 4; ++j) {
        G.lrow[j] = off;
        G.lcnt[j] = G.s.klim[j] + 1;
        off += (uint32_t)(G.s.klim[j] + 1);
    }
    const float u0f = G.s.u0f;
    G.u0lim = u0f;
    G.rg = G.s.rg;
    // a leaf is LDS-only when every lane's u < u0lim: leaf_r2 * rg below u0lim, with a 1e-5 margin
    // for the rounding of the lanes' d2 (as the band gather's lds_r2_lim)
    G.lds_r2 = (float)((double)u0f / ((double)G.s.rg * 1.00001));
    // (the rows always begin at the near field's end, so that a lane's row path is u0lim <= u < u1lim:
    // one compare; the cells before the chosen start are flagged)
    G.c0 = (int64_t)std::floor((double)u0f);
    G.vbase = std::max<int64_t>(0, G.c0 - 1);
    for (int j = 0; j < 4; ++j) {
        const int c = G.band[j];
        if (c < 0) {
            G.tau[j] = INFINITY;  // (its sum is never stored)
            continue;
        }
        const float rc = in.rcp[c];
        const float endf = (float)(L - 1);
        float x = (float)((double)(L - 1) / (double)rc);
        auto past = [&](float d2) {
            volatile float f = d2 * rc;  // the float product of sampleProfile (multipole.cpp:63)
            return f >= endf;
        };
        while (x > 0.f && past(x)) x = std::nextafter(x, 0.f);
        while (!past(x)) x = std::nextafter(x, INFINITY);
        G.tau[j] = x;
    }
    return true;
}

// Stage 2, here: the peaks and the per-knot test of every band knot past the near field, at each spacing
void scan_knots(const GridIn &in, GroupGrid &G) {
    const int L = in.L;
    for (int j = 0; j < 4; ++j) {
        if (G.band[j] < 0) continue;
        const float *T = in.tab + (size_t)G.band[j] * L;
        for (int k = 0; k < L; ++k) G.peak[j] = cg_max(G.peak[j], std::fabs((double)T[k]));
        for (int k = cg_first_knot((double)G.s.u0f, G.s.r[j]); k < L - 1; ++k) {
            const double u = (double)k / G.s.r[j];
            const double bound = cg_knot_bound(in.tab, L, G.band, G.s.r, j, k, in.rgb, G.peak[j]);
            for (int hi = 0; hi < 3; ++hi)
                if (cg_knot_err(in.tab, L, G.band[j], G.s.r[j], k, kH[hi], bound) == INFINITY)
                    G.bad[hi][(size_t)std::floor(u / kH[hi])] = 1;
        }
    }
}

// Stage 2, from the GPU: the same peaks (a maximum, the same bits in any order) and maps (the same per-knot
// test, common_grid_gpu.hip; a cell is only ever set, so the threads' order cannot show)
void take_scan(const CgScan &pre, int g, GroupGrid &G) {
    for (int j = 0; j < 4; ++j) G.peak[j] = pre.peak[g][j];
    for (int hi = 0; hi < 3; ++hi)
        if (pre.bad[g][hi].size() == G.bad[hi].size()) G.bad[hi] = pre.bad[g][hi];
}

// The candidate starts of the range: the near field's end, and just past each of the first bad fine
// knots -- the set cells of the H = 1 map in ascending order, before the profile ends flag theirs
void candidate_starts(const GridIn &in, GroupGrid &G) {
    const double uend = (double)(in.L - 1);
    G.starts.assign(1, (double)G.s.u0f);
    for (size_t m = 0; m < G.bad[0].size() && G.starts.size() < kCgMaxStarts; ++m) {
        if (!G.bad[0][m]) continue;
        const double st = (double)m + 2.0;
        if (st > G.starts.back() && st < uend) G.starts.push_back(st);
    }
}

// Stage 3: a cell within a step of a band's profile end (u_end = (L - 1) / r_j) is flagged too: there the
// lanes take the own path, whose pairs carry sampleProfile's exact cutoff (multipole.cpp:65-66);
// past it the band's rows are exactly 0 (R is 0 from u_end + 1 on), before it every lane's f_j is
// at least one table step below L - 1 -- so the combine needs no range test
void flag_profile_ends(const GridIn &in, GroupGrid &G) {
    for (int j = 0; j < 4; ++j) {
        if (G.band[j] < 0) continue;
        const double ue = (double)(in.L - 1) / G.s.r[j];
        for (int hi = 0; hi < 3; ++hi) {
            const int H = kH[hi];
            const int64_t m0 = std::max<int64_t>(0, (int64_t)std::floor((ue - 1.0) / H));
            const int64_t m1 = (int64_t)std::floor((ue + 2.0) / H);
            for (int64_t m = m0; m <= m1 && m < (int64_t)G.bad[hi].size(); ++m) G.bad[hi][(size_t)m] = 1;
        }
    }
}

// Stage 4: prefix scores per spacing: a good cell +w, a bad one -w, w = the cell's share of records
// (~ H / u); W0: the fine cells' weights, unsigned
struct Scores {
    std::vector<double> P[3], W0;
};
Scores prefix_scores(const GroupGrid &G) {
    Scores S;
    S.W0.assign(G.bad[0].size() + 1, 0.0);
    for (size_t m = 0; m < G.bad[0].size(); ++m) S.W0[m + 1] = S.W0[m] + 1.0 / std::max(1.0, (double)m + 0.5);
    for (int hi = 0; hi < 3; ++hi) {
        const int H = kH[hi];
        const size_t n = G.bad[hi].size();
        S.P[hi].assign(n + 1, 0.0);
        for (size_t m = 0; m < n; ++m) {
            const double w = (double)H / std::max(1.0, (double)H * ((double)m + 0.5));
            S.P[hi][m + 1] = S.P[hi][m] + (G.bad[hi][m] ? -w : w);
        }
    }
    return S;
}

// The first index of the maximum of P over a window that only grows: each [lo, hi] holds the one before
struct GrowingArgmax {
    const std::vector<double> &P;
    int64_t lo = 0, hi = -1, e = 0;
    int64_t grow(int64_t nlo, int64_t nhi) {
        if (lo > hi) lo = hi = e = nlo;  // the first, innermost window
        while (lo > nlo) {
            --lo;
            e = P[(size_t)e] > P[(size_t)lo] ? e : lo;  // (the earlier index wins a tie)
        }
        while (hi < nhi) {
            ++hi;
            e = P[(size_t)hi] > P[(size_t)e] ? hi : e;
        }
        return e;
    }
};

// The coarse rows' window of a range that turns coarse at ua (a multiple of 64): cells (ua / H, end] of the
// H grid, what the row cap leaves after the fine rows; usable when end > ua / H. It depends on ua alone,
// and shrinks at both ends as ua steps up: the usable ua are a run from the first one on.
int64_t coarse_end(const GridIn &in, const GroupGrid &G, int H, int64_t ua) {
    const int64_t uend = (int64_t)in.L - 1, left = in.cap - (ua - G.vbase);
    return ua < uend && left >= 2 ? std::min<int64_t>(ua / H + left, uend / H) : 0;
}

// Stage 5: the range [start, u1), ua and H of the best score among the candidate starts. Every best end
// the starts ask for is the first index of a maximum of P over a window from one of two nested families,
// filled from the innermost window outwards in one pass each:
//   H = 1: fine rows only, ends in (sb, hiu] -- hiu the same for every start;
//   H = 2, 4: fine rows [start, ua), coarse rows [ua, u1), ua a multiple of 64 (so hc is exact): ends in
//   (ua / H, coarse_end(ua)], whatever the start.
void choose_range(const GridIn &in, GroupGrid &G, const Scores &S) {
    const int64_t uend = (int64_t)in.L - 1;  // the rows serve u < u1lim <= L - 1
    const size_t ns = G.starts.size();
    std::vector<int64_t> sb(ns), e1(ns, -1);
    for (size_t i = 0; i < ns; ++i) sb[i] = (int64_t)std::floor(G.starts[i]);
    const int64_t hiu = std::min<int64_t>(uend, G.vbase + in.cap);
    GrowingArgmax fine{S.P[0]};
    for (size_t i = ns; i-- > 0;)
        if (hiu > sb[i]) e1[i] = fine.grow(sb[i] + 1, hiu);
    const int64_t k0 = (sb[0] + 64) / 64;  // the first start's first ua / 64
    std::vector<int64_t> ec[3];            // per H and ua / 64 - k0: the best coarse end
    for (int hi = 1; hi < 3; ++hi) {
        const int H = kH[hi];
        int64_t n = 0;
        while (coarse_end(in, G, H, 64 * (k0 + n)) > 64 * (k0 + n) / H) ++n;
        ec[hi].resize((size_t)n);
        GrowingArgmax coarse{S.P[hi]};
        for (int64_t k = n; k-- > 0;) ec[hi][(size_t)k] = coarse.grow(64 * (k0 + k) / H + 1, coarse_end(in, G, H, 64 * (k0 + k)));
    }
    G.score = 0.0;
    G.start = G.s.u0f;
    for (size_t i = 0; i < ns; ++i) {
        const double pre = S.W0[(size_t)sb[i]] - S.W0[(size_t)G.c0];  // the flagged cells before the start
        if (e1[i] >= 0) {
            const double sc = S.P[0][(size_t)e1[i]] - S.P[0][(size_t)sb[i]] - pre;
            if (sc > G.score) G.score = sc, G.start = G.starts[i], G.row_ua = e1[i], G.u1 = e1[i], G.hi = 0;
        }
        for (int hi = 1; hi < 3; ++hi) {
            const int H = kH[hi];
            for (int64_t k = (sb[i] + 64) / 64 - k0; k < (int64_t)ec[hi].size(); ++k) {
                const int64_t ua = 64 * (k0 + k), m0 = ua / H, e = ec[hi][(size_t)k];
                const double sf = S.P[0][(size_t)ua] - S.P[0][(size_t)sb[i]];
                const double sc = sf + S.P[hi][(size_t)e] - S.P[hi][(size_t)m0] - pre;
                if (sc > G.score) G.score = sc, G.start = G.starts[i], G.row_ua = ua, G.u1 = e * H, G.hi = hi;
            }
        }
    }
}

// The chosen range as the lanes' row coordinate. False: no accurate range, the exact tables past the near field.
bool lay_out_rows(GroupGrid &G) {
    if (!(G.score > 0.0) || G.u1 <= (int64_t)G.start + 1) {
        G.u1lim = G.u1start = G.s.u0f;
        return false;
    }
    if (G.hi) {
        G.hinv = 1.f / (float)G.H();
        G.hc = (float)((double)G.row_ua * (1.0 - 1.0 / G.H()));  // exact: ua a multiple of 64
        G.ua = (float)G.row_ua;
    } else {
        G.row_ua = G.u1;  // every row fine
    }
    G.ubase = (uint32_t)G.vbase;
    G.u1start = (float)G.start;  // (u0f, or an integer below 2^24)
    G.u1lim = (float)G.u1;
    return true;
}

// Stage 6: the pair rows from the near field's end to v(u1); lanes read rows <= v1 (v may round up to v1)
void emit_rows(const GridIn &in, GroupGrid &G) {
    const int64_t v1 = G.row_ua + (G.u1 - G.row_ua) / G.H();
    G.rows.reserve((size_t)(2 * (v1 - G.vbase + 1)));
    for (int64_t v = G.vbase; v <= v1; ++v) {
        const int64_t u = G.upos(v), un = G.upos(v + 1);
        float vv[4][2];
        for (int j = 0; j < 4; ++j) {
            vv[j][0] = cg_R(in.tab, in.L, G.band[j], G.s.r[j], u);
            vv[j][1] = cg_R(in.tab, in.L, G.band[j], G.s.r[j], un);
        }
        if (G.cell_bad(v)) vv[0][0] = NAN;  // its lanes read the bands' own tables (cg_fix)
        G.rows.push_back(make_float4(vv[0][0], vv[0][1], vv[1][0], vv[1][1]));
        G.rows.push_back(make_float4(vv[2][0], vv[2][1], vv[3][0], vv[3][1]));
    }
}

// Stage 7: each slot's error over the knots the good rows serve
void sum_errors(const GridIn &in, GroupGrid &G) {
    const int L = in.L;
    const int64_t ua = G.row_ua;
    for (int j = 0; j < 4; ++j) {
        const int c = G.band[j];
        if (c < 0) continue;
        const float *T = in.tab + (size_t)c * L;
        const double rj = G.s.r[j];
        double l1 = 0.0, emax = 0.0, esum = 0.0;
        for (int k = 0; k < L; ++k) l1 += std::fabs(T[k]);
        for (int k = cg_first_knot(G.start, rj); k < L - 1; ++k) {
            const double u = (double)k / rj;
            if (u < G.start) continue;
            if (u >= (double)G.u1) break;
            const int Hk = u < (double)ua ? 1 : G.H();
            const int64_t v = u < (double)ua ? (int64_t)std::floor(u) : ua + (int64_t)std::floor((u - ua) / G.H());
            if (G.cell_bad(v)) continue;
            // (relative error -- to cg_scale: the band's own value, or the largest of R, G, B -- where
            // the relative bound governs: scale >= kCgAbsTol / kCgRelTol of the peak)
            const double sc = cg_scale(in.tab, L, G.band, G.s.r, j, k, in.rgb);
            const double e = cg_knot_err(in.tab, L, c, rj, k, Hk, cg_max(kCgRelTol * sc, kCgAbsTol * G.peak[j]));
            if (kCgRelTol * sc >= kCgAbsTol * G.peak[j]) emax = std::max(emax, e / sc);
            esum += e;
        }
        G.rel[j] = (float)emax;
        G.l1[j] = (float)(l1 > 0.0 ? esum / l1 : 0.0);
    }
}

void build_group(const GridIn &in, const CgScan *pre, int g, GroupGrid &G) {
    if (!split_and_tau(in, G)) return;
    for (int hi = 0; hi < 3; ++hi) G.bad[hi].assign((size_t)(in.L + 2) / kH[hi] + 2, 0);
    if (pre)
        take_scan(*pre, g, G);
    else
        scan_knots(in, G);
    candidate_starts(in, G);
    flag_profile_ends(in, G);
    choose_range(in, G, prefix_scores(G));
    if (!lay_out_rows(G)) return;
    emit_rows(in, G);
    sum_errors(in, G);
    G.any = true;
}

}  // namespace

bool build_common_grid(const float *tab, int L, const float *host_rcp, const BandGroups &groups, CommonGrid &cg,
                       std::vector<float4> &h, float cg_rel_err[NB], float cg_l1_err[NB], int near_field,
                       int lds_reserve, bool rgb, const CgScan *pre) {
    cg = CommonGrid{};
    for (int g = 0; g < kGroups; ++g) {  // (one row per grid step unless a group's layout says otherwise)
        cg.hinv[g] = 1.f;
        cg.hc[g] = 0.f;
        cg.ua[g] = (float)L;
    }
    h.clear();
    for (int c = 0; c < NB; ++c) cg_rel_err[c] = cg_l1_err[c] = 0.f;
    if (!cg_can_build(L, host_rcp, groups)) return false;
    const GridIn in{tab, L, host_rcp, 4 * (near_field + 3) - lds_reserve, rgb, cg_max_rows()};
    // The groups are independent (their own slots, LDS split, rows and errors): each is built on its
    // own thread, then laid out in group order. (For the rgbprofile all groups hold the same three
    // slots: one group is built and copied.)
    std::vector<GroupGrid> G(kGroups);
    for (int g = 0; g < kGroups; ++g) {
        for (int j = 0; j < 4; ++j) G[g].band[j] = groups.band[g][j];
        G[g].ua = (float)L;
    }
    if (cg_same_slots(groups, rgb)) {
        build_group(in, pre, 0, G[0]);
        for (int g = 1; g < kGroups; ++g) G[g] = G[0];
    } else {
        std::vector<std::thread> th;
        for (int g = 0; g < kGroups; ++g) th.emplace_back(build_group, std::cref(in), pre, g, std::ref(G[g]));
        for (std::thread &t : th) t.join();
    }
    bool any = false, failed = false;
    for (int g = 0; g < kGroups; ++g) {
        const GroupGrid &s = G[g];
        cg.rg[g] = s.rg, cg.u0lim[g] = s.u0lim, cg.u1lim[g] = s.u1lim, cg.u1start[g] = s.u1start;
        cg.ua[g] = s.ua, cg.hinv[g] = s.hinv, cg.hc[g] = s.hc, cg.lds_r2[g] = s.lds_r2, cg.ubase[g] = s.ubase;
        for (int j = 0; j < 4; ++j) cg.tau[g][j] = s.tau[j], cg.lrow[g][j] = s.lrow[j], cg.lcnt[g][j] = s.lcnt[j];
        if ((failed = failed || s.fail)) continue;  // a group without a split: no grid, nothing more is laid out
        cg.row0[g] = (uint32_t)(h.size() / 2);
        h.insert(h.end(), s.rows.begin(), s.rows.end());
        any = any || s.any;
        for (int j = 0; j < 4; ++j) {
            const int c = s.band[j];
            if (c < 0) continue;
            cg_rel_err[c] = std::max(cg_rel_err[c], s.rel[j]);
            cg_l1_err[c] = std::max(cg_l1_err[c], s.l1[j]);
        }
    }
    if (failed) return false;
    cg.on = any ? 1 : 0;
    return any;
}

}  // namespace mpss
