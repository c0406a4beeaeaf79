// mo_kernel.hip -- the Mo() hierarchical irradiance gather on CDNA4 (gfx950).
//
// Computes, for each query point p, SubsurfaceOctreeNode::Mo(octreeBounds, p, ...)
// (reference src/integrators/diffusionutil.h:175-210) with the multipole profile
// Rd(d^2) of MultipoleProfileData::reflectance (src/core/multipole.cpp:60-113).
//
// Mapping: one wave64 = two queries; each 32-lane half-wave owns one query and lane
// c = lane & 31 owns spectral band c (30 bands, lanes 30/31 idle). The traversal is
// stackless over the pre-order node array (skip pointers, octree.h), so control flow is
// uniform inside a half-wave. Every node record and every spectral row is read by the
// half-wave as one coalesced 128-B line (Et/E) plus one broadcast 64-B header.
//
// Summation order is the reference's recursion order: S[d][lane] in LDS holds the
// running sum of the children of the open node at depth d-1; a finished subtree is
// folded into its parent level on the way back up. With FP contraction disabled
// (-ffp-contract=off) every product and sum rounds exactly as the reference's scalar
// code, so the result is bit-identical to the CPU oracle.
//
// Exact pruning: sampleProfile returns exactly 0 once d^2 * rcpDsqSpacing >= L-1
// (multipole.cpp:63-66). Every point of a subtree and its clusters' centroids lie inside the
// node's box, so if the box's squared distance to p times the smallest rcp over bands is past
// L-1 (with a 1e-4 relative margin that dominates float rounding of the two distances), the
// whole subtree adds only +0 terms in the reference and is skipped here without changing a
// bit of the result. The COUNT variant reports both the reference traversal's visits and the
// pruned traversal's visits (SURVEY.md 8d counters).
#include "dipole.h"
#include "mo_kernel.h"
#include "spectral.h"
#include "mo_packet.h"
#include "mo_wave.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace mpss {

namespace {

struct MoArgs {
    const NodeHdr *__restrict__ nodes;
    const float *__restrict__ node_et;
    const float4 *__restrict__ pt_hdr;
    const float *__restrict__ pt_e;
    const float *__restrict__ table;    // [NB][L]
    const float *__restrict__ rcp;      // [NB]
    const float *__restrict__ queries;  // q * 3
    float *__restrict__ out;            // q * out_stride
    int32_t *__restrict__ counters;     // COUNT: q * 4
    int L, n_nodes, nq, out_stride;
    float max_error, prune_f;           // prune when d2box * rcp_min >= prune_f
    float rcp_min;
    const float *__restrict__ dipole;   // FN_DIPOLE: [4][NB] zpos, zneg, sigma_tr, k (dipole.h)
    // render path (instead of queries): queries4[i] = {p, w} (w < 0: no BSSRDF), i < *count, and
    // with hit_s the material filter; out[i * out_stride + c]
    const float4 *__restrict__ queries4;
    const int *__restrict__ count;
    const uint32_t *__restrict__ hit_s;
    int mat;
};

// Rd functors of the reference-order gather: the tabulated spectral profile, the closed-form
// single dipole (DiffusionReflectance), and the RGB profile (rgbprofile: three tables, Rd =
// SampledSpectrum::FromRGB(reflectance) of the three lookups, multipole.cpp:85-107).
enum { FN_TABLE = 0, FN_DIPOLE = 1, FN_RGB = 2 };

// rgbRefl2Spect{White, Cyan, Magenta, Yellow, Red, Green, Blue} (spectrum.cpp, SampledSpectrum::Init)
__constant__ float kRefl[7][NB] = {MPSS_BAND_RGBREFL2SPECTWHITE_INIT, MPSS_BAND_RGBREFL2SPECTCYAN_INIT,
                                   MPSS_BAND_RGBREFL2SPECTMAGENTA_INIT, MPSS_BAND_RGBREFL2SPECTYELLOW_INIT,
                                   MPSS_BAND_RGBREFL2SPECTRED_INIT, MPSS_BAND_RGBREFL2SPECTGREEN_INIT,
                                   MPSS_BAND_RGBREFL2SPECTBLUE_INIT};

// Band c of SampledSpectrum::FromRGB(rgb, SPECTRUM_REFLECTANCE) (spectrum.cpp:103-186): the same
// float operations as the 30-band code (spectral.cpp spectrum_from_rgb), one band.
__device__ __forceinline__ float from_rgb_band(float R, float G, float B, int c) {
    enum { W = 0, CY = 1, MG = 2, YE = 3, RD = 4, GR = 5, BL = 6 };
    float r = 0.f;
    if (R <= G && R <= B) {
        r += kRefl[W][c] * R;
        if (G <= B) { r += kRefl[CY][c] * (G - R); r += kRefl[BL][c] * (B - G); }
        else { r += kRefl[CY][c] * (B - R); r += kRefl[GR][c] * (G - B); }
    } else if (G <= R && G <= B) {
        r += kRefl[W][c] * G;
        if (R <= B) { r += kRefl[MG][c] * (R - G); r += kRefl[BL][c] * (B - R); }
        else { r += kRefl[MG][c] * (B - G); r += kRefl[RD][c] * (R - B); }
    } else {
        r += kRefl[W][c] * B;
        if (R <= G) { r += kRefl[YE][c] * (R - B); r += kRefl[GR][c] * (G - R); }
        else { r += kRefl[YE][c] * (G - B); r += kRefl[RD][c] * (R - G); }
    }
    const float v = r * (float).94;
    return v < 0.f ? 0.f : v;  // Clamp(0, INFINITY)
}

__device__ __forceinline__ float rd_lerp(const float *__restrict__ tb, float f) {
    const uint32_t s = (uint32_t)f;
    const float t = f - (float)s;
    const float a = tb[s], b = tb[s + 1];
    return (1.f - t) * a + t * b;
}

// MultipoleProfileData::reflectance with isRGBProfile (multipole.cpp:85-107): sampleProfile of
// the R, G, B tables, then band c of Spectrum::FromRGBSpectrum
__device__ __forceinline__ float rgb_rd(const float *__restrict__ table, int L, const float rcp3[3], float lm1, float d2,
                                        int c) {
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = d2 * rcp3[k];
        v[k] = f < lm1 ? rd_lerp(table + (size_t)k * L, f) : 0.f;
    }
    return from_rgb_band(v[0], v[1], v[2], c);
}

__device__ __forceinline__ float box_d2(float px, float py, float pz, const NodeHdr &h) {
    const float bx = fmaxf(fmaxf(h.bminx - px, px - h.bmaxx), 0.f);
    const float by = fmaxf(fmaxf(h.bminy - py, py - h.bmaxy), 0.f);
    const float bz = fmaxf(fmaxf(h.bminz - pz, pz - h.bmaxz), 0.f);
    return bx * bx + by * by + bz * bz;
}

// FN_DIPOLE: the Rd functor is the closed-form single dipole (DiffusionReflectance, dipole.h)
// instead of the tabulated profile; it never returns an exact 0 past a range, so nothing is
// pruned. FN_RGB: a.table holds the R, G, B profiles ([3][L]) and a.rcp their rcpDsqSpacing; the
// three lookups are wave-uniform per half-wave, each lane converts them to its band.
template <int MAXD, bool COUNT, int FN>
__global__ __launch_bounds__(256) void mo_gather_kernel(MoArgs a) {
    constexpr bool DIP = FN == FN_DIPOLE;
    __shared__ float S[4][MAXD + 1][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int c = lane & 31;
    const int q = ((int)blockIdx.x * 4 + wave) * 2 + (lane >> 5);
    bool active = q < a.nq;
    float(*St)[64] = S[wave];

    float px = 0.f, py = 0.f, pz = 0.f;
    if (a.queries4) {  // render path: the compacted hit list (count on the device) and its filter
        if (active) active = q < *a.count;
        if (active) {
            const float4 v = a.queries4[q];
            px = v.x;
            py = v.y;
            pz = v.z;
            active = v.w >= 0.f && (!a.hit_s || (int)((a.hit_s[q] >> 16) & 0xffu) == a.mat);
        }
    } else if (active) {
        px = a.queries[3 * (size_t)q];
        py = a.queries[3 * (size_t)q + 1];
        pz = a.queries[3 * (size_t)q + 2];
    }
    const float rcp = (FN == FN_TABLE && c < NB) ? a.rcp[c] : INFINITY;
    float rcp3[3] = {0.f, 0.f, 0.f};
    if (FN == FN_RGB)
        for (int k = 0; k < 3; ++k) rcp3[k] = a.rcp[k];
    const float lm1 = (float)(a.L - 1);
    const float *__restrict__ tb = a.table + (size_t)(c < NB ? c : 0) * a.L;
    float dzp = 0.f, dzn = 0.f, dtr = 0.f, dk = 0.f;
    if (DIP) {
        const int cc = c < NB ? c : 0;
        dzp = a.dipole[cc];
        dzn = a.dipole[NB + cc];
        dtr = a.dipole[2 * NB + cc];
        dk = a.dipole[3 * NB + cc];
    }

    int node = active ? 0 : a.n_nodes;
    int dlast = 0;
    St[0][lane] = 0.f;
    // COUNT: reference visits (no pruning) and pruned-kernel visits
    int ref_nodes = 0, ref_pts = 0, k_nodes = 0, k_pts = 0, pruned_until = 0;

    while (node < a.n_nodes) {
        const NodeHdr h = a.nodes[node];
        const int d = h.depth;
        while (dlast > d) {  // close finished subtrees (return from the recursion)
            St[dlast - 1][lane] += St[dlast][lane];
            --dlast;
        }
        int next = h.skip;
        const bool prune = box_d2(px, py, pz, h) * a.rcp_min >= a.prune_f;
        if (COUNT) {
            ++ref_nodes;
            if (node >= pruned_until) {
                ++k_nodes;
                if (prune) pruned_until = h.skip;
            }
        } else if (prune) {
            node = next;
            continue;
        }
        if (!(h.flags & NODE_BLACK)) {
            const float dx = px - h.px, dy = py - h.py, dz = pz - h.pz;
            const float d2 = dx * dx + dy * dy + dz * dz;
            const float dw = h.sum_area / d2;
            const bool inside = px >= h.bminx && px <= h.bmaxx && py >= h.bminy && py <= h.bmaxy &&
                                pz >= h.bminz && pz <= h.bmaxz;
            if (dw < a.max_error && !inside) {
                if (DIP) {
                    St[d][lane] += dipole_band(dzp, dzn, dtr, dk, d2) * a.node_et[(size_t)node * ROW + c];
                } else if (FN == FN_RGB) {
                    St[d][lane] += rgb_rd(a.table, a.L, rcp3, lm1, d2, c < NB ? c : 0) * a.node_et[(size_t)node * ROW + c];
                } else {
                    const float f = d2 * rcp;
                    if (f < lm1) St[d][lane] += rd_lerp(tb, f) * a.node_et[(size_t)node * ROW + c];
                }
            } else if (h.leaf_first >= 0) {
                float acc = 0.f;
                for (int i = 0; i < h.leaf_count; ++i) {
                    const int k = h.leaf_first + i;
                    const float4 ph = a.pt_hdr[k];
                    if (__builtin_signbit(ph.w)) continue;  // E is black
                    if (COUNT) {
                        ++ref_pts;
                        if (node >= pruned_until) ++k_pts;
                    }
                    const float ex = px - ph.x, ey = py - ph.y, ez = pz - ph.z;
                    if (DIP) {
                        acc += dipole_band(dzp, dzn, dtr, dk, ex * ex + ey * ey + ez * ez) *
                               a.pt_e[(size_t)k * ROW + c] * ph.w;
                        continue;
                    }
                    if (FN == FN_RGB) {
                        acc += rgb_rd(a.table, a.L, rcp3, lm1, ex * ex + ey * ey + ez * ez, c < NB ? c : 0) *
                               a.pt_e[(size_t)k * ROW + c] * ph.w;
                        continue;
                    }
                    const float f = (ex * ex + ey * ey + ez * ez) * rcp;
                    if (f < lm1) acc += rd_lerp(tb, f) * a.pt_e[(size_t)k * ROW + c] * ph.w;
                }
                St[d][lane] += acc;
            } else {  // open the node: recurse into its children
                next = node + 1;
                St[d + 1][lane] = 0.f;
                dlast = d + 1;
            }
        }
        node = next;
    }
    while (dlast > 0) {
        St[dlast - 1][lane] += St[dlast][lane];
        --dlast;
    }
    if (active && c < NB) a.out[(size_t)q * a.out_stride + c] = St[0][lane];
    if (COUNT && active && c == 0) {
        int4 v = {ref_nodes, ref_pts, k_nodes, k_pts};
        reinterpret_cast<int4 *>(a.counters)[q] = v;
    }
}

// ---------------------------------------------------------------------------------------
// Packet kernel (default): one wave64 = a packet of 8 queries x 8 band-groups of 4 bands.
// The 8 queries (consecutive in the caller's order: samples of one pixel / neighbouring
// shading points) walk the UNION of their pruned traversals once: node headers and leaf
// point headers are wave-uniform scalar loads, Et/E rows are one 128-B line per wave, and
// each lane owns 4 bands of one query. A query that does not open node j (it pruned it,
// took its cluster contribution, or the node is black) sits out until j's skip index.
// Per query the visited node set, the decisions and every product are those of the
// reference; only the order of the final float additions differs (one running sum per
// band instead of the recursion's per-level sums), so results agree with the reference
// order to float reassociation (tests bound it at 2e-5 relative; north star: 1e-4).
// ---------------------------------------------------------------------------------------
template <bool COUNT>
__global__ __launch_bounds__(256) void mo_packet_kernel(MoArgs a, int nblocks) {
    const int lb = xcd_remap((int)blockIdx.x, nblocks);
    const int lane = threadIdx.x & 63;
    const int g = lane >> 3, k = lane & 7;
    const int q = (lb * 4 + (int)(threadIdx.x >> 6)) * 8 + g;
    const bool valid = q < a.nq;
    float px = 0.f, py = 0.f, pz = 0.f;
    if (valid) {
        px = a.queries[3 * (size_t)q];
        py = a.queries[3 * (size_t)q + 1];
        pz = a.queries[3 * (size_t)q + 2];
    }
    PacketTree t{a.nodes, a.node_et, a.pt_hdr, a.pt_e, a.table, a.rcp, a.L, a.n_nodes, a.max_error, a.prune_f,
                 a.rcp_min};
    float acc[4];
    int kn = 0, kp = 0, un = 0;
    mo_packet_traverse<COUNT>(t, px, py, pz, valid, k, acc, kn, kp, &un);
    if (valid) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * k + j;
            if (c < NB) a.out[(size_t)q * a.out_stride + c] = acc[j];
        }
        if (COUNT && k == 0) {
            int4 v = {un, 0, kn, kp};  // packet: wave (union) iterations, -, own nodes, own points
            reinterpret_cast<int4 *>(a.counters)[q] = v;
        }
    }
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
        static const float refl[7][NB] = {MPSS_BAND_RGBREFL2SPECTWHITE_INIT, MPSS_BAND_RGBREFL2SPECTCYAN_INIT,
                                          MPSS_BAND_RGBREFL2SPECTMAGENTA_INIT, MPSS_BAND_RGBREFL2SPECTYELLOW_INIT,
                                          MPSS_BAND_RGBREFL2SPECTRED_INIT, MPSS_BAND_RGBREFL2SPECTGREEN_INIT,
                                          MPSS_BAND_RGBREFL2SPECTBLUE_INIT};
        for (int g = 0; g < kGroups; ++g)
            for (int s2 = 0; s2 < 4; ++s2) {
                const int c = p.groups.band[g][s2];
                auto at = [&](int t) { return c >= 0 ? refl[t][c] : 0.f; };
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
    bt.prune_f = (p.rcp_min > 0.f) ? (float)(p.L - 1) * 1.0001f : INFINITY;
    if (!(p.rcp_min > 0.f))
        for (int g = 0; g < kGroups; ++g) bt.groups.rcp_min[g] = 0.f;  // rcp <= 0: no pruning
    return bt;
}

template <int MAXD, int FN>
void launch_t(const MoArgs &a, bool count, hipStream_t s) {
    const int waves = (a.nq + 1) / 2;
    const int blocks = (waves + 3) / 4;
    if (blocks == 0) return;
    if (count)
        hipLaunchKernelGGL((mo_gather_kernel<MAXD, true, FN>), dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((mo_gather_kernel<MAXD, false, FN>), dim3(blocks), dim3(256), 0, s, a);
}

template <int FN>
void launch_exact(const MoArgs &a, int max_depth, bool count, hipStream_t s) {
    if (max_depth < 16)
        launch_t<16, FN>(a, count, s);
    else if (max_depth < 32)
        launch_t<32, FN>(a, count, s);
    else if (max_depth < 64)
        launch_t<64, FN>(a, count, s);
    else
        throw Error(-2, "octree deeper than 63 levels is not supported by the gather kernel");
    MPSS_HIP(hipGetLastError());
}

}  // namespace

// The device copy moves each leaf's black points (E == 0: every kernel skips them, they add
// nothing) behind its other points, keeping the others' order, and records the count of the
// rest in NodeHdr::pad's low half (a leaf holds at most 8 points), so the sharded gather's leaf loop
// needs no per-point test. (The high half: ensure_leaf_r2's leaf code.)
void DeviceOctree::upload(const FlatOctree &t) {
    std::vector<NodeHdr> hdr = t.hdr;
    std::vector<float> ph(t.pt_hdr.size()), pe(t.pt_e.size());
    std::vector<int> pidx(t.pt_index.size());
    for (NodeHdr &h : hdr) {
        h.pad = 0;
        if (h.leaf_first < 0) continue;
        int o = h.leaf_first;
        for (int pass = 0; pass < 2; ++pass)
            for (int i = 0; i < h.leaf_count; ++i) {
                const size_t k = (size_t)h.leaf_first + i;
                const bool blk = std::signbit(t.pt_hdr[4 * k + 3]);
                if (blk != (pass == 1)) continue;
                memcpy(&ph[4 * (size_t)o], &t.pt_hdr[4 * k], 4 * sizeof(float));
                memcpy(&pe[(size_t)o * ROW], &t.pt_e[k * ROW], ROW * sizeof(float));
                pidx[o] = t.pt_index[k];
                ++o;
                if (pass == 0) ++h.pad;
            }
    }
    layouts.clear();
    leaf_r2_error = -1.f;
    nodes.upload(hdr.data(), hdr.size());
    node_et.upload(t.node_et.data(), t.node_et.size());
    pt_hdr.upload(reinterpret_cast<const float4 *>(ph.data()), ph.size() / 4);
    pt_e.upload(pe.data(), pe.size());
    pt_index.upload(pidx.data(), pidx.size());
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
                      int mode, const GatherOpts &opts, hipStream_t stream) {
    const bool exact = mode == 1;
    if (nq <= 0) return;
    if (t.n_nodes <= 0) throw Error(-1, "launch_mo_gather: octree is empty");
    if (p.L < 2) throw Error(-1, "launch_mo_gather: profile table has fewer than 2 entries");
    const bool count = counters != nullptr;
    if (mode == 0) {
        if (!layout || !work) throw Error(-2, "launch_mo_gather: the sharded gather needs a band layout and work counters");
        if (count) MPSS_HIP(hipMemsetAsync(counters, 0, sizeof(int32_t) * 4 * (size_t)nq, stream));
        BandArgs b{};
        b.t = band_tree(t, *layout, p, max_error);
        b.queries3 = queries;
        b.nq = nq;
        b.out = out;
        b.out_stride = out_stride;
        b.counters = counters;
        b.work = work;
        b.perm = perm;
        launch_band(b, nq, t, count, opts, stream);
        return;
    }
    MoArgs a{};  // value-initialized: unused fields (render-path queries, functor tables) are null
    a.nodes = t.nodes.ptr;
    a.node_et = t.node_et.ptr;
    a.pt_hdr = t.pt_hdr.ptr;
    a.pt_e = t.pt_e.ptr;
    a.table = p.table.ptr;
    a.rcp = p.rcp.ptr;
    a.queries = queries;
    a.out = out;
    a.counters = counters;
    a.L = p.L;
    a.n_nodes = t.n_nodes;
    a.nq = nq;
    a.out_stride = out_stride;
    a.max_error = max_error;
    a.rcp_min = p.rcp_min > 0.f ? p.rcp_min : 0.f;  // rcp_min <= 0 disables pruning
    a.prune_f = (a.rcp_min > 0.f) ? (float)(p.L - 1) * 1.0001f : INFINITY;
    if (!exact) {
        const int packets = (nq + 7) / 8, blocks = (packets + 3) / 4;
        if (count)
            hipLaunchKernelGGL((mo_packet_kernel<true>), dim3(blocks), dim3(256), 0, stream, a, blocks);
        else
            hipLaunchKernelGGL((mo_packet_kernel<false>), dim3(blocks), dim3(256), 0, stream, a, blocks);
        MPSS_HIP(hipGetLastError());
        return;
    }
    a.dipole = nullptr;
    launch_exact<FN_TABLE>(a, t.max_depth, count, stream);
}

void launch_mo_dipole(const DeviceOctree &t, const float *dipole_dev, float max_error, int nq, const float *queries,
                      float *out, int out_stride, int32_t *counters, hipStream_t stream) {
    if (nq <= 0) return;
    if (t.n_nodes <= 0) throw Error(-1, "launch_mo_dipole: octree is empty");
    MoArgs a{};
    a.nodes = t.nodes.ptr;
    a.node_et = t.node_et.ptr;
    a.pt_hdr = t.pt_hdr.ptr;
    a.pt_e = t.pt_e.ptr;
    a.queries = queries;
    a.out = out;
    a.counters = counters;
    a.L = 2;
    a.n_nodes = t.n_nodes;
    a.nq = nq;
    a.out_stride = out_stride;
    a.max_error = max_error;
    a.rcp_min = 0.f;
    a.prune_f = INFINITY;
    a.dipole = dipole_dev;
    launch_exact<FN_DIPOLE>(a, t.max_depth, counters != nullptr, stream);
}

void launch_mo_rgb(const DeviceOctree &t, const float *table3, const float *rcp3_dev, const float rcp3[3], int L,
                   float max_error, int nq, const float *queries, const float4 *queries4, const int *count_dev,
                   const uint32_t *hit_s, int mat, float *out, int out_stride, int32_t *counters, hipStream_t stream) {
    if (nq <= 0) return;
    if (t.n_nodes <= 0) throw Error(-1, "launch_mo_rgb: octree is empty");
    if (L < 2) throw Error(-1, "launch_mo_rgb: profile table has fewer than 2 entries");
    MoArgs a{};
    a.nodes = t.nodes.ptr;
    a.node_et = t.node_et.ptr;
    a.pt_hdr = t.pt_hdr.ptr;
    a.pt_e = t.pt_e.ptr;
    a.table = table3;
    a.rcp = rcp3_dev;
    a.queries = queries;
    a.queries4 = queries4;
    a.count = count_dev;
    a.hit_s = hit_s;
    a.mat = mat;
    a.out = out;
    a.counters = counters;
    a.L = L;
    a.n_nodes = t.n_nodes;
    a.nq = nq;
    a.out_stride = out_stride;
    a.max_error = max_error;
    // every band is FromRGB of the three lookups: +0 once all three are past their table's end
    float rmin = rcp3[0] < rcp3[1] ? rcp3[0] : rcp3[1];
    rmin = rcp3[2] < rmin ? rcp3[2] : rmin;
    a.rcp_min = rmin > 0.f ? rmin : 0.f;
    a.prune_f = (a.rcp_min > 0.f) ? (float)(L - 1) * 1.0001f : INFINITY;
    launch_exact<FN_RGB>(a, t.max_depth, counters != nullptr, stream);
}

}  // namespace mpss
