// mo_exact.hip -- the Mo() gather in the reference's summation order: a checking path (exact_mo 1, the
// dipole and rgbprofile functors), bit-identical to the CPU oracle.
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
// Exact pruning (mo_band.h prune_limit): every point of a subtree and its clusters' centroids lie
// inside the node's box, so a subtree past the limit adds only +0 terms in the reference and is skipped
// here without changing a bit of the result. The COUNT variant reports both the reference traversal's
// visits and the pruned traversal's visits (SURVEY.md 8d counters).
#include "dipole.h"
#include "mo_args.h"
#include "spectrum_tables.h"

namespace mpss {

namespace {

// Rd functors of the reference-order gather: the tabulated spectral profile, the closed-form
// single dipole (DiffusionReflectance), and the RGB profile (rgbprofile: three tables, Rd =
// SampledSpectrum::FromRGB(reflectance) of the three lookups, multipole.cpp:85-107).
enum { FN_TABLE = 0, FN_DIPOLE = 1, FN_RGB = 2 };

__device__ __forceinline__ float rd_lerp(const float *__restrict__ tb, float f) {
    const uint32_t s = (uint32_t)f;
    const float t = f - (float)s;
    const float a = tb[s], b = tb[s + 1];
    return (1.f - t) * a + t * b;
}

// MultipoleProfileData::reflectance with isRGBProfile (multipole.cpp:85-107): sampleProfile of
// the R, G, B tables, then band c of Spectrum::FromRGBSpectrum (spectrum_tables.h refl_band)
__device__ __forceinline__ float rgb_rd(const float *__restrict__ table, int L, const float rcp3[3], float lm1, float d2,
                                        int c) {
    float v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = d2 * rcp3[k];
        v[k] = f < lm1 ? rd_lerp(table + (size_t)k * L, f) : 0.f;
    }
    return refl_band(v, c);
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

void launch_mo_exact(const DeviceOctree &t, const DeviceProfile &p, float max_error, int nq, const float *queries,
                     float *out, int out_stride, int32_t *counters, hipStream_t stream) {
    const MoArgs a = mo_args(t, p, nq, queries, out, out_stride, counters, max_error);
    launch_exact<FN_TABLE>(a, t.max_depth, counters != nullptr, stream);
}

void launch_mo_dipole(const DeviceOctree &t, const float *dipole_dev, float max_error, int nq, const float *queries,
                      float *out, int out_stride, int32_t *counters, hipStream_t stream) {
    if (nq <= 0) return;
    if (t.n_nodes <= 0) throw Error(-1, "launch_mo_dipole: octree is empty");
    MoArgs a = mo_args(t, nq, queries, out, out_stride, counters, max_error);
    a.L = 2;
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
    MoArgs a = mo_args(t, nq, queries, out, out_stride, counters, max_error);
    a.table = table3;
    a.rcp = rcp3_dev;
    a.queries4 = queries4;
    a.count = count_dev;
    a.hit_s = hit_s;
    a.mat = mat;
    a.L = L;
    // every band is FromRGB of the three lookups: +0 once all three are past their table's end
    float rmin = rcp3[0] < rcp3[1] ? rcp3[0] : rcp3[1];
    rmin = rcp3[2] < rmin ? rcp3[2] : rmin;
    const PruneLimit pl = prune_limit(L, rmin);
    a.rcp_min = pl.rcp_min;
    a.prune_f = pl.prune_f;
    launch_exact<FN_RGB>(a, t.max_depth, counters != nullptr, stream);
}

}  // namespace mpss
