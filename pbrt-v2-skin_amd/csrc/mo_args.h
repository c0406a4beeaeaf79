// mo_args.h -- private to the two checking paths of the Mo() gather, mo_exact.hip (reference order) and
// mo_packet.hip: the kernel arguments they share and one fill of them.
#pragma once
#include "mo_kernel.h"

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

// The tree, the queries and the outputs; value-initialized, so what a launcher does not set (the
// render-path queries, the functor tables) is null. Every launcher sets L and the pruning pair.
inline MoArgs mo_args(const DeviceOctree &t, int nq, const float *queries, float *out, int out_stride,
                      int32_t *counters, float max_error) {
    MoArgs a{};
    a.nodes = t.nodes.ptr;
    a.node_et = t.node_et.ptr;
    a.pt_hdr = t.pt_hdr.ptr;
    a.pt_e = t.pt_e.ptr;
    a.queries = queries;
    a.out = out;
    a.counters = counters;
    a.n_nodes = t.n_nodes;
    a.nq = nq;
    a.out_stride = out_stride;
    a.max_error = max_error;
    return a;
}

// ... with a tabulated spectral profile and its pruning limit (modes 1 and 2)
inline MoArgs mo_args(const DeviceOctree &t, const DeviceProfile &p, int nq, const float *queries, float *out,
                      int out_stride, int32_t *counters, float max_error) {
    MoArgs a = mo_args(t, nq, queries, out, out_stride, counters, max_error);
    a.table = p.table.ptr;
    a.rcp = p.rcp.ptr;
    a.L = p.L;
    const PruneLimit pl = prune_limit(p.L, p.rcp_min);
    a.rcp_min = pl.rcp_min;
    a.prune_f = pl.prune_f;
    return a;
}

}  // namespace

}  // namespace mpss
