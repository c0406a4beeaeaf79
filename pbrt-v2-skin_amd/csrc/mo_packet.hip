// mo_packet.hip -- the packet Mo() gather of mpss_mo_batch (launch_mo_gather's mode 2): a checking path
// whose sums the sharded gather's per-band tables match bit for bit (mo_band.h).
#include "mo_args.h"
#include "mo_packet.h"

namespace mpss {

namespace {

// ---------------------------------------------------------------------------------------
// Packet kernel: one wave64 = a packet of 8 queries x 8 band-groups of 4 bands.
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

}  // namespace

void launch_mo_packet(const DeviceOctree &t, const DeviceProfile &p, float max_error, int nq, const float *queries,
                      float *out, int out_stride, int32_t *counters, hipStream_t stream) {
    const MoArgs a = mo_args(t, p, nq, queries, out, out_stride, counters, max_error);
    const int packets = (nq + 7) / 8, blocks = (packets + 3) / 4;
    if (counters)
        hipLaunchKernelGGL((mo_packet_kernel<true>), dim3(blocks), dim3(256), 0, stream, a, blocks);
    else
        hipLaunchKernelGGL((mo_packet_kernel<false>), dim3(blocks), dim3(256), 0, stream, a, blocks);
    MPSS_HIP(hipGetLastError());
}

}  // namespace mpss
