// mc_profile_batch.hip -- the random walk of mc_profile.hip over a batch of slabs in one kernel
// (Renderer "batchmcprofile", reference src/renderers/batchmcprofile.cpp:43-100, which runs one
// MonteCarloProfileRenderer per top-layer thickness).
//
// Work items are (slab, run of kMcPool photon ids), numbered slab-major and taken from one global
// counter, one atomic per run and wave. A lane whose photon has finished is refilled from its wave's
// current run, so the long-lived last photons of one slab run beside the first photons of the next:
// lanes of one wave can be in different slabs, and each lane carries its own slab index and reads the
// slab's constants (McScene) from a device table through it -- the walk's per-layer constants are
// indexed by the lane's layer already, so they are vector loads either way.
// Photon k of every slab draws McRng::init(seed, k), and the step is mc_walk_event, the single kernel's:
// a slab's tallies hold the same terms as mpss_mc_profile's, summed in another order.
// Tallies: rings mode adds each exit to [nslabs][nsegments] global arrays (one FP64 atomic per
// photon, spread over the rings). Totals-only mode keeps a per-lane FP64 sum tagged with the lane's
// slab; when a refill moves lanes to another slab, the lanes leaving the same slab are summed across
// the wave and added to the slab's global totals by one lane. No LDS in either mode.
#include "mc_walk.h"

#include <algorithm>
#include <vector>

namespace mpss {

namespace {

struct McBatchArgs {
    const McScene *slabs;  // [nslabs]
    uint64_t nphotons, seed;        // per slab
    uint64_t runs_per_slab, nruns;  // work items: nruns = nslabs * runs_per_slab
    unsigned long long *next;       // work-item counter
    double *refl, *trans;           // rings mode: [nslabs][nsegments]
    double *tot;                    // totals-only mode: [nslabs][2]
    unsigned long long *events;
    int nsegments;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Wave-uniform call. Lanes with pred hand their sums to tot[slab]: per distinct slab among them one
// cross-wave sum and one lane's pair of atomics.
__device__ __forceinline__ void flush_totals(bool pred, int slab, double &acc_r, double &acc_t, double *tot, int lane) {
    uint64_t m = __builtin_amdgcn_ballot_w64(pred);
    while (m) {
        const int leader = __builtin_ctzll(m);
        const int s = __shfl(slab, leader);
        const bool mine = pred && slab == s;
        const double r = wave_sum(mine ? acc_r : 0.), t = wave_sum(mine ? acc_t : 0.);
        if (lane == leader) {
            if (r != 0.) atomicAdd(tot + 2 * (size_t)s, r);
            if (t != 0.) atomicAdd(tot + 2 * (size_t)s + 1, t);
        }
        if (mine) {
            acc_r = acc_t = 0.;
            pred = false;
        }
        m = __builtin_amdgcn_ballot_w64(pred);
    }
}

template <bool RINGS>
__global__ __launch_bounds__(256) void mc_profile_batch_kernel(McBatchArgs a) {
    const int lane = (int)(threadIdx.x & 63);
    bool alive = false, exhausted = false;
    McPhoton p{};
    p.dz = 1.;
    p.thr = p.mfp = 1.;
    int slab = 0;                    // the lane's slab: its photon's, and its partial sums'
    const McScene *sc = a.slabs;     // = a.slabs + slab
    double acc_r = 0., acc_t = 0.;   // totals-only: the lane's sums for `slab`
    unsigned long long nev = 0;
    // the wave's current run: photon ids [pool, pool + pool_left) of slab run_slab
    uint64_t pool = 0;
    int pool_left = 0, run_slab = 0;
    for (;;) {
        // refill lanes whose photon has finished
        if (!exhausted) {
            const uint64_t need = __builtin_amdgcn_ballot_w64(!alive);
            if (need) {
                if (pool_left == 0) {
                    unsigned long long item = 0;
                    if (lane == 0) item = atomicAdd(a.next, 1ull);
                    item = __shfl(item, 0);
                    if (item < a.nruns) {
                        run_slab = (int)(item / a.runs_per_slab);
                        pool = (item % a.runs_per_slab) * (uint64_t)kMcPool;
                        const uint64_t rem = a.nphotons - pool;
                        pool_left = (int)(rem < (uint64_t)kMcPool ? rem : (uint64_t)kMcPool);
                    } else {
                        exhausted = true;
                    }
                }
                const int rank = __builtin_popcountll(need & ((1ull << lane) - 1ull));
                const bool take = !alive && rank < pool_left;
                if (!RINGS) flush_totals(take && slab != run_slab && (acc_r != 0. || acc_t != 0.), slab, acc_r, acc_t, a.tot, lane);
                if (take) {
                    slab = run_slab;
                    sc = a.slabs + slab;
                    mc_photon_start(*sc, a.seed, pool + (uint64_t)rank, p);
                    alive = true;
                }
                const int used = __builtin_popcountll(need) < pool_left ? __builtin_popcountll(need) : pool_left;
                pool += (uint64_t)used;
                pool_left -= used;
            }
        }
        if (__builtin_amdgcn_ballot_w64(alive) == 0) break;
        if (!alive) continue;
        ++nev;
        alive = mc_walk_event(*sc, p, [&](bool top, int seg, double w) {
            if (RINGS) {
                atomicAdd((top ? a.refl : a.trans) + (size_t)slab * (size_t)a.nsegments + (size_t)seg, w);
            } else {
                if (top)
                    acc_r += w;
                else
                    acc_t += w;
            }
        });
    }
    if (!RINGS) flush_totals(acc_r != 0. || acc_t != 0., slab, acc_r, acc_t, a.tot, lane);
    if (a.events) atomicAdd(a.events, nev);
}

}  // namespace

void run_mc_profile_batch(const McScene *scenes, int nslabs, uint64_t nphotons, uint64_t seed, double *refl,
                          double *trans, double *total_r, double *total_t, uint64_t *events, hipStream_t stream) {
    if (nslabs < 1 || nslabs > kMcMaxSlabs) throw Error(-1, "mc_profile_batch: 1..65536 slabs supported");
    const int nseg = scenes[0].nsegments;
    for (int s = 1; s < nslabs; ++s)
        if (scenes[s].nsegments != nseg) throw Error(-1, "mc_profile_batch: slabs differ in segments");
    if (nphotons > ((uint64_t)1 << 40)) throw Error(-1, "mc_profile_batch: at most 2^40 photons per slab");
    const bool rings = refl || trans;
    const size_t nring = rings ? (size_t)nslabs * nseg : 0;
    if (nphotons == 0) {
        if (refl) std::fill(refl, refl + nring, 0.);
        if (trans) std::fill(trans, trans + nring, 0.);
        std::fill(total_r, total_r + nslabs, 0.);
        std::fill(total_t, total_t + nslabs, 0.);
        if (events) *events = 0;
        return;
    }
    // one allocation for every tally: totals [nslabs][2], then the two ring arrays
    DevBuf<McScene> d_sc;
    DevBuf<double> d_tal;
    DevBuf<unsigned long long> d_cnt;
    d_sc.upload(scenes, (size_t)nslabs);
    const size_t ntal = 2 * (size_t)nslabs + 2 * nring;
    d_tal.alloc(ntal);
    d_cnt.alloc(2);
    MPSS_HIP(hipMemsetAsync(d_tal.ptr, 0, sizeof(double) * ntal, stream));
    MPSS_HIP(hipMemsetAsync(d_cnt.ptr, 0, sizeof(unsigned long long) * 2, stream));
    McBatchArgs a{};
    a.slabs = d_sc.ptr;
    a.nphotons = nphotons;
    a.seed = seed;
    a.runs_per_slab = (nphotons + (uint64_t)kMcPool - 1) / (uint64_t)kMcPool;
    a.nruns = a.runs_per_slab * (uint64_t)nslabs;
    a.next = d_cnt.ptr;
    a.tot = d_tal.ptr;
    a.refl = rings ? d_tal.ptr + 2 * (size_t)nslabs : nullptr;
    a.trans = rings ? a.refl + nring : nullptr;
    a.events = d_cnt.ptr + 1;
    a.nsegments = nseg;
    int dev = 0, ncu = 0;
    MPSS_HIP(hipGetDevice(&dev));
    MPSS_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev));
    // a 256-lane workgroup per run of kMcPool = 256 photons, up to 8 per CU
    const unsigned blocks = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ncu * 8, a.nruns));
    if (rings)
        hipLaunchKernelGGL(mc_profile_batch_kernel<true>, dim3(blocks), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(mc_profile_batch_kernel<false>, dim3(blocks), dim3(256), 0, stream, a);
    MPSS_HIP(hipGetLastError());
    std::vector<double> tal(ntal);
    unsigned long long cnt[2];
    MPSS_HIP(hipMemcpyAsync(tal.data(), d_tal.ptr, sizeof(double) * ntal, hipMemcpyDeviceToHost, stream));
    MPSS_HIP(hipMemcpyAsync(cnt, d_cnt.ptr, sizeof(cnt), hipMemcpyDeviceToHost, stream));
    MPSS_HIP(hipStreamSynchronize(stream));
    // normalise by photons and ring area (Render, :482-498), per slab as run_mc_profile does
    for (int s = 0; s < nslabs; ++s) {
        double tr = tal[2 * (size_t)s], tt = tal[2 * (size_t)s + 1];
        if (rings) {
            const McScene &sc = scenes[s];
            const double *r = tal.data() + 2 * (size_t)nslabs + (size_t)s * nseg, *t = r + nring;
            tr = tt = 0.;
            for (int i = 0; i < nseg; ++i) {
                const double sum = (double)(2 * i + 1) * sc.extent / sc.nsegments;
                const double h = sc.extent / sc.nsegments;
                const double area = kPbrtPi * sum * h;
                const double factor = (double)nphotons * area;
                tr += r[i];
                tt += t[i];
                if (refl) refl[(size_t)s * nseg + i] = r[i] / factor;
                if (trans) trans[(size_t)s * nseg + i] = t[i] / factor;
            }
        }
        total_r[s] = tr / (double)nphotons;
        total_t[s] = tt / (double)nphotons;
    }
    if (events) *events = cnt[1];
}

}  // namespace mpss
